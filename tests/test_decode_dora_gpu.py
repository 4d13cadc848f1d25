"""GPU: the decode fast path of DoRA linears (csrc/decode.hip: llx_gemv_bf16_dora; llx/decode.py; llx/ops.py: dora_scale_cached).

Kernel tests: the expected values are restated in fp32 with the kernel's rounding points - t = bf16(x^ A^T) with x^ = x or rmsnorm(x)
rounded to bf16, z = bf16(x^ W^T + s t B^T), v = bf16(z c), then the epilogue - so only summation order separates the two sides; the
bars are those of tests/test_decode_gpu.py for the same epilogues (0.01 plain / residual / q|k|v, 0.02 SwiGLU, 0.03 whole-model
logits), times max|want|.  c is drawn uniformly in [0.5, 2] per row and per segment: a missing factor, a wrong row or the wrong
segment's vector moves outputs by tens of per cent."""
import pytest
import torch

from oracle import ref as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
R_, S_ = 8, 2.0  # rank per member and alpha / rank of the kernel tests


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


def _close(a, b, rel, name):
    scale = b.abs().max().item()
    err = (a - b).abs().max().item()
    print(f"[{name}] max err {err:.4e}, bar {rel * scale:.4e}")
    assert err <= rel * scale + 1e-6, f"{name}: max err {err:.4e} vs scale {scale:.4e} (allowed {rel * scale:.4e})"


def _operands(tag, M, Kd, ns):
    """(ws, As, Bs, cs, x, norm weight) on the host, bf16."""
    ws = [O.randn(f"dd_w{i}_{tag}", (n, Kd), 0.05).to(BF) for i, n in enumerate(ns)]
    As = [O.randn(f"dd_a{i}_{tag}", (R_, Kd), 0.05).to(BF) for i, n in enumerate(ns)]
    Bs = [O.randn(f"dd_b{i}_{tag}", (n, R_), 0.05).to(BF) for i, n in enumerate(ns)]
    cs = [O.uniform(f"dd_c{i}_{tag}", (n,), 0.5, 2.0).to(BF) for i, n in enumerate(ns)]
    x = O.randn(f"dd_x_{tag}", (M, Kd), 1.0).to(BF)
    nw = (1 + O.randn(f"dd_n_{tag}", (Kd,), 0.1)).to(BF)
    return ws, As, Bs, cs, x, nw


def _xhat(x, nw, norm):
    return (O.rmsnorm(x, nw, 1e-5).to(BF) if norm else x).float()


def _want(xh, ws, As, Bs, cs):
    """Per member: v = bf16(bf16(x^ W^T + s bf16(x^ A^T) B^T) c), fp32 [M, n_s]."""
    out = []
    for w, a, b, c in zip(ws, As, Bs, cs):
        t = (xh @ a.float().T).to(BF).float()
        z = (xh @ w.float().T + S_ * (t @ b.float().T)).to(BF).float()
        out.append((z * c.float()).to(BF).float())
    return out


def _dev(ts, cuda):
    return [t.to(cuda) for t in ts]


def _run(K, cuda, ws, As, Bs, cs, x, nw, norm, **kw):
    """The two launches of the decode path: t = x^ A^T, then the main stream with the B factors and (cs given) the row factors."""
    nm = (nw.to(cuda), 1e-5) if norm else None
    t = K.gemv(_dev(As, cuda), x.to(cuda), norm=nm)
    return K.gemv(_dev(ws, cuda), x.to(cuda), norm=nm, lora=(_dev(Bs, cuda), t, S_), colscale=_dev(cs, cuda) if cs is not None else None, **kw)


# ------------------------------------------------------------------------------------------------- 1. plain and residual
@pytest.mark.parametrize("M,Kd,ns", [(1, 512, (512, 128, 128)), (2, 1792, (512,)), (3, 520, (36,)), (4, 4096, (256, 64, 64))])
@pytest.mark.parametrize("norm", [False, True])
def test_dora_gemv_plain_and_residual(K, cuda, M, Kd, ns, norm):
    """Three segments with three factor vectors; the 4-row build with 3 live rows, ragged N, K that is not a whole step; a second launch
    is bit-identical."""
    ws, As, Bs, cs, x, nw = _operands(f"p{M}_{Kd}", M, Kd, ns)
    want = torch.cat(_want(_xhat(x, nw, norm), ws, As, Bs, cs), 1)
    got = _run(K, cuda, ws, As, Bs, cs, x, nw, norm)
    assert got.shape == want.shape
    _close(got.float().cpu(), want, 0.01, f"dora gemv M={M} K={Kd} norm={norm}")
    res = O.randn(f"dd_r{M}_{sum(ns)}", (M, sum(ns)), 1.0).to(BF)
    got_r = _run(K, cuda, ws, As, Bs, cs, x, nw, norm, epilogue=K.GV_RESIDUAL, res=res.to(cuda))
    _close(got_r.float().cpu(), (want + res.float()).to(BF).float(), 0.01, f"dora gemv + residual M={M} K={Kd} norm={norm}")
    assert torch.equal(got, _run(K, cuda, ws, As, Bs, cs, x, nw, norm))


# ------------------------------------------------------------------------------------------------- 2. neutral factor
def test_dora_gemv_neutral_factor_is_the_lora_build(K, cuda):
    """colscale of ones = the same call without colscale, bit for bit, through all four epilogues (and both caches): the new path shares
    every other rounding point with the LoRA build."""
    D, H, KVH, hd, Smax, M = 512, 4, 1, 128, 96, 3
    ns = (H * hd, KVH * hd, KVH * hd)
    ws, As, Bs, _, x, nw = _operands("neutral", M, D, ns)
    ones = [torch.ones(n, dtype=BF) for n in ns]
    res = O.randn("dd_r_neutral", (M, sum(ns)), 1.0).to(BF).to(cuda)
    for kw in (dict(), dict(epilogue=K.GV_RESIDUAL, res=res)):
        assert torch.equal(_run(K, cuda, ws, As, Bs, ones, x, nw, True, **kw), _run(K, cuda, ws, As, Bs, None, x, nw, True, **kw)), kw
    table = O.rope_table(O.TINY._replace(max_seq_len=Smax)).to(cuda)
    pos = torch.tensor([70, 0, 95], device=cuda)
    outs = []
    for c in (ones, None):
        kc = O.randn("dd_kc_neutral", (1, KVH, Smax, hd), 1.0).to(BF).to(cuda)
        vc = O.randn("dd_vc_neutral", (1, KVH, Smax, hd), 1.0).to(BF).to(cuda)
        q = _run(K, cuda, ws, As, Bs, c, x, nw, True, epilogue=K.GV_QKV, qkv=(table, H * hd, KVH * hd, kc, vc, pos))
        outs.append((q, kc, vc))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    g = _operands("neutral_gu", M, D, (776, 776))
    assert torch.equal(_run(K, cuda, g[0], g[1], g[2], [torch.ones(776, dtype=BF)] * 2, g[4], g[5], True, epilogue=K.GV_SWIGLU),
                       _run(K, cuda, g[0], g[1], g[2], None, g[4], g[5], True, epilogue=K.GV_SWIGLU))


# ------------------------------------------------------------------------------------------------- 3. SwiGLU
@pytest.mark.parametrize("M", [1, 3])
def test_dora_gemv_swiglu(K, cuda, M):
    """gate and up each with their own A, B and c; h = bf16(bf16(silu(g)) u) on the scaled bf16 g and u."""
    D, I = 512, 1796
    ws, As, Bs, cs, x, nw = _operands(f"sw{M}", M, D, (I, I))
    g, u = _want(_xhat(x, nw, True), ws, As, Bs, cs)
    want = (torch.nn.functional.silu(g).to(BF).float() * u).to(BF).float()
    h = _run(K, cuda, ws, As, Bs, cs, x, nw, True, epilogue=K.GV_SWIGLU)
    assert h.shape == (M, I)
    _close(h.float().cpu(), want, 0.02, f"dora swiglu M={M}")


# ------------------------------------------------------------------------------------------------- 4. q|k|v
@pytest.mark.parametrize("pos", [[95], [0, 95], [70, 0, 95, 41]])
def test_dora_gemv_qkv_rope_and_cache(K, cuda, pos):
    """q = RoPE of the scaled rows; the k (rotated) and v cache rows at the positions; every other cache element keeps its sentinel."""
    D, H, KVH, hd, Smax, M = 512, 4, 1, 128, 96, len(pos)
    ns = (H * hd, KVH * hd, KVH * hd)
    ws, As, Bs, cs, x, nw = _operands(f"qkv{M}", M, D, ns)
    q, k, v = _want(_xhat(x, nw, True), ws, As, Bs, cs)
    table = O.rope_table(O.TINY._replace(max_seq_len=Smax))
    q_want = O.rope_apply(q.to(BF).view(1, M, H, hd), table).float()
    k_want = O.rope_apply(k.to(BF).view(1, M, KVH, hd), table).float().transpose(1, 2)
    v_want = v.view(1, M, KVH, hd).transpose(1, 2)
    sentinel = 7.25
    kc = torch.full((1, KVH, Smax, hd), sentinel, dtype=BF, device=cuda)
    vc = torch.full((1, KVH, Smax, hd), sentinel, dtype=BF, device=cuda)
    p = torch.tensor(pos)
    got = _run(K, cuda, ws, As, Bs, cs, x, nw, True, epilogue=K.GV_QKV, qkv=(table.to(cuda), H * hd, KVH * hd, kc, vc, p.to(cuda)))
    assert got.shape == (M, H * hd)
    _close(got.float().cpu().view(1, M, H, hd), q_want, 0.01, f"dora q with RoPE M={M}")
    _close(kc.cpu()[:, :, p].float(), k_want, 0.01, f"dora k cache rows M={M}")
    _close(vc.cpu()[:, :, p].float(), v_want, 0.01, f"dora v cache rows M={M}")
    others = torch.ones(Smax, dtype=torch.bool)
    others[p] = False
    assert (kc.cpu()[:, :, others] == sentinel).all() and (vc.cpu()[:, :, others] == sentinel).all(), "a cache row outside the positions was written"


# ------------------------------------------------------------------------------------------------- 5. rejections
def test_dora_gemv_rejections(K, cuda):
    from llx._lib import LlxError

    ws, As, Bs, cs, x, nw = _operands("rej", 1, 512, (64,))
    with pytest.raises(LlxError):  # int8 weights
        K.gemv([torch.zeros(64, 512, dtype=torch.int8, device=cuda)], x.to(cuda), wscale=[torch.ones(64, dtype=BF, device=cuda)], colscale=_dev(cs, cuda))
    with pytest.raises(LlxError):  # wrong length
        K.gemv(_dev(ws, cuda), x.to(cuda), colscale=[torch.ones(60, dtype=BF, device=cuda)])
    with pytest.raises(LlxError):  # wrong dtype
        K.gemv(_dev(ws, cuda), x.to(cuda), colscale=[torch.ones(64, dtype=torch.float32, device=cuda)])
    with pytest.raises(LlxError):  # one vector for two weights
        K.gemv(_dev(ws + ws, cuda), x.to(cuda), colscale=_dev(cs, cuda))


# ------------------------------------------------------------------------------------------------- models
def _dora_model(cfg, pb, rank, alpha, inference=True):
    """Llama with DoRA on every layer linear (apply_linear_adapter_(model.layers, "dora")), factors and m from the parameter dict; on the host."""
    from modelling import Llama, apply_linear_adapter_
    from tests.util import to_model_config

    model = Llama(to_model_config(cfg)).bfloat16()
    model.load_state_dict({k: v for k, v in pb.items() if "lora_" not in k and not k.endswith(".m")})
    apply_linear_adapter_(model.layers, "dora", rank=rank, alpha=alpha)
    with torch.no_grad():
        for name, mod in model.layers.named_modules():
            if f"layers.{name}.lora_a" in pb:
                mod.lora_a.copy_(pb[f"layers.{name}.lora_a"])
                mod.lora_b.copy_(pb[f"layers.{name}.lora_b"])
                mod.m.copy_(pb[f"layers.{name}.m"])
    model.build_cache(inference=inference)
    return model


def _tiny_params(cfg):
    from tests.util import bf16_params

    p = O.init_params(cfg)
    p.update(O.init_lora(cfg, 8))  # lora_b ~ N(0, 0.01^2): non-zero
    p.update(O.init_dora_m(p, cfg))
    return bf16_params(p)


def _generic(fn):
    """fn() with the decode fast path switched off (the generic inference path), as test_decode_layer_at_8b_dimensions does."""
    import llx.decode as D

    old = D.MAX_TOKENS
    D.MAX_TOKENS = 0
    try:
        return fn()
    finally:
        D.MAX_TOKENS = old


def _zero_caches(model):
    for layer in model.layers:
        layer.attention.kv_cache.k_cache.zero_()
        layer.attention.kv_cache.v_cache.zero_()


# ------------------------------------------------------------------------------------------------- 6. tiny model
def test_dora_tiny_model_fast_and_generic_against_oracle(cuda):
    """O.TINY with DoRA r = 8 (alpha / r = 1, the scale of O.llama_forward_cached) on every layer linear: a 40-token prefill and three decode
    steps on the fast path, then on the generic path, each against the oracle on the fp32 parameters (O.linear takes the DoRA branch)."""
    import llx.decode as D
    from modelling import LoRALinear

    cfg = O.TINY
    pb, pf = _tiny_params(cfg)
    model = _dora_model(cfg, pb, 8, 8.0).to(cuda).eval()
    assert all(m.lora_b.abs().max() > 0 for m in model.layers.modules() if hasattr(m, "lora_b"))
    tokens = O.randint("dd_tiny_tok", (1, 43), 0, cfg.vocab_size)
    calls = [(tokens[:, :40], torch.arange(40))] + [(tokens[:, 40 + i : 41 + i], torch.tensor([40 + i])) for i in range(3)]
    cache = O.new_cache(cfg)
    want = [O.llama_forward_cached(tok, pf, cfg, cache, pos) for tok, pos in calls]
    with torch.no_grad():
        for tok, pos in ((tokens[:, :1], torch.tensor([5])), (tokens[:, :4], torch.tensor([5, 6, 7, 8]))):
            assert D.layer_ok(model.layers[0], model.tok_embeddings(tok.to(cuda)), model.causal_mask[None, None, pos.to(cuda)])

        def run():
            _zero_caches(model)
            return [model(tok.to(cuda), input_pos=pos.to(cuda)).float().cpu() for tok, pos in calls]

        fast = run()
        slow = _generic(run)
    for i, (f, s, w) in enumerate(zip(fast, slow, want)):
        _close(f, w, 0.03, f"tiny DoRA call {i}: fast path vs oracle")
        _close(s, w, 0.03, f"tiny DoRA call {i}: generic path vs oracle")
        _close(f, s, 0.03, f"tiny DoRA call {i}: fast path vs generic path")
    # a gate|up group with a DoRA w1 and a LoRA w3 is not streamed
    w3 = model.layers[1].feed_forward.w3
    w3.__class__ = LoRALinear
    del w3.m
    x1 = model.tok_embeddings(tokens[:, :1].to(cuda))
    mask1 = model.causal_mask[None, None, torch.tensor([5], device=cuda)]
    assert not D.layer_ok(model.layers[1], x1, mask1) and D.layer_ok(model.layers[0], x1, mask1)


# ------------------------------------------------------------------------------------------------- 7. one 8B-dimension layer + head
def test_dora_decode_layer_at_8b_dimensions(cuda):
    """The DoRA twin of test_decode_layer_at_8b_dimensions: r = 16, alpha / r = 2, a cache holding 4100 positions, one token and then three
    in one call against the oracle, then the generic path.  The first step builds the cached factors: what stays allocated is c (2 B)
    and ||W||^2 (4 B) per output row, about 0.1 % of the weight bytes, and no second copy of any weight."""
    import llx.decode as D
    import oracle.ref as R
    from tests.util import bf16_params

    t0, Smax, scale = 4100, 4352, 2.0
    cfg = O.LLAMA31_8B._replace(num_layers=1, max_seq_len=Smax, vocab_size=8)
    p = O.init_params(cfg)
    p.update(O.init_lora(cfg, 16))
    p.update(O.init_dora_m(p, cfg))
    pb, pf = bf16_params(p)
    model = _dora_model(cfg, pb, 16, 32.0).to(cuda).eval()
    kc0 = O.randn("dl_kc", (1, cfg.num_kv_heads, Smax, 128), 1.0).to(BF)
    vc0 = O.randn("dl_vc", (1, cfg.num_kv_heads, Smax, 128), 1.0).to(BF)
    kc0[:, :, t0:], vc0[:, :, t0:] = 0, 0
    cache_mod = model.layers[0].attention.kv_cache
    cache_mod.k_cache.copy_(kc0)
    cache_mod.v_cache.copy_(vc0)
    cache = {0: (kc0.float().clone(), vc0.float().clone())}
    tokens = O.randint("dl_tok", (1, 4), 0, 8)

    def oracle_step(tok, pos):  # O.llama_forward_cached with the adapter scale threaded through
        L_ = tok.shape[1]
        x = torch.nn.functional.embedding(tok, pf["tok_embeddings.weight"])
        table = R.rope_table(cfg)[:L_]
        mask = torch.tril(torch.ones(Smax, Smax, dtype=torch.bool))[None, None, pos]
        pre = "layers.0."
        h = R.rmsnorm(x, pf[pre + "attention_norm.weight"])
        q = R.linear(h, pf, pre + "attention.wq", scale).view(1, L_, cfg.num_heads, 128)
        k = R.linear(h, pf, pre + "attention.wk", scale).view(1, L_, cfg.num_kv_heads, 128)
        v = R.linear(h, pf, pre + "attention.wv", scale).view(1, L_, cfg.num_kv_heads, 128)
        q, k, v = R.rope_apply(q, table).transpose(1, 2), R.rope_apply(k, table).transpose(1, 2), v.transpose(1, 2)
        kc, vc = cache[0]
        kc[:, :, pos], vc[:, :, pos] = k, v
        o = R.sdpa(q, kc, vc, mask).transpose(1, 2).reshape(1, L_, -1)
        x = x + R.linear(o, pf, pre + "attention.wo", scale)
        x = x + R.feed_forward(R.rmsnorm(x, pf[pre + "ffn_norm.weight"]), pf, pre + "feed_forward.", scale)
        return torch.nn.functional.linear(R.rmsnorm(x, pf["norm.weight"]), pf["output.weight"])

    lins = [m for m in model.layers.modules() if hasattr(m, "lora_b")]
    weight_bytes = sum(m.weight.numel() * 2 for m in lins)
    rows = sum(m.out_features for m in lins)
    steps = ((tokens[:, :1], torch.tensor([t0])), (tokens[:, 1:], torch.tensor([t0 + 1, t0 + 2, t0 + 3])))
    with torch.no_grad():
        for i, (tok, pos) in enumerate(steps):
            assert D.layer_ok(model.layers[0], model.tok_embeddings(tok.to(cuda)), model.causal_mask[None, None, pos.to(cuda)])
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            got = model(tok.to(cuda), input_pos=pos.to(cuda)).float().cpu()
            if i == 0:
                torch.cuda.synchronize()
                grown = torch.cuda.memory_allocated() - before
                print(f"[8B DoRA layer] first step keeps {grown} B, weights {weight_bytes} B ({100 * grown / weight_bytes:.3f} %)")
                assert grown < 0.01 * weight_bytes
                for m in lins:
                    kept = m.weight.__dict__["_llx_cache"]
                    assert set(kept) == {"dora_c", "wn2m"}, set(kept)
                    c, wn2 = kept["dora_c"][1], kept["wn2m"][1]
                    assert c.dtype is BF and c.shape == (m.out_features,) and wn2.dtype is torch.float32 and wn2.shape == (m.out_features,)
                assert 6 * rows < 0.002 * weight_bytes
            _close(got, oracle_step(tok, pos), 0.03, f"8B DoRA decode logits at {pos.tolist()}")
            _close(cache_mod.k_cache[:, :, pos.to(cuda)].float().cpu(), cache[0][0][:, :, pos], 0.02, "k cache rows written by the fused projection")

        def first():
            cache_mod.k_cache.copy_(kc0)
            cache_mod.v_cache.copy_(vc0)
            return model(tokens[:, :1].to(cuda), input_pos=torch.tensor([t0], device=cuda)).float().cpu()

        fast = first()
        slow = _generic(first)
    _close(fast, slow, 0.03, "8B DoRA: weight-streaming path vs generic inference path")


# ------------------------------------------------------------------------------------------------- 8. cache behaviour
def test_dora_scale_cache_behaviour(cuda, monkeypatch):
    """Which forwards build a row factor (K.dora_colscale is counted), what invalidates it, and that a forward with grad enabled is
    untouched by all of it."""
    import llx.decode as D
    from llx import kernels as K_

    cfg = O.TINY
    pb, _ = _tiny_params(cfg)
    model = _dora_model(cfg, pb, 8, 8.0, inference=False).to(cuda).eval()
    for n, q in model.named_parameters():
        q.requires_grad_("lora_" in n or n.endswith(".m"))
    n_lin = 7 * cfg.num_layers
    calls = []
    real = K_.dora_colscale
    monkeypatch.setattr(K_, "dora_colscale", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def built():
        n = len(calls)
        calls.clear()
        return n

    tokens = O.randint("dd_cache_tok", (1, 256), 0, cfg.vocab_size).to(cuda)
    labels = torch.roll(tokens, -1, 1)
    train = [q for n, q in model.named_parameters() if q.requires_grad]
    assert len(train) == 3 * n_lin  # lora_a, lora_b, m of every layer linear

    def loss_and_grads():
        for q in train:
            q.grad = None
        loss = model(tokens, labels=labels)
        loss.backward()
        return loss.detach().clone(), [q.grad.clone() for q in train]

    loss0, grads0 = loss_and_grads()
    built()
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    model.build_cache(inference=True)
    model = model.to(cuda).eval()
    tok, pos = tokens[:, :4], torch.arange(4, device=cuda)
    with torch.no_grad():
        first = model(tok, input_pos=pos)
        assert built() == n_lin, "the first forward builds one factor per DoRA linear"
        assert torch.equal(model(tok, input_pos=pos), first) and built() == 0, "the second forward builds nothing"
        model.layers[0].attention.wo.m.mul_(1.5)
        after = model(tok, input_pos=pos)
        assert built() == 1, "an in-place update of one m rebuilds exactly that linear"
        assert not torch.equal(after, first)
        fresh = _dora_model(cfg, pb, 8, 8.0)
        fresh.load_state_dict(model.state_dict())
        fresh = fresh.to(cuda).eval()
        assert torch.equal(fresh(tok, input_pos=pos), after), "logits of a fresh model holding the updated m"
        built()
        other = {k: (v * 1.25 if k.endswith(".m") else v.clone()) for k, v in sd0.items()}
        model.load_state_dict(other)
        loaded = model(tok, input_pos=pos)
        assert built() == n_lin and not torch.equal(loaded, first), "load_state_dict rebuilds every factor"
        model.load_state_dict(sd0)
        assert D.prepare(model) is model and built() == n_lin
        assert torch.equal(model(tok, input_pos=pos), first) and built() == 0, "prepare() leaves nothing to build"
        model.load_state_dict(sd0)  # (bumps every version: the generic path starts cold)
        cold = _generic(lambda: model(tok, input_pos=pos))
        assert built() == n_lin
        cached = _generic(lambda: model(tok, input_pos=pos))
        assert built() == 0 and torch.equal(cold, cached), "generic path: cold and cached calls agree bit for bit"
    for layer in model.layers:
        layer.attention.kv_cache = None
    loss1, grads1 = loss_and_grads()
    assert torch.equal(loss0, loss1) and all(torch.equal(a, b) for a, b in zip(grads0, grads1)), "the forward with grad enabled changed"


# ------------------------------------------------------------------------------------------------- 9. generate()
def test_dora_generate_equals_the_hand_loop(cuda):
    """Greedy generate() of 8 tokens on the tiny DoRA model = a hand loop of model(...) calls with lowest-index argmax."""
    cfg = O.TINY
    pb, _ = _tiny_params(cfg)
    model = _dora_model(cfg, pb, 8, 8.0).to(cuda).eval()
    P, n = 40, 8
    prompt = O.randint("generate_prompt", (1, P), 0, cfg.vocab_size).to(cuda)
    toks = []
    with torch.no_grad():
        last = model(prompt, input_pos=torch.arange(P, device=cuda))[0, -1:]
        for k in range(n):
            x = last.float()
            t = (x[0] == x[0].max()).nonzero()[0]  # lowest index among ties
            toks.append(t.view(1))
            if k < n - 1:
                last = model(t.view(1, 1), input_pos=torch.tensor([P + k], device=cuda))[0]
    want = torch.cat(toks)[None]
    got = model.generate(prompt, n)
    assert got.shape == (1, n) and torch.equal(got, want)
    assert len(set(got[0].tolist())) > 1
