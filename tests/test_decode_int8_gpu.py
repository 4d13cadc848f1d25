"""GPU: the decode fast path on Int8LinearWeight linears (csrc/decode.hip: llx_gemv_i8; llx/decode.py) - the weight-streaming GEMV on
int8 rows, weight-only and dynamic, with every prologue / epilogue of the bf16 kernel, against the oracle's int8 linear
(oracle/ref.py restating subclasses/int8.py:106-121 and int8_mm.py:93-118), kernel by kernel and as one Llama-3.1-8B-dimension layer
+ head decoding against a 4k-token cache."""
import functools

import pytest
import torch

from oracle import ref as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
MODES = [pytest.param(False, id="weight-only"), pytest.param(True, id="dynamic")]
SHAPES = [(1, 1024, (64,)), (3, 1040, (36,)), (4, 4096, (256, 64, 64)), (2, 14336, (128,)), (1, 4096, (38,))]


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


def _close(a, b, rel, name):
    scale = b.abs().max().item()
    err = (a - b).abs().max().item()
    assert err <= rel * scale + 1e-6, f"{name}: max err {err:.4e} vs scale {scale:.4e} (allowed {rel * scale:.4e})"


@functools.lru_cache(maxsize=None)
def _qweight(name, n, k, std=0.05):
    """(int8 rows, bf16 per-row scales) of a seeded bf16 matrix, as Int8LinearWeight.from_float makes them."""
    return O.quantize_int8_rowwise(O.randn(name, (n, k), std).to(BF))


@functools.lru_cache(maxsize=None)
def _operands(M, K_, ns):
    qs = [_qweight(f"g8_w{i}_{K_}_{n}", n, K_) for i, n in enumerate(ns)]
    x = O.randn(f"g8_x{M}_{K_}", (M, K_), 1.0).to(BF)
    nw = (1 + O.randn(f"g8_n{K_}", (K_,), 0.1)).to(BF)
    res = O.randn(f"g8_r{M}_{sum(ns)}", (M, sum(ns)), 1.0).to(BF)
    return qs, x, nw, res


def _dev(qs, cuda):
    return dict(ws=[q.to(cuda) for q, _ in qs], wscale=[s.to(cuda) for _, s in qs])


@pytest.mark.parametrize("M,K_,ns", SHAPES)
def test_gemv_i8_dynamic_is_bit_exact(K, cuda, M, K_, ns):
    """Dynamic int8 activations: the prologue's quantiser is int8_quant.hip's, the int32 sums do not depend on their order and the
    dequantisation has the reference's two fp32 products - without a fused norm the output is the oracle's bit for bit (plain and
    + residual).  With the fused norm the on-chip sum of squares can move a normalised value by one bf16 ulp and with it an int8 code:
    the bf16 GEMV tests' 1 % bar.  K with a partly filled last 1024-element piece (1040), three tokens on the 4-token build, ragged N."""
    qs, x, nw, res = _operands(M, K_, ns)
    wi, sc = torch.cat([q for q, _ in qs]), torch.cat([s for _, s in qs])
    w = _dev(qs, cuda)
    want = O.int8_linear(x, wi, sc, dynamic=True)
    got = K.gemv(x=x.to(cuda), dynamic=True, **w)
    assert got.dtype is BF and got.shape == want.shape
    assert torch.equal(got.cpu(), want), f"dynamic int8 gemv: {(got.cpu().float() - want.float()).abs().max().item():.4e} off the bit-exact target"
    got_r = K.gemv(x=x.to(cuda), dynamic=True, epilogue=K.GV_RESIDUAL, res=res.to(cuda), **w)
    assert torch.equal(got_r.cpu(), (want.float() + res.float()).to(BF)), "dynamic int8 gemv + residual"
    xin = O.rmsnorm(x, nw, 1e-5)
    want_n = O.int8_linear(xin, wi, sc, dynamic=True).float()
    got_n = K.gemv(x=x.to(cuda), dynamic=True, norm=(nw.to(cuda), 1e-5), **w)
    _close(got_n.float().cpu(), want_n, 0.01, "norm + dynamic int8 gemv")
    got_nr = K.gemv(x=x.to(cuda), dynamic=True, norm=(nw.to(cuda), 1e-5), epilogue=K.GV_RESIDUAL, res=res.to(cuda), **w)
    _close(got_nr.float().cpu(), want_n.to(BF).float() + res.float(), 0.01, "norm + dynamic int8 gemv + residual")
    assert torch.equal(got, K.gemv(x=x.to(cuda), dynamic=True, **w))
    assert torch.equal(got_n, K.gemv(x=x.to(cuda), dynamic=True, norm=(nw.to(cuda), 1e-5), **w))


@pytest.mark.parametrize("M,K_,ns", SHAPES)
@pytest.mark.parametrize("norm", [False, True])
def test_gemv_i8_weight_only(K, cuda, M, K_, ns, norm):
    """Weight-only: bf16(bf16(x @ W_i8^T) * scale) (subclasses/int8.py:118), fp32 accumulation in another order than the reference's."""
    qs, x, nw, res = _operands(M, K_, ns)
    wi, sc = torch.cat([q for q, _ in qs]), torch.cat([s for _, s in qs])
    w = _dev(qs, cuda)
    xin = O.rmsnorm(x, nw, 1e-5) if norm else x
    want = ((xin.float() @ wi.float().T).to(BF) * sc).float()
    nd = (nw.to(cuda), 1e-5) if norm else None
    got = K.gemv(x=x.to(cuda), norm=nd, **w)
    assert got.dtype is BF and got.shape == want.shape
    _close(got.float().cpu(), want, 0.01, "weight-only int8 gemv")
    got_r = K.gemv(x=x.to(cuda), norm=nd, epilogue=K.GV_RESIDUAL, res=res.to(cuda), **w)
    _close(got_r.float().cpu(), want.to(BF).float() + res.float(), 0.01, "weight-only int8 gemv + residual")
    assert torch.equal(got, K.gemv(x=x.to(cuda), norm=nd, **w))


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("dynamic", MODES)
def test_gemv_i8_swiglu_and_lora(K, cuda, M, dynamic):
    """gate|up on int8 rows with the SwiGLU epilogue, without and with LoRA adapters on both members: the dequantised base is rounded to
    bf16, the adapter term (t = rmsnorm(x) @ [A1; A3]^T from the bf16 kernel on the un-quantised x) is added in fp32 and the sum is
    rounded once (modelling/lora.py:41-43)."""
    D, I, r = 512, 1792, 16
    (q1, s1), (q3, s3) = (_qweight(f"s8_w{i}", I, D) for i in (1, 3))
    a1, a3 = (O.randn(f"s8_a{i}", (r, D), 0.05).to(BF) for i in (1, 3))
    b1, b3 = (O.randn(f"s8_b{i}", (I, r), 0.05).to(BF) for i in (1, 3))
    x = O.randn(f"s8_x{M}", (M, D), 1.0).to(BF)
    nw = (1 + O.randn("s8_n", (D,), 0.1)).to(BF)
    xb = O.rmsnorm(x, nw, 1e-5)
    xn = xb.float()
    w = dict(ws=[q1.to(cuda), q3.to(cuda)], wscale=[s1.to(cuda), s3.to(cuda)], dynamic=dynamic)
    for lora in (False, True):
        g = O.int8_linear(xb, q1, s1, dynamic=dynamic).float() + (2.0 * (xn @ a1.float().T) @ b1.float().T if lora else 0)
        u = O.int8_linear(xb, q3, s3, dynamic=dynamic).float() + (2.0 * (xn @ a3.float().T) @ b3.float().T if lora else 0)
        want = torch.nn.functional.silu(g.to(BF).float()).to(BF).float() * u.to(BF).float()
        lo = None
        if lora:
            t = K.gemv([a1.to(cuda), a3.to(cuda)], x.to(cuda), norm=(nw.to(cuda), 1e-5))
            lo = ([b1.to(cuda), b3.to(cuda)], t, 2.0)
        h = K.gemv(x=x.to(cuda), norm=(nw.to(cuda), 1e-5), epilogue=K.GV_SWIGLU, lora=lo, **w)
        assert h.shape == (M, I)
        _close(h.float().cpu(), want, 0.02, f"int8 swiglu lora={lora}")


@pytest.mark.parametrize("M", [1, 2, 4])
@pytest.mark.parametrize("dynamic", MODES)
def test_gemv_i8_qkv_rope_and_cache_scatter(K, cuda, M, dynamic):
    """The q|k|v projection of a decode step on int8 rows: RoPE on q and k with the table rows of the call, k / v written into the
    caches at input_pos, every other cache row untouched."""
    D, H, KVH, hd, Smax = 512, 4, 2, 128, 96
    qs = [_qweight("q8_wq", H * hd, D), _qweight("q8_wk", KVH * hd, D), _qweight("q8_wv", KVH * hd, D)]
    x = O.randn(f"q8_x{M}", (M, D), 1.0).to(BF)
    nw = (1 + O.randn("q8_n", (D,), 0.1)).to(BF)
    table = O.rope_table(O.TINY._replace(max_seq_len=Smax))
    pos = torch.tensor([70, 3, 95, 41][:M])
    xb = O.rmsnorm(x, nw, 1e-5)
    q, k, v = (O.int8_linear(xb, wi, sc, dynamic=dynamic).to(BF).view(1, M, -1, hd) for wi, sc in qs)
    q_want, k_want = O.rope_apply(q, table), O.rope_apply(k, table)
    kc = O.randn("q8_kc", (1, KVH, Smax, hd), 1.0).to(BF)
    vc = O.randn("q8_vc", (1, KVH, Smax, hd), 1.0).to(BF)
    kc_d, vc_d = kc.to(cuda), vc.to(cuda)
    got = K.gemv(x=x.to(cuda), norm=(nw.to(cuda), 1e-5), epilogue=K.GV_QKV, dynamic=dynamic,
                 qkv=(table.to(cuda), H * hd, KVH * hd, kc_d, vc_d, pos.to(cuda)), **_dev(qs, cuda))
    assert got.shape == (M, H * hd)
    _close(got.float().cpu().view(1, M, H, hd), q_want.float(), 0.01, "q with RoPE")
    others = torch.ones(Smax, dtype=torch.bool)
    others[pos] = False
    assert torch.equal(kc_d.cpu()[:, :, others], kc[:, :, others]) and torch.equal(vc_d.cpu()[:, :, others], vc[:, :, others]), "untouched cache rows"
    _close(kc_d.cpu()[:, :, pos].float(), k_want.transpose(1, 2).float(), 0.01, "k cache rows")
    _close(vc_d.cpu()[:, :, pos].float(), v.transpose(1, 2).float(), 0.01, "v cache rows")


def test_gemv_i8_rejects(K, cuda):
    from llx._lib import LlxError

    wi, sc = _qweight("r8_w", 64, 1040)
    wb = O.randn("r8_wb", (64, 1040), 0.05).to(BF)
    x = O.randn("r8_x", (5, 1040), 1.0).to(BF)
    with pytest.raises(LlxError):  # one kind per call
        K.gemv([wb.to(cuda), wi.to(cuda)], x[:1].to(cuda), wscale=[sc.to(cuda), sc.to(cuda)])
    with pytest.raises(LlxError):  # K % 16 != 0
        K.gemv([wi[:, :1032].contiguous().to(cuda)], x[:1, :1032].contiguous().to(cuda), wscale=[sc.to(cuda)])
    with pytest.raises(LlxError):  # M > 4 belongs to the MFMA GEMM
        K.gemv([wi.to(cuda)], x.to(cuda), wscale=[sc.to(cuda)], dynamic=True)


def test_layer_with_mixed_group_takes_the_generic_path(cuda):
    """(w1, w3) share one launch: a layer whose pair mixes kinds is not taken; groups of different kinds next to each other are."""
    import llx.decode as D
    from subclasses import quantize_linear_
    from tests.util import bf16_params, build_model

    cfg = O.TINY._replace(num_layers=1, vocab_size=8, max_seq_len=64)
    pb, _ = bf16_params(O.init_params(cfg))
    model = build_model(cfg, pb, "cpu")
    model.build_cache(inference=True)
    layer = model.layers[0]
    quantize_linear_(layer.feed_forward.w1, "int8")
    model = model.to(cuda).eval()
    x = model.tok_embeddings(torch.zeros(1, 1, dtype=torch.int64, device=cuda))
    mask = model.causal_mask[None, None, torch.tensor([5], device=cuda)]
    assert D._plain(layer.feed_forward.w1) == D.KIND_I8W and D._plain(layer.feed_forward.w3) == D.KIND_BF16
    assert not D.layer_ok(layer, x, mask)
    quantize_linear_(layer.feed_forward.w3, "int8")  # the pair of one kind, q|k|v / wo / w2 still bf16
    assert D.layer_ok(layer, x, mask)
    quantize_linear_(layer.attention.wk, "int8", dynamic_int8_act=True)
    assert not D.layer_ok(layer, x, mask)


@functools.lru_cache(maxsize=None)
def _layer_params(lora):
    from tests.util import bf16_params

    cfg = O.LLAMA31_8B._replace(num_layers=1, max_seq_len=4352, vocab_size=8)
    p = O.init_params(cfg)
    if lora:
        p.update(O.init_lora(cfg, 16))
    pb, pf = bf16_params(p)
    quant = {f"layers.0.{suf}": O.quantize_int8_rowwise(pb[f"layers.0.{suf}.weight"]) for suf in O.LINEAR_SUFFIXES}
    return cfg, pb, pf, quant


@pytest.mark.parametrize("lora", [False, True])
@pytest.mark.parametrize("dynamic", MODES)
def test_decode_int8_layer_at_8b_dimensions(cuda, dynamic, lora):
    """One Llama-3.1-8B-dimension layer quantised to int8 + norm + bf16 head decoding 1 token, then 3 tokens in one call, against a cache
    holding 4100 positions.  The layer takes the weight-streaming path; the generic inference path (MFMA GEMMs at M <= 4) on the same
    device state agrees within 3 %; a weight-only layer agrees with the oracle within the bf16 test's 3 % and leaves no bf16 image of
    its int8 matrices behind; a captured decode step replays to the eager logits.  Dynamic activations: the fp32 oracle and any bf16
    product flip a few int8 codes differently (tests/test_model_gpu.py:153-157), so the bar is the generic path's own error against the
    oracle, measured here: fast <= 1.5 x generic + 0.005 x scale.
    Measured max errors against the oracle, (fast path, generic path) / logit scale: dynamic 0.0993, 0.0993 / 3.81 at 1 token and
    0.1222, 0.1222 / 2.58 at 3 tokens; dynamic + LoRA 0.0904, 0.0904 / 3.87 and 0.1529, 0.1529 / 2.71 (the two paths round at the same
    points and land on the same worst logit); weight-only 0.0180, 0.0155 / 3.73 and 0.0190, 0.0190 / 2.65; weight-only + LoRA
    0.0308, 0.0308 / 3.87 and 0.0175, 0.0201 / 2.69."""
    import llx.decode as D
    import oracle.ref as R
    from tests.util import build_model

    t0 = 4100
    cfg, pb, pf0, quant = _layer_params(lora)
    Smax = cfg.max_seq_len
    pf = dict(pf0)
    for key, (q, sc) in quant.items():  # the oracle's weights: quantised exactly as Int8LinearWeight.from_float does (scales in bf16)
        pf.pop(key + ".weight")
        pf[key + ".int_data"], pf[key + ".scale"], pf[key + ".dynamic"] = q, sc.float(), dynamic
    model = build_model(cfg, pb, "cpu", lora_rank=16 if lora else 0, lora_alpha=32.0, quantize="int8", quantize_kwargs=dict(dynamic_int8_act=dynamic))
    model.build_cache(inference=True)
    model = model.to(cuda).eval()
    layer = model.layers[0]
    assert torch.equal(layer.attention.wq.weight.int_data.cpu(), quant["layers.0.attention.wq"][0])
    kc0 = O.randn("dl_kc", (1, cfg.num_kv_heads, Smax, 128), 1.0).to(BF)
    vc0 = O.randn("dl_vc", (1, cfg.num_kv_heads, Smax, 128), 1.0).to(BF)
    kc0[:, :, t0:], vc0[:, :, t0:] = 0, 0
    cache_mod = layer.attention.kv_cache
    cache = {0: (kc0.float().clone(), vc0.float().clone())}
    tokens = O.randint("dl_tok", (1, 4), 0, 8)
    scale = 2.0 if lora else 1.0

    def reset():
        cache_mod.k_cache.copy_(kc0)
        cache_mod.v_cache.copy_(vc0)

    def oracle_step(tok, pos):
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

    calls = ((tokens[:, :1], torch.tensor([t0])), (tokens[:, 1:], torch.tensor([t0 + 1, t0 + 2, t0 + 3])))
    want = [oracle_step(tok, pos) for tok, pos in calls]
    fast, slow = [], []
    with torch.no_grad():
        reset()
        for tok, pos in calls:
            assert D.layer_ok(layer, model.tok_embeddings(tok.to(cuda)), model.causal_mask[None, None, pos.to(cuda)]), "int8 layer not on the fast path"
            fast.append(model(tok.to(cuda), input_pos=pos.to(cuda)).float().cpu())
        # one captured decode step replays to the eager logits
        tok_d, pos_d = calls[0][0].to(cuda), calls[0][1].to(cuda)
        reset()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eager = model(tok_d, input_pos=pos_d)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            logits = model(tok_d, input_pos=pos_d)
        reset()
        logits.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(logits, eager), "graph replay of a decode step differs from the eager call"
        assert torch.equal(eager.float().cpu(), fast[0])
        if not dynamic:  # the weight-only fast path streams the int8 rows themselves
            for m in (layer.attention.wq, layer.attention.wo, layer.feed_forward.w1, layer.feed_forward.w2):
                assert "bf16" not in m.weight.int_data.__dict__.get("_llx_cache", {}), "a decode call built the bf16 image of an int8 matrix"
        # the generic inference path on the same device state
        reset()
        old = D.MAX_TOKENS
        D.MAX_TOKENS = 0
        try:
            for tok, pos in calls:
                slow.append(model(tok.to(cuda), input_pos=pos.to(cuda)).float().cpu())
        finally:
            D.MAX_TOKENS = old
    for i, (tok, pos) in enumerate(calls):
        at = f"at {pos.tolist()}"
        _close(fast[i], slow[i], 0.03, f"weight-streaming path vs generic inference path {at}")
        sc = want[i].abs().max().item()
        e_fast, e_slow = (fast[i] - want[i]).abs().max().item(), (slow[i] - want[i]).abs().max().item()
        print(f"[int8 decode dynamic={dynamic} lora={lora} {at}] fast err {e_fast:.4e}, generic err {e_slow:.4e}, scale {sc:.4e}")
        if dynamic:
            assert e_fast <= 1.5 * e_slow + 0.005 * sc, f"decode logits {at}: fast path err {e_fast:.4e} vs generic path err {e_slow:.4e} against the oracle (scale {sc:.4e})"
        else:
            _close(fast[i], want[i], 0.03, f"decode logits {at}")
