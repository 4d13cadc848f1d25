"""GPU: attention dropout in training.  The keep bytes the kernels' own device function writes against the numpy restatement
(bit for bit); the dropped forward and backward against the float64 reference under the restated mask at the bars of
tests/attn_cases.py (checked for discriminating power on the CPU: tests/test_dropout_cases.py); one Attention block against a
float64 composition; the tiny model in train mode (determinism, checkpointing, eval, the dense causal mask= route); a captured
training step that draws a new mask on every replay; the rejections.

Shapes follow the tile geometry: forward and dQ work on 256 query rows per workgroup and 64-key tiles, dK/dV on 128 keys per
workgroup and 64-row query tiles.  S = 64 is one tile, 320 the size the adapter tests use, 577 = 9 * 64 + 1: three query blocks
(the last of 65 rows), a last key tile of one key, a ragged last 128-key block."""
import math

import pytest
import torch

from oracle import ref as O
from tests import attn_cases as C
from tests import dropout_cases as D

pytestmark = pytest.mark.gpu

B, H, KVH = 2, 4, 2
SEED, COUNTER, STREAM = 20240607, 3, 1
SIZES = (64, 320, 577)
PS = (0.1, 0.5)
CASES = (("unit", "causal"), ("mixed", "docprefix"))


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


def _rng(cuda, seed=SEED, counter=COUNTER):
    return torch.tensor([seed, counter], dtype=torch.int64, device=cuda)


@pytest.mark.parametrize("p", PS)
def test_keep_bytes_equal_the_restatement(K, cuda, p):
    Bk, Hk, S = 2, 3, 200
    t = K.attn_dropout_threshold(p)
    assert t == D.threshold(p)
    for counter in (0, 5):
        for stream in (0, 3):
            got = K.attn_dropout_keep(Bk, Hk, S, S, (t, _rng(cuda, SEED, counter), stream))
            want = D.keep_tensor(SEED, counter, stream, Bk, Hk, S, S, t)
            assert got.dtype is torch.uint8 and got.shape == (Bk, Hk, S, S)
            assert torch.equal(got.cpu().bool(), want), (p, counter, stream)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("family,kind", CASES)
def test_attn_fwd_bwd_dropout_against_float64(K, cuda, family, kind, S, p):
    q, k, v, do = (x.to(cuda) for x in C.make_case(family, B, S, H, KVH, f"drop{kind}"))
    mask, doc, prefix = C.dense_mask(kind, B, S)
    mask = mask.to(cuda)
    ms = K.MaskSpec(doc, prefix) if (doc is not None or prefix is not None) else None
    t = K.attn_dropout_threshold(p)
    c = D.scale_c(t)
    keep = D.keep_tensor(SEED, COUNTER, STREAM, B, H, S, S, t, cuda)
    drop = (t, _rng(cuda), STREAM)
    label = f"dropout {family} {kind} S={S} p={p}"

    o, lse = K.attn_fwd(q, k, v, ms, dropout=drop)
    o0, lse0 = K.attn_fwd(q, k, v, ms)
    assert torch.equal(lse, lse0), "lse is that of the undropped rows, bit for bit"
    o_ref, lse_ref = D.fwd64(q, k, v, mask, keep, c)
    err, cos, le = C.max_rel(o, o_ref), C.worst_row_cos(o, o_ref), C.lse_rel(lse, lse_ref)
    print(f"[{label}] O {err:.2e} (bar {C.FWD_O_BAR:.0e})  cos {cos:.6f} (bar {C.FWD_O_COS})  lse {le:.1e} (bar {C.LSE_REL:.0e})")

    g = [torch.full_like(x, float("nan")) for x in (q, k, v)]
    K.attn_bwd(q, k, v, o, do, lse, *g, ms, dropout=drop)
    ref, rnd = D.bwd64(q, k, v, o, do, mask, keep, c)
    res = [(n, *C.bwd_err(a, b_, r)) for n, a, b_, r in zip(("dq", "dk", "dv"), g, ref, rnd)]
    print(f"[{label}] " + "  ".join(f"{n} {r:.3f} of bar, cos {cs:.6f}" for n, r, cs in res) + f"  (cos bar {C.BWD_COS})")

    # a query row whose every allowed key was dropped: exact zeros in O and dQ (the cosine checks leave zero rows out by themselves)
    live = mask.expand(B, H, S, S) & keep
    dead_rows = ~live.any(-1)                                # [B, H, S]
    print(f"[{label}] rows with every allowed key dropped: {int(dead_rows.sum())}")
    dr = dead_rows.transpose(1, 2)                           # [B, S, H]
    assert (o[dr] == 0).all() and (g[0][dr] == 0).all(), "a fully dropped row is an exact zero row in O and dQ"
    if p == 0.5 and kind == "causal":
        assert int(dead_rows.sum()) > 0  # (row 0 has one allowed key)
    # a key dropped for every query of its head group: exact zero dV
    dead_keys = ~live.view(B, KVH, H // KVH, S, S).any(3).any(2)   # [B, KVH, S]
    print(f"[{label}] keys dropped for every query of their group: {int(dead_keys.sum())}")
    assert (g[2][dead_keys.transpose(1, 2)] == 0).all(), "a key no query keeps has exactly zero dV"

    assert err <= C.FWD_O_BAR, f"{label}: O max-norm error {err:.3e}"
    assert cos >= C.FWD_O_COS, f"{label}: worst row cosine {cos:.6f}"
    assert le <= C.LSE_REL, f"{label}: lse error {le:.3e}"
    for n, ratio, cs in res:
        assert ratio <= 1.0, f"{label} {n}: error {ratio:.3f} x the bar"
        assert cs >= C.BWD_COS, f"{label} {n}: worst row cosine {cs:.6f}"

    # the same ticket again: bit-identical
    o2, lse2 = K.attn_fwd(q, k, v, ms, dropout=(t, _rng(cuda), STREAM))
    g2 = [torch.full_like(x, float("nan")) for x in (q, k, v)]
    K.attn_bwd(q, k, v, o2, do, lse2, *g2, ms, dropout=(t, _rng(cuda), STREAM))
    assert torch.equal(o, o2) and torch.equal(lse, lse2) and all(torch.equal(a, b_) for a, b_ in zip(g, g2))
    assert not torch.equal(o, o0)


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


def test_attention_block_against_float64_composition(K, cuda):
    """One Attention module at the tiny configuration's dimensions, train mode, p = 0.25: projections, rotary embedding, masked
    softmax with the keep bytes of attn_dropout_keep, wo - composed in float64 here.  Bars: those of the tiny layer in
    tests/test_model_gpu.py (output 0.03, dx 0.05, weight gradients 0.06)."""
    from llx import ops
    from modelling.llama import Attention
    from tests.util import to_model_config

    cfg = O.TINY._replace(attn_dropout=0.25)
    S, Bt, p = 200, 2, 0.25
    Hh, KV, hd, Dm = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, cfg.embed_dim
    att = Attention(to_model_config(cfg)).bfloat16()
    w = {n: O.randn("attdrop_" + n, tuple(getattr(att, n).weight.shape), 0.05).bfloat16() for n in ("wq", "wk", "wv", "wo")}
    with torch.no_grad():
        for n, t_ in w.items():
            getattr(att, n).weight.copy_(t_)
    att = att.to(cuda).train()
    x = O.randn("attdrop_x", (Bt, S, Dm), 1.0).bfloat16()
    dy = O.randn("attdrop_dy", (Bt, S, Dm), 0.1).bfloat16()
    rope = O.rope_table(cfg)[:S]
    seed, counter = 99, 7
    ops.seed_attn_dropout(seed, counter)
    xg = x.to(cuda).requires_grad_()
    y = att(xg, rope.to(cuda))  # a stand-alone module draws its own ticket, stream id 0
    y.backward(dy.to(cuda))

    t = K.attn_dropout_threshold(p)
    keep = K.attn_dropout_keep(Bt, Hh, S, S, (t, torch.tensor([seed, counter], dtype=torch.int64, device=cuda), 0)).cpu().bool()
    assert torch.equal(keep, D.keep_tensor(seed, counter, 0, Bt, Hh, S, S, t))
    xr = x.double().requires_grad_()
    wr = {n: t_.double().requires_grad_() for n, t_ in w.items()}
    qd = O.rope_apply((xr @ wr["wq"].T).view(Bt, S, Hh, hd), rope.double()).transpose(1, 2)
    kd = O.rope_apply((xr @ wr["wk"].T).view(Bt, S, KV, hd), rope.double()).transpose(1, 2).repeat_interleave(Hh // KV, dim=1)
    vd = (xr @ wr["wv"].T).view(Bt, S, KV, hd).transpose(1, 2).repeat_interleave(Hh // KV, dim=1)
    s = ((qd @ kd.transpose(-1, -2)) / math.sqrt(hd)).masked_fill(~torch.ones(S, S, dtype=torch.bool).tril(), float("-inf"))
    pm = torch.softmax(s, dim=-1) * keep.double() * D.scale_c(t)
    ref = (pm @ vd).transpose(1, 2).reshape(Bt, S, Hh * hd) @ wr["wo"].T
    ref.backward(dy.double())
    errs = {"y": (_rel(y.cpu(), ref.detach()), 0.03), "dx": (_rel(xg.grad.cpu(), xr.grad), 0.05)}
    for n in w:
        errs["d" + n] = (_rel(getattr(att, n).weight.grad.cpu(), wr[n].grad), 0.06)
    print("[attention block p=0.25] " + "  ".join(f"{n} {e:.4f} (bar {b_})" for n, (e, b_) in errs.items()))
    for n, (e, b_) in errs.items():
        assert e <= b_, (n, e, b_)


def _tiny(cuda, p, **cfg_kw):
    from tests.util import bf16_params, build_model

    cfg = O.TINY._replace(attn_dropout=p, **cfg_kw)
    pb, _ = bf16_params(O.init_params(cfg))
    return build_model(cfg, pb, cuda)


def _data(cuda, Bt=2, S=192):
    tokens = O.randint("drop_tokens", (Bt, S), 0, O.TINY.vocab_size)
    labels = torch.roll(tokens, -1, 1).clone()
    labels[:, : S // 4] = -100
    labels[:, -1] = -100
    return tokens.to(cuda), labels.to(cuda)


def _step(model, tokens, labels, seed=None, counter=0):
    from llx import ops

    if seed is not None:
        ops.seed_attn_dropout(seed, counter)
    for q in model.parameters():
        q.grad = None
    loss = model(tokens, labels=labels)
    loss.backward()
    return loss.detach().clone(), {n: q.grad.detach().clone() for n, q in model.named_parameters()}


def _same(a, b):
    return torch.equal(a[0], b[0]) and all(torch.equal(a[1][n], b[1][n]) for n in a[1])


def test_tiny_model_trains_with_attention_dropout(cuda):
    from llx import ops

    tokens, labels = _data(cuda)
    model = _tiny(cuda, 0.25).train()
    plain = _tiny(cuda, 0.0).train()
    first = _step(model, tokens, labels, 11, 0)
    loss0, _ = _step(plain, tokens, labels)
    assert torch.isfinite(first[0]) and first[0].item() != loss0.item()
    assert abs(first[0].item() - loss0.item()) < 0.5  # (a perturbation of the same model, not another one)
    # the same seed and counter: bit-identical loss and gradients
    again = _step(model, tokens, labels, 11, 0)
    assert _same(first, again)
    # consecutive steps differ (the counter advanced on the device)
    nxt = _step(model, tokens, labels)
    assert nxt[0].item() != first[0].item()
    assert _same(nxt, _step(model, tokens, labels, 11, 1))
    # activation checkpointing recomputes every layer with the step's ticket: bit-identical to off
    model.config = model.config._replace(activation_checkpointing=True)
    assert _same(first, _step(model, tokens, labels, 11, 0))
    model.config = model.config._replace(activation_checkpointing=False)
    # eval: the kernels without dropout, bit-identical to attn_dropout = 0
    model.eval()
    plain.eval()
    with torch.no_grad():
        assert torch.equal(model(tokens, labels=labels), plain(tokens, labels=labels))
        assert torch.equal(model(tokens), plain(tokens))
    # a dense causal mask= under autograd takes the dropout route and equals the no-mask run, bit for bit
    model.train()
    layer = model.layers[1]
    S = 192
    hid = O.randn("drop_hidden", (1, S, O.TINY.embed_dim), 0.5).bfloat16().to(cuda)
    dy = O.randn("drop_dy", (1, S, O.TINY.embed_dim), 0.1).bfloat16().to(cuda)
    outs = []
    for mask in (None, torch.ones(S, S, dtype=torch.bool, device=cuda).tril()):
        ops.seed_attn_dropout(5, 2)
        xg = hid.clone().requires_grad_()
        out = layer(xg, model.rope[:S], mask=mask)
        out.backward(dy)
        outs.append((out.detach(), xg.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    layer.eval()
    with torch.no_grad():
        assert not torch.equal(layer(hid, model.rope[:S]), outs[0][0])


def test_captured_training_step_draws_a_new_mask_per_replay(cuda, monkeypatch):
    """Forward and backward of the tiny model captured once and replayed three times: the counter advances on the device inside the
    graph, so the losses differ pairwise, and replay i equals the eager step at the same counter value bit for bit.  The captured
    step is one linear stream: nothing inside it enters or waits for a side stream."""
    from llx import ops

    tokens, labels = _data(cuda)
    model = _tiny(cuda, 0.25).train()
    seed, c0 = 17, 10
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            _step(model, tokens, labels, seed, 0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for q in model.parameters():
        q.grad = None
    ops.seed_attn_dropout(seed, c0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side_uses = []
    with torch.cuda.graph(graph):
        with monkeypatch.context() as mp:
            for name in ("wait_stream", "wait_event"):
                orig = getattr(torch.cuda.Stream, name)
                mp.setattr(torch.cuda.Stream, name, lambda self, *a, _o=orig, _n=name: (side_uses.append(_n), _o(self, *a))[1])
            orig_ctx = torch.cuda.stream
            mp.setattr(torch.cuda, "stream", lambda s: (side_uses.append("stream"), orig_ctx(s))[1])
            static_loss = model(tokens, labels=labels)
            static_loss.backward()
    assert side_uses == [], f"the captured step left its stream: {side_uses}"
    replays = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        replays.append((static_loss.detach().clone(), {n: q.grad.detach().clone() for n, q in model.named_parameters()}))
    losses = [r[0].item() for r in replays]
    assert len(set(losses)) == 3, losses
    del graph
    for i, rep in enumerate(replays):
        eager = _step(model, tokens, labels, seed, c0 + i)
        assert _same(rep, eager), f"replay {i} against the eager step at counter {c0 + i}"


def test_rejections_name_the_field(cuda):
    from llx._lib import LlxError
    from modelling.llama import MaskSpec, TransformerLayer
    from tests.util import to_model_config

    S = 64
    x = O.randn("drop_rej_x", (1, S, O.TINY.embed_dim), 0.5).bfloat16().to(cuda)
    rope = O.rope_table(O.TINY)[:S].to(cuda)

    def layer_with(p):
        return TransformerLayer(to_model_config(O.TINY._replace(attn_dropout=p))).bfloat16().to(cuda).train()

    for p in (1.0, -0.1):
        with pytest.raises(LlxError, match="attn_dropout"):
            layer_with(p)(x.clone().requires_grad_(), rope)
        with pytest.raises(LlxError, match="attn_dropout"):
            _tiny(cuda, p).train()(torch.zeros(1, S, dtype=torch.int64, device=cuda))
    layer = layer_with(0.25)
    tril = torch.ones(S, S, dtype=torch.bool, device=cuda).tril()
    with pytest.raises(LlxError, match="attn_dropout"):
        layer(x.clone().requires_grad_(), rope, block_mask=MaskSpec(prefix_len=torch.tensor([8])))
    with pytest.raises(LlxError, match="attn_dropout"):
        layer(x.clone().requires_grad_(), rope, block_mask=MaskSpec(dense=tril))
    g = torch.Generator().manual_seed(3)
    scattered = (torch.rand(S, S, generator=g) < 0.5) | torch.eye(S, dtype=torch.bool)
    with pytest.raises(LlxError, match="attn_dropout"):
        layer(x.clone().requires_grad_(), rope, mask=scattered.to(cuda))
    # the same calls are served in eval mode (no dropout there)
    layer.eval()
    with torch.no_grad():
        layer(x, rope, block_mask=MaskSpec(prefix_len=torch.tensor([8])))
