"""GPU: the attention kernels at the softmax dynamic range of trained models (tests/attn_cases.py families: diagonal heads, score
ramps, attention sinks, near one-hot rows, and all of them inside one wave) against float64 references computed on the device.

Forward (attn_fwd, causal and mask-metadata kernels): O by max-norm and per-row cosine, and the lse it hands to the backward,
checked directly.  Backward (both routes): dq, dk, dv against `bwd64`.  Decode (split cache) with a sink and the maximum at the
last valid key.  Dense-mask inference kernel at its broadcast mask shapes.  One 8B-dimension layer with diagonal-dominant heads.
Every bar is a constant of tests/attn_cases.py, the same for every family; each case prints its measured error next to it."""
import math

import pytest
import torch

from oracle import ref as O
from tests import attn_cases as C

pytestmark = pytest.mark.gpu

MASKS = ("causal", "doc", "prefix", "docprefix")
SHAPES = [(2, 449, 4, 4), (2, 705, 8, 2), (2, 1024 + 37, 4, 1)]  # (B, S, H, KVH): GQA 1:1 and 4:1, S off the 64 / 128 / 256 tiles


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


def _case(K, cuda, family, kind, i, tag):
    B, S, H, KVH = SHAPES[i % len(SHAPES)]
    q, k, v, do = (t.to(cuda) for t in C.make_case(family, B, S, H, KVH, tag))
    mask, doc, prefix = C.dense_mask(kind, B, S)
    ms = K.MaskSpec(doc, prefix) if (doc is not None or prefix is not None) else None
    return (B, S, H, KVH), q, k, v, do, mask.to(cuda), ms


def _check_fwd(label, o, lse, o_ref, lse_ref):
    err, cos, le = C.max_rel(o, o_ref), C.worst_row_cos(o, o_ref), C.lse_rel(lse, lse_ref)
    print(f"[{label}] O {err:.2e} (bar {C.FWD_O_BAR:.0e})  cos {cos:.6f} (bar {C.FWD_O_COS})  lse {le:.1e} (bar {C.LSE_REL:.0e})")
    assert err <= C.FWD_O_BAR, f"{label}: O max-norm error {err:.3e}"
    assert cos >= C.FWD_O_COS, f"{label}: worst row cosine {cos:.6f}"
    assert le <= C.LSE_REL, f"{label}: lse error {le:.3e}"


def _check_bwd(label, grads, ref, rnd):
    out = []
    for name, a, b, r in zip(("dq", "dk", "dv"), grads, ref, rnd):
        ratio, cos = C.bwd_err(a, b, r)
        out.append((name, ratio, cos))
    print(f"[{label}] " + "  ".join(f"{n} {r:.3f} of bar, cos {c:.6f}" for n, r, c in out) + f"  (cos bar {C.BWD_COS})")
    for name, ratio, cos in out:
        assert ratio <= 1.0, f"{label} {name}: error {ratio:.3f} x the bar"
        assert cos >= C.BWD_COS, f"{label} {name}: worst row cosine {cos:.6f}"


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("family", C.FAMILIES)
def test_attn_fwd_dynamic_range(K, cuda, family, kind):
    i = C.FAMILIES.index(family) + MASKS.index(kind)
    shp, q, k, v, _, mask, ms = _case(K, cuda, family, kind, i, "fwd")
    o_ref, lse_ref = C.sdpa64(q, k, v, mask)
    o, lse = K.attn_fwd(q, k, v, ms)
    _check_fwd(f"attn_fwd {family} {kind} B,S,H,KVH={shp}", o, lse, o_ref, lse_ref)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("family", C.FAMILIES)
def test_attn_bwd_dynamic_range_both_routes(K, cuda, family, kind):
    """Both routes of llx_attn_bwd (with / without the dS^T scratch) against bwd64, given the forward kernel's own O and lse; each
    route is deterministic (bit-identical reruns) and the two agree within the same bar."""
    i = C.FAMILIES.index(family) + MASKS.index(kind) + 1
    shp, q, k, v, do, mask, ms = _case(K, cuda, family, kind, i, "bwd")
    o, lse = K.attn_fwd(q, k, v, ms)
    ref, rnd = C.bwd64(q, k, v, o, do, mask)
    out = {}
    for route in (True, False):
        old = K._ATTN_BWD_DS
        K._ATTN_BWD_DS = route
        try:
            runs = []
            for _ in range(2):
                g = [torch.full_like(t, float("nan")) for t in (q, k, v)]
                K.attn_bwd(q, k, v, o, do, lse, *g, ms)
                runs.append(g)
        finally:
            K._ATTN_BWD_DS = old
        assert all(torch.equal(a, b) for a, b in zip(*runs)), f"route ds={route}: bit-identical reruns"
        out[route] = runs[0]
        _check_bwd(f"attn_bwd ds={int(route)} {family} {kind} B,S,H,KVH={shp}", runs[0], ref, rnd)
    for name, a, b, r in zip(("dq", "dk", "dv"), out[True], out[False], rnd):
        ratio, _ = C.bwd_err(a, b, r)
        assert ratio <= 1.0, f"routes disagree on {name}: {ratio:.3f} x the bar"


@pytest.mark.parametrize("family", ["ramp", "diag"])
def test_attn_long_sequence_base_moves_across_flag_reloads(K, cuda, family):
    """S = 4160: the mask-metadata kernels reload their 64-tile flag word while the base keeps moving.  A MaskSpec encoding the
    plain causal mask gives what the causal kernels give, bit for bit, and both meet float64."""
    B, S, H, KVH = 1, 4160, 2, 1
    q, k, v, do = (t.to(cuda) for t in C.make_case(family, B, S, H, KVH, "long"))
    mask = torch.ones(S, S, dtype=torch.bool, device=cuda).tril()[None, None]
    o0, lse0 = K.attn_fwd(q, k, v)
    g0 = [torch.empty_like(t) for t in (q, k, v)]
    K.attn_bwd(q, k, v, o0, do, lse0, *g0)
    o_ref, lse_ref = C.sdpa64(q, k, v, mask)
    _check_fwd(f"attn_fwd {family} causal S={S}", o0, lse0, o_ref, lse_ref)
    del o_ref, lse_ref
    ref, rnd = C.bwd64(q, k, v, o0, do, mask)
    _check_bwd(f"attn_bwd {family} causal S={S}", g0, ref, rnd)
    del ref, rnd
    for ms in (K.MaskSpec(doc_ids=torch.zeros(B, S, device=cuda, dtype=torch.int32)),
               K.MaskSpec(prefix_len=torch.zeros(B, device=cuda, dtype=torch.int32))):
        o1, lse1 = K.attn_fwd(q, k, v, ms)
        assert torch.equal(o0, o1) and torch.equal(lse0, lse1)
        g1 = [torch.empty_like(t) for t in (q, k, v)]
        K.attn_bwd(q, k, v, o0, do, lse0, *g1, ms)
        assert all(torch.equal(a, b) for a, b in zip(g0, g1))


def _sdpa64_bhsd(q, k, v, mask):
    """float64 SDPA in the [B, H, M, 128] / [B, KVH, Skv, 128] layout of the inference kernels (GQA by head grouping)."""
    g = q.shape[1] // k.shape[1]
    s = (q.double() @ k.double().repeat_interleave(g, dim=1).transpose(-1, -2)) * C.SCALE
    return torch.softmax(s.masked_fill(~mask, float("-inf")), dim=-1) @ v.double().repeat_interleave(g, dim=1)


@pytest.mark.parametrize("M", [1, 2, 3, 4])
@pytest.mark.parametrize("Skv", [4096, 8192 + 5])
def test_attn_decode_sink_and_late_maximum(K, cuda, Skv, M):
    """Split-cache decode, GQA 32:8: key 0 is a 26-nat sink and every query row's maximum is its last valid key (top nats above
    the row's typical score), so the splits' maxima differ by tens of nats - at top = 120 every combine factor but the last
    split's underflows.  Then a per-row mask with holes over the same cache."""
    H, KVH, hd = 32, 8, 128
    G = H // KVH
    u = C._unit(O.randn(f"dk_u{Skv}", (KVH, hd)))
    uq = u.repeat_interleave(G, dim=0)[None, :, None]                                      # [1, H, 1, hd]
    q = O.randn(f"dk_q{Skv}{M}", (1, H, M, hd))
    q = q - (q * uq).sum(-1, keepdim=True) * uq + 4.0 * uq                               # q.u = 4 for every row
    kc = O.randn(f"dk_k{Skv}", (1, KVH, Skv, hd))
    vc = O.randn(f"dk_v{Skv}", (1, KVH, Skv, hd))
    pos = torch.arange(Skv - M, Skv)
    mask = torch.ones(Skv, Skv, dtype=torch.bool).tril()[None, None, pos]                # [1, 1, M, Skv]: row m sees keys <= pos[m]
    qd, vd, md = q.bfloat16().to(cuda), vc.bfloat16().to(cuda), mask.to(cuda)
    for top in (40.0, 120.0):
        k = kc.clone()
        k[0, :, 0] = (26.0 / (4.0 * C.SCALE)) * u
        for m in range(M):  # row m's own key: (top + m) nats, above every earlier row's maximum
            k[0, :, Skv - M + m] = ((top + m) / (4.0 * C.SCALE)) * u
        kd = k.bfloat16().to(cuda)
        want = _sdpa64_bhsd(qd, kd, vd, md)
        got = K.attn_decode(qd, kd, vd, md, K.mask_extent(md)).view(1, M, H, hd).transpose(1, 2)
        err, cos = C.max_rel(got, want), C.worst_row_cos(got, want)
        print(f"[attn_decode Skv={Skv} M={M} top={top:.0f}] O {err:.2e} (bar {C.FWD_O_BAR:.0e}) cos {cos:.6f} (bar {C.FWD_O_COS})")
        assert err <= C.FWD_O_BAR and cos >= C.FWD_O_COS, (top, err, cos)
    # a per-(head, row) mask with holes: ~30 % of the keys, the sink kept for even heads, the row's own key for odd ones
    g = torch.Generator().manual_seed(Skv + M)
    m2 = torch.rand(1, H, M, Skv, generator=g) < 0.3
    m2 &= mask
    m2[:, 0::2, :, 0] = True
    m2[:, 1::2, torch.arange(M), pos] = True
    m2[:, 1::2, :, 0] = False
    m2d = m2.to(cuda)
    want = _sdpa64_bhsd(qd, kd, vd, m2d)
    got = K.attn_decode(qd, kd, vd, m2d, K.mask_extent(m2d)).view(1, M, H, hd).transpose(1, 2)
    err, cos = C.max_rel(got, want), C.worst_row_cos(got, want)
    print(f"[attn_decode Skv={Skv} M={M} holes] O {err:.2e} (bar {C.FWD_O_BAR:.0e}) cos {cos:.6f} (bar {C.FWD_O_COS})")
    assert err <= C.FWD_O_BAR and cos >= C.FWD_O_COS, (err, cos)


@pytest.mark.parametrize("mshape", ["SqSkv", "B1SqSkv", "BHSqSkv"])
@pytest.mark.parametrize("family", ["unit", "diag", "sink"])
def test_attn_dense_fwd_dynamic_range(K, cuda, family, mshape):
    """llx_attn_dense_fwd (explicit bool mask / KV-cache prefill, modelling/llama.py:_run_dense) at its broadcast mask shapes, q as
    the strided view of a fused q|k|v row buffer and k / v as views of a K|V buffer (the layouts _run_dense passes), Skv off the
    64-key chunk, Sq from 1 to 300 (the last Sq positions of the sequence, as a prefill continuing a cache).  A fully masked row
    comes out NaN, as SDPA, and leaves its neighbours finite."""
    B, H, KVH, hd = 2, 8, 2, 128
    Skv = 333 + 100 * (C.FAMILIES.index(family) % 3)
    for Sq in (1, 37, 300):
        q_all, k_all, v_all, _ = C.make_case(family, B, Skv, H, KVH, f"dense{mshape}")
        qbuf = torch.zeros(B, Sq, (H + 2 * KVH) * hd, dtype=torch.bfloat16)
        qbuf[..., : H * hd] = q_all[:, Skv - Sq :].reshape(B, Sq, H * hd)
        kvbuf = torch.cat([k_all.reshape(B, Skv, KVH * hd), v_all.reshape(B, Skv, KVH * hd)], dim=-1).to(cuda)
        qbuf = qbuf.to(cuda)
        q = qbuf[..., : H * hd].unflatten(-1, (H, hd)).transpose(1, 2)                    # [B, H, Sq, hd], strided
        k = kvbuf[..., : KVH * hd].unflatten(-1, (KVH, hd)).transpose(1, 2)               # [B, KVH, Skv, hd], strided
        v = kvbuf[..., KVH * hd :].unflatten(-1, (KVH, hd)).transpose(1, 2)
        pos = torch.arange(Skv - Sq, Skv)
        causal = torch.ones(Skv, Skv, dtype=torch.bool).tril()[pos]                       # [Sq, Skv]
        dead = None
        if mshape == "SqSkv":
            mask = causal
        elif mshape == "B1SqSkv":  # batch 1: a left-padded sample (its first 20 keys are padding; every row starts at key >= 33)
            mask = causal[None, None].repeat(B, 1, 1, 1)
            mask[1, :, :, :20] = False
        else:  # per-head holes; the row's own key always kept; one row of one head fully masked
            g = torch.Generator().manual_seed(Sq)
            mask = causal[None, None] & (torch.rand(B, H, Sq, Skv, generator=g) < 0.5)
            mask[:, :, torch.arange(Sq), pos] = True
            dead = (1, 3, Sq // 2)
            mask[dead] = False
        md = mask.to(cuda)
        got = K.attn_dense_fwd(q, k, v, md)
        want = _sdpa64_bhsd(q, k, v, md.expand(B, H, Sq, Skv))
        live = torch.ones(B, H, Sq, dtype=torch.bool, device=cuda)
        if dead is not None:
            assert torch.isnan(got[dead]).all(), "a fully masked row is NaN (SDPA's softmax over -inf)"
            live[dead] = False
        assert not torch.isnan(got[live]).any()
        err, cos = C.max_rel(got[live], want[live]), C.worst_row_cos(got[live], want[live])
        print(f"[attn_dense_fwd {family} mask {mshape} Sq={Sq} Skv={Skv}] O {err:.2e} (bar {C.FWD_O_BAR:.0e}) cos {cos:.6f} (bar {C.FWD_O_COS})")
        assert err <= C.FWD_O_BAR and cos >= C.FWD_O_COS, (Sq, err, cos)


@pytest.mark.parametrize("kind", ["causal", "prefix"])
def test_layer_with_diagonal_dominant_heads_at_8b_dimensions(cuda, kind):
    """One TransformerLayer at Llama-3.1-8B dimensions, S = 4096, LoRA r = 16, with wk of every KV head tied to a scaled copy of wq
    of the first query head of its group: RoPE at equal positions cancels, so that head's diagonal score is c |q_i|^2 / sqrt(128),
    ~20 nats above the row's typical score (the other three heads of the group stay random).  Drives the q|k|v GEMM's RoPE
    epilogue, the forward's rescale path and both backward kernels at production tile shapes.  Oracle: O.layer in fp32 on the
    device; bars and row cosines of test_model_gpu.py::test_full_dimension_layer_parity (bf16).

    One exception, of rounding alone: the rows of wq.lora_b's gradient that belong to the tied heads are held to the max-norm bar
    but not to the row cosine.  A tied head is one-hot to ~1e-5, so its exact dq is ~1e-5 of |dO| |V| |k|, while the backward's
    documented delta = rowsum(dO . O) from the bf16 O leaves ~2^-9 |dO| |O| in every dS of the row: those gradient rows are
    rounding noise in any bf16-O flash backward (measured on the MI355X: worst row cosine 0.006 causal / -0.097 prefix, max-norm
    error 0.011 / 0.010 against the 0.05 bar).  The kernel-level diag cases check the same dq against the reference that takes
    delta from the bf16 O (test_attn_bwd_dynamic_range_both_routes)."""
    from modelling import apply_linear_adapter_
    from modelling.llama import LlamaConfig, MaskSpec, TransformerLayer, build_rope
    from tests.util import _close, _rows_close, bf16_params

    S = 4096
    cfg = O.LLAMA31_8B._replace(num_layers=1, max_seq_len=S)
    p = {k: v for k, v in O.init_params(cfg._replace(vocab_size=8)).items() if k.startswith("layers.0.")}
    wq, wk = p["layers.0.attention.wq.weight"], p["layers.0.attention.wk.weight"]
    G = cfg.num_heads // cfg.num_kv_heads
    for j in range(cfg.num_kv_heads):
        w0 = wq[j * G * 128 : (j * G + 1) * 128]
        c = 20.0 * math.sqrt(128) / float(w0.pow(2).sum())  # E|q|^2 = ||w0||_F^2 for unit-rms normalised rows
        wk[j * 128 : (j + 1) * 128] = c * w0
    p.update(O.init_lora(cfg, 16))
    pb, pf = bf16_params(p)
    x = O.randn("x_diag", (1, S, cfg.embed_dim), 0.5).bfloat16()
    dy = O.randn("dy_diag", (1, S, cfg.embed_dim), 0.1).bfloat16()
    if kind == "causal":
        dense, spec = torch.ones(S, S, dtype=torch.bool).tril(), None
    else:
        P = S // 2 - 56
        dense, spec = O.prefix_lm_mask(S, [P])[0, 0], MaskSpec(prefix_len=torch.tensor([P]))
    train = [k for k in pf if "lora_" in k or k.endswith("_norm.weight")]
    pr = {k: (v.to(cuda).clone().requires_grad_() if k in train else v.to(cuda)) for k, v in pf.items()}
    xr = x.float().to(cuda).requires_grad_()
    ref = O.layer(xr, pr, 0, cfg, O.rope_table(cfg)[:S].to(cuda), dense.to(cuda), 1.0)
    ref.backward(dy.float().to(cuda))
    ref = ref.detach()

    layer = TransformerLayer(LlamaConfig(**{f: getattr(cfg, f) for f in LlamaConfig._fields})).bfloat16()
    layer.load_state_dict({k[len("layers.0."):]: v for k, v in pb.items() if "lora_" not in k})
    apply_linear_adapter_(layer, "lora", rank=16, alpha=16.0)
    with torch.no_grad():
        for name, mod in layer.named_modules():
            if f"layers.0.{name}.lora_a" in pb:
                mod.lora_a.copy_(pb[f"layers.0.{name}.lora_a"])
                mod.lora_b.copy_(pb[f"layers.0.{name}.lora_b"])
    layer = layer.to(cuda)
    for n, q in layer.named_parameters():
        q.requires_grad_("lora_" in n or n.endswith("_norm.weight"))
    rope = build_rope(LlamaConfig(**{f: getattr(cfg, f) for f in LlamaConfig._fields})).to(cuda)
    xg = x.to(cuda).requires_grad_()
    out = layer(xg, rope[:S], block_mask=spec)
    out.backward(dy.to(cuda))
    o_f, dx_f = out.float(), xg.grad.float()
    print(f"[layer 8B diag heads S={S} {kind}] out err {C.max_rel(o_f, ref):.4f} (bar 0.02) cos {C.worst_row_cos(o_f, ref):.6f} (bar 0.999), "
          f"dx err {C.max_rel(dx_f, xr.grad):.4f} (bar 0.04) cos {C.worst_row_cos(dx_f, xr.grad):.6f} (bar 0.998)")
    _close(o_f, ref, 0.02, "layer output, diagonal heads")
    _rows_close(o_f, ref, "layer output rows, diagonal heads", min_cos=0.999)
    _close(dx_f, xr.grad, 0.04, "dx, diagonal heads")
    _rows_close(dx_f, xr.grad, "dx rows, diagonal heads", min_cos=0.998)
    tied = torch.zeros(cfg.num_heads, dtype=torch.bool)
    tied[::G] = True
    checks = []
    for name, q in layer.named_parameters():
        if q.requires_grad:
            g, want = q.grad.float(), pr["layers.0." + name].grad
            if name == "attention.wq.lora_b":  # rows of the random heads only for the cosine (docstring)
                rows = ~tied.repeat_interleave(128).to(cuda)
                gc, wc = g[rows], want[rows]
            else:
                gc, wc = g, want
            print(f"  {name}: err {C.max_rel(g, want):.4f} (bar 0.05)" + (f" cos {C.worst_row_cos(gc, wc):.6f} (bar 0.995)" if g.dim() == 2 else ""))
            checks.append((name, g, want, gc, wc))
    for name, g, want, gc, wc in checks:
        _close(g, want, 0.05, name)
        if g.dim() == 2:
            _rows_close(gc, wc, name, min_cos=0.995)
