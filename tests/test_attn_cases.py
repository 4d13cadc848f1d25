"""CPU checks of the attention input families (tests/attn_cases.py) and of the bars the GPU tests hold the kernels to.

Precondition: the families other than `unit` / `sink` move the forward's deferred softmax base after state has accumulated, at
every tile width the kernel could use.  Discriminating power: a restatement of the forward's documented arithmetic lands inside
the GPU bars on every family, and its two mutants (no `l_run *= alpha`, no O rescale) land at least 10x outside them wherever
the path is reached.  The backward's restatement meets the backward bars on every family with the same numbers."""
import pytest
import torch

from oracle import ref as O
from tests import attn_cases as C

# (B, S, H, KVH, mask kind): a causal GQA 4:1 wave sweep and a document + prefix mask with S off the tile grid
SHAPES = [(1, 384, 4, 1, "causal"), (1, 449, 4, 2, "docprefix")]


@pytest.mark.parametrize("family", ["diag", "ramp", "hot", "mixed"])
@pytest.mark.parametrize("B,S,H,KVH,kind", SHAPES)
def test_families_move_the_base_on_later_tiles(family, B, S, H, KVH, kind):
    q, k, _, _ = C.make_case(family, B, S, H, KVH, "pre")
    mask, _, _ = C.dense_mask(kind, B, S)
    for tile in (32, 64, 128):
        assert C.late_base_moves(q, k, mask, tile) > 0, (family, kind, tile)


@pytest.mark.parametrize("B,S,H,KVH", [(1, 256, 4, 1), (2, 384, 4, 1), (1, 200, 8, 2)])
def test_unit_scale_causal_cases_never_move_the_base_late(B, S, H, KVH):
    """The draws of test_kernels_gpu.py::test_attention_fwd_bwd's causal cases: the base moves only on the first tile (from -inf),
    so a rescale bug is invisible to them.  (Their document / prefix cases do reach the path: a row whose document starts inside a
    wave moves the whole wave's base from -inf while its neighbours hold state.)"""
    q = O.randn("q", (B, S, H, 128)).bfloat16()
    k = O.randn("k", (B, S, KVH, 128)).bfloat16()
    mask, _, _ = C.dense_mask("causal", B, S)
    assert C.late_base_moves(q, k, mask, 64) == 0
    qs, ks, _, _ = C.make_case("sink", B, S, H, KVH, "pre")  # a sink fixes the base on tile 0 for good
    assert C.late_base_moves(qs, ks, mask, 64) == 0


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("B,S,H,KVH,kind", SHAPES)
def test_forward_emulation_inside_the_bars_and_mutants_outside(family, B, S, H, KVH, kind):
    q, k, v, _ = C.make_case(family, B, S, H, KVH, "emu")
    mask, _, _ = C.dense_mask(kind, B, S)
    o_ref, lse_ref = C.sdpa64(q, k, v, mask)
    o, lse = C.emulate_fwd(q, k, v, mask)
    err, cos, le = C.max_rel(o, o_ref), C.worst_row_cos(o, o_ref), C.lse_rel(lse, lse_ref)
    print(f"[emulated fwd {family} {kind}] O {err:.2e} (bar {C.FWD_O_BAR:.0e}) cos {cos:.6f} (bar {C.FWD_O_COS}) lse {le:.1e} (bar {C.LSE_REL:.0e})")
    assert err <= C.FWD_O_BAR and cos >= C.FWD_O_COS and le <= C.LSE_REL, (err, cos, le)
    if C.late_base_moves(q, k, mask, 64) == 0:
        return  # nothing to rescale: the mutants compute the same thing (unit / sink under a causal mask)
    for mutant in ("drop_l_rescale", "drop_o_rescale"):
        om, lm = C.emulate_fwd(q, k, v, mask, **{mutant: True})
        em = C.max_rel(om, o_ref)
        print(f"  mutant {mutant}: O {em:.2e} ({em / C.FWD_O_BAR:.0f}x the bar), lse {C.lse_rel(lm, lse_ref):.1e}")
        assert em >= 10 * C.FWD_O_BAR, (mutant, em)


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("B,S,H,KVH,kind", SHAPES + [(2, 320, 4, 4, "prefix")])
def test_backward_emulation_inside_the_bars(family, B, S, H, KVH, kind):
    q, k, v, do = C.make_case(family, B, S, H, KVH, "emu")
    mask, _, _ = C.dense_mask(kind, B, S)
    o, lse = C.emulate_fwd(q, k, v, mask)
    ref, rnd = C.bwd64(q, k, v, o, do, mask)
    got = C.emulate_bwd(q, k, v, o, do, lse, mask)
    for name, a, b, r in zip(("dq", "dk", "dv"), got, ref, rnd):
        ratio, cos = C.bwd_err(a, b, r)
        print(f"[emulated bwd {family} {kind}] {name} {ratio:.3f} of the bar, cos {cos:.6f} (bar {C.BWD_COS})")
        assert ratio <= 1.0 and cos >= C.BWD_COS, (name, ratio, cos)


@pytest.mark.parametrize("family", ["unit", "sink", "mixed"])
def test_backward_reference_is_the_autograd_gradient(family):
    """bwd64 given the exact O is float64 autograd of sdpa64 (the GPU tests feed it the kernel's bf16 O instead)."""
    B, S, H, KVH = 1, 200, 4, 2
    q, k, v, do = C.make_case(family, B, S, H, KVH, "ag")
    mask, _, _ = C.dense_mask("prefix", B, S)
    qr, kr, vr = (t.double().requires_grad_() for t in (q, k, v))
    o, _ = C.sdpa64(qr, kr, vr, mask)
    o.backward(do.double())
    (dq, dk, dv), rnd = C.bwd64(q, k, v, o.detach(), do, mask)
    for a, b, r in zip((dq, dk, dv), (qr.grad, kr.grad, vr.grad), rnd):  # (a sink head's gradient is ~1e-17: float64 cancellation)
        torch.testing.assert_close(a, b, rtol=1e-9, atol=1e-10 * r.abs().max().item())
