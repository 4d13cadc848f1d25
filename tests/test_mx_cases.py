"""CPU checks of the MXFP4 cases (tests/mx_cases.py): the oracle reproduces the hand-computed vectors, the host quantiser of
subclasses/mxfp4.py equals the oracle bit for bit, the tensor subclass behaves as the int8 one does, the restated dispatch puts every
class in the table, every GEMV case is exact and every planted fault is caught by at least one of the cases aimed at it."""
import io

import pytest
import torch
from torch import nn

from oracle import ref as O
from tests import mx_cases as C

BF16 = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------------------ the format
@pytest.mark.parametrize("name", [h[0] for h in C.HAND])
def test_hand_vectors(name):
    """The oracle and the host quantiser on the hand-computed blocks: codes, nibble order, scale byte."""
    from subclasses.mxfp4 import quantize_mxfp4

    _, x, codes, b = next(h for h in C.HAND if h[0] == name)
    want_packed = C._pack(codes.view(1, 32))
    for what, (packed, scale) in (("oracle", C.quantize(x)), ("host", quantize_mxfp4(x))):
        assert packed.dtype is torch.uint8 and scale.dtype is torch.uint8 and packed.shape == (1, 16) and scale.shape == (1, 1)
        assert int(scale) == b, f"{what} {name}: scale byte {int(scale)} != {b}"
        assert torch.equal(packed, want_packed), f"{what} {name}: codes {packed.tolist()} != {want_packed.tolist()}"
    if name == "nibbles":
        assert int(want_packed[0, 0]) == 0x71 and int(want_packed[0, 1]) == 0x3A


def test_grid_and_dequantise():
    """Every (code, scale byte the quantiser emits) dequantises to magnitude x 2^(b - 127), a normal bf16; product == oracle."""
    from subclasses.mxfp4 import dequantize_mxfp4

    codes = torch.arange(16, dtype=torch.uint8).repeat(2).view(1, 32)
    for b in (2, 3, 126, 127, 128, 251, 252):
        packed, scale = C._pack(codes), torch.tensor([[b]], dtype=torch.uint8)
        want = C.dequantize(packed, scale)
        mags = torch.tensor(C.GRID.tolist() + (-C.GRID).tolist(), dtype=torch.float64).repeat(2) * 2.0 ** (b - 127)
        assert torch.equal(want.double().view(-1), mags)
        nz = want.float().abs()[want.float() != 0]
        assert (nz >= 2.0 ** -126).all(), "a denormal"
        got = dequantize_mxfp4(packed, scale)
        assert got.dtype is BF16 and torch.equal(got.view(torch.int16), want.view(torch.int16)), b  # bit for bit: the sign of -0 too


@pytest.mark.parametrize("dtype", [BF16, torch.float32])
def test_host_quantiser_equals_oracle_and_round_trips(dtype):
    """Random matrices over many binades (and exact zeros, a zero block, tiny and huge blocks): host from_float == oracle bit for bit;
    quantise(dequantise(q)) == q."""
    from subclasses.mxfp4 import MXFP4LinearWeight

    x = O.randn(f"mxq_{dtype}", (24, 256), 1.0) * torch.exp2(O.randint(f"mxq_e_{dtype}", (24, 8), -20, 21).float()).repeat_interleave(32, 1)
    x[3, 32:64] = 0
    x[5, ::7] = 0
    x[7] *= 2.0 ** 100
    x[9] *= 2.0 ** -110
    x = x.to(dtype)
    w = MXFP4LinearWeight.from_float(x)
    packed, scale = C.quantize(x)
    assert torch.equal(w.packed, packed) and torch.equal(w.scale, scale)
    assert int(scale[3, 1]) == 127 and int(scale.min()) >= 2 and int(scale.max()) <= 252
    img = C.dequantize(packed, scale)
    assert torch.equal(w.dequantize().view(torch.int16), img.view(torch.int16))
    p2, s2 = C.quantize(img)
    # a block whose largest code fell short of 4 re-quantises under a smaller exponent: the VALUES are the fixed point, and codes and
    # scales are too wherever the block's largest magnitude is 4 or 6
    assert torch.equal(C.dequantize(p2, s2).view(torch.int16), img.view(torch.int16))
    top = (torch.stack([packed & 7, (packed >> 4) & 7], -1).view(24, 8, 32).amax(-1) >= 6)
    assert top.float().mean() > 0.9
    assert torch.equal(s2[top], scale[top]) and torch.equal(p2.view(24, 8, 16)[top], packed.view(24, 8, 16)[top])


# ------------------------------------------------------------------------------------------------------------------------ the subclass
def _lin(n=8, k=64, tag="mxl"):
    m = nn.Linear(k, n, bias=False, dtype=BF16)
    with torch.no_grad():
        m.weight.copy_(O.randn(tag, (n, k), 0.05))
    return m


def test_subclass_surface():
    from llx._lib import LlxError
    from subclasses import MXFP4LinearWeight, _QUANTIZERS, quantize_linear_

    assert _QUANTIZERS["mxfp4"] == MXFP4LinearWeight.from_float
    m = _lin()
    w0 = m.weight.detach().clone()
    quantize_linear_(m, "mxfp4")
    w = m.weight
    assert isinstance(w, nn.Parameter) and isinstance(w, MXFP4LinearWeight) and not w.requires_grad
    assert tuple(w.shape) == (8, 64) and w.dtype is BF16 and w.packed.shape == (8, 32) and w.scale.shape == (8, 2)
    packed, scale = C.quantize(w0)
    assert torch.equal(w.packed, packed) and torch.equal(w.scale, scale)
    assert torch.equal(w.dequantize(), C.dequantize(packed, scale))
    # state-dict round trip through torch.save
    buf = io.BytesIO()
    torch.save(m.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, weights_only=False)
    m2 = _lin(tag="mxl_other")
    quantize_linear_(m2, "mxfp4")
    assert not torch.equal(m2.weight.packed, packed)
    m2.load_state_dict(sd)
    assert torch.equal(m2.weight.packed, packed) and torch.equal(m2.weight.scale, scale)
    # detach / clone keep the class and the bytes
    for t in (w.detach(), w.clone()):
        assert isinstance(t, MXFP4LinearWeight) and torch.equal(t.packed, packed) and torch.equal(t.scale, scale)
    assert w.clone().packed.data_ptr() != w.packed.data_ptr()
    # the three copy_ cases: MXFP4 -> MXFP4, float -> MXFP4 (re-quantise), MXFP4 -> float (dequantise)
    other = O.randn("mxl_src", (8, 64), 0.3).to(BF16)
    dst = MXFP4LinearWeight.from_float(torch.ones(8, 64, dtype=BF16))
    dst.copy_(w.detach())
    assert torch.equal(dst.packed, packed) and torch.equal(dst.scale, scale)
    dst.copy_(other)
    po, so = C.quantize(other)
    assert torch.equal(dst.packed, po) and torch.equal(dst.scale, so)
    flat = torch.empty(8, 64, dtype=BF16)
    flat.copy_(dst)
    assert torch.equal(flat, C.dequantize(po, so))
    # refusals
    with pytest.raises(LlxError, match="multiple of 32"):
        MXFP4LinearWeight.from_float(torch.ones(4, 48, dtype=BF16))
    for bad in (float("inf"), float("-inf"), float("nan")):
        x = torch.ones(4, 64)
        x[2, 40] = bad
        with pytest.raises(LlxError, match="non-finite"):
            MXFP4LinearWeight.from_float(x)
    with pytest.raises(KeyError):
        quantize_linear_(_lin(), "mxfp8")


def test_plans_and_decode_kinds():
    """DoRA on the format is refused as on int8; the decode path knows the kind before its bf16 fall-through; no batched stream."""
    import llx.decode as D
    from llx import ops
    from llx._lib import LlxError
    from modelling import apply_linear_adapter_
    from subclasses import quantize_linear_

    m = _lin(16, 64)
    quantize_linear_(m, "mxfp4")
    assert D._plain(m) == D.KIND_MX4 and D.KIND_MX4 not in (D.KIND_BF16, D.KIND_I8W, D.KIND_I8D)
    assert not D._batch_group((m,))
    plan = ops.LinearPlan(m)
    assert plan.mx4 and not plan.int8 and plan.tensors() == []
    w = D._w((m,))
    assert w["ws"][0] is m.weight.packed and w["mxscale"][0] is m.weight.scale and set(w) == {"ws", "mxscale"}
    apply_linear_adapter_(m, "lora", rank=8, alpha=16.0)
    assert m.lora_a.dtype is BF16 and D._plain(m) == D.KIND_MX4 and not D._batch_group((m,))
    assert [t is p for t, p in zip(ops.LinearPlan(m).tensors(), (m.lora_a, m.lora_b))] == [True, True]
    bf = _lin(16, 64)
    assert not ops.GroupPlan((m, bf)).fused  # a fused group is one kind
    m.m = nn.Parameter(torch.ones(m.out_features, dtype=BF16))  # (DoRALinear cannot take the row norms of the packed weight itself)
    with pytest.raises(LlxError, match="DoRA on an MXFP4LinearWeight"):
        ops.LinearPlan(m)
    assert D._plain(m) is None
    m2 = _lin(16, 64)
    m2.bias = nn.Parameter(torch.zeros(16, dtype=BF16))
    quantize_linear_(m2, "mxfp4")
    assert D._plain(m2) is None


# ------------------------------------------------------------------------------------------------------------------------ the GEMV cases
def test_dispatch_classes_are_in_the_table():
    cs = list(C.CASES.values())
    assert {C.pass_class(c.K, c.M) for c in cs} == {"one", "pairs", "single"}
    assert {c.M for c in cs} == {1, 2, 3, 4} and {len(c.ns) for c in cs} == {1, 2, 3}
    for epi in ("none", "res", "qkv", "swiglu"):
        assert {c.norm for c in cs if c.epi == epi} == {False, True}, epi
        assert any(c.ranks for c in cs if c.epi == epi), epi
    assert {r for c in cs for r in c.ranks} >= {8, 24, 64}
    ks = {c.K for c in cs}
    assert {32, C.PIECE, C.PIECE + 32, C.STEP, C.STEP + 32, 14336} <= ks
    assert any(c.N % 4 for c in cs) and any(c.strided for c in cs)
    assert C.launch_shape(8192)[:2] == (2048, 1) and C.launch_shape(8196)[:2] == (2049, 2) and C.launch_shape(2 * 4098, True)[:2] == (2049, 2)
    assert any(c.N == 8196 and c.K > C.STEP for c in cs)  # a wave's second group behind a two-step first one
    # the thresholds of the passes
    assert C.pass_class(14336, 2) == "one" and C.pass_class(14368, 2) == "single" and C.pass_class(14336, 4) == "pairs"
    assert C.pass_class(30720, 1) == "one" and C.pass_class(30752, 1) == "reject" and C.pass_class(2064, 1) == "reject"
    for what, K, M, rank in C.REJECTS:
        assert rank or C.passes(K, M) is None


@pytest.mark.parametrize("cid", [c for c in C.CASES if C.CASES[c].N * C.CASES[c].K <= 4_000_000])
def test_cases_are_exact(cid):
    """`reference` asserts its own exactness conditions; the operands are what the docstring says."""
    d = C.build(cid)
    c = d["case"]
    out = C.reference(d)
    assert out["out"].shape == (c.M, c.n_out) and out["out"].dtype is BF16
    for w, sc in zip(d["ws"], d["scales"]):
        assert int(sc.min()) >= 126 and int(sc.max()) <= 128
        if sc.shape[1] > 1:
            assert (sc[:, 1:] != sc[:, :-1]).all()
        if sc.shape[0] > 1:
            assert (sc[1:] != sc[:-1]).all()
        assert len(set((w & 15).flatten().tolist()) | set((w >> 4).flatten().tolist())) == 16 or w.numel() < 64


@pytest.mark.parametrize("fault", C.FAULTS)
def test_faults_are_caught(fault):
    """Every case aimed at a fault tells the faulty kernel from the right one, in the output (or the caches)."""
    assert set(C.FAULT_CASES) == set(C.FAULTS)
    for cid in C.FAULT_CASES[fault]:
        d = C.build(cid)
        good, bad = C.reference(d), C.reference(d, fault)
        differs = any(not torch.equal(good[k], bad[k]) for k in ("out", "kc", "vc") if k in good)
        assert differs, f"{fault} passes {cid}"
