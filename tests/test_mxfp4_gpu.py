"""GPU: the MXFP4 kernels (csrc/mxfp4.hip) against the oracle of tests/mx_cases.py, bit for bit.  The quantiser on hand vectors and random
matrices (bf16 and fp32, strided, the device result equal to the host's), the dequantiser plain and transposed, and the decode GEMV on
packed rows (llx.kernels.gemv with mxscale) at every dispatch class of the case table: on those operands the fp32 sums do not depend on
their order, so the float64 reference is the one correct answer and torch.equal is the bar (tests/test_mx_cases.py shows on the CPU that
each case is exact and that the planted faults would fail here).  Output buffers are compared whole: gaps and unwritten cache rows keep
their sentinel.  On the same operands the result also equals llx_gemv_bf16 on the dequantised image."""
import pytest
import torch

from oracle import ref as O

pytestmark = pytest.mark.gpu

from tests import mx_cases as C  # noqa: E402
from tests.test_gemv_classes_gpu import _dev, _mismatch, _whole  # noqa: E402

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


# ------------------------------------------------------------------------------------------------------------------------ quantiser
def test_quantiser_hand_vectors(K, cuda):
    for name, x, codes, b in C.HAND:
        packed, scale = K.quantize_mxfp4(x.to(cuda))
        assert int(scale.cpu()) == b, f"{name}: scale byte {int(scale.cpu())} != {b}"
        assert torch.equal(packed.cpu(), C._pack(codes.view(1, 32))), f"{name}: {packed.cpu().tolist()}"


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("Kd", [32, 64, 2048, 2080])
def test_quantiser_equals_oracle_and_host(K, cuda, dtype, N, Kd):
    """Random values over many binades with zeros and a zero block, contiguous and as a column slice of a wider matrix."""
    from subclasses.mxfp4 import MXFP4LinearWeight, quantize_mxfp4

    KB = Kd // 32
    x = O.randn(f"mxg_{N}_{Kd}", (N, Kd), 1.0) * torch.exp2(O.randint(f"mxg_e_{N}_{Kd}", (N, KB), -30, 31).float()).repeat_interleave(32, 1)
    x[0, ::5] = 0
    x[-1, -32:] = 0
    x = x.to(dtype)
    want_p, want_s = C.quantize(x)
    host_p, host_s = quantize_mxfp4(x)
    assert torch.equal(host_p, want_p) and torch.equal(host_s, want_s)
    wide = torch.full((N, Kd + 24), float("nan"), dtype=dtype)
    wide[:, 8:8 + Kd] = x
    for what, xd in (("contiguous", x.to(cuda)), ("strided", wide.to(cuda)[:, 8:8 + Kd])):
        p, s = K.quantize_mxfp4(xd)
        assert p.shape == (N, Kd // 2) and s.shape == (N, KB) and p.dtype is torch.uint8 and s.dtype is torch.uint8
        assert torch.equal(s.cpu(), want_s), f"{what}: scale bytes"
        assert torch.equal(p.cpu(), want_p), f"{what}: " + _mismatch(p.cpu(), want_p)
    w = MXFP4LinearWeight.from_float(x.to(cuda))
    assert w.is_cuda and torch.equal(w.packed.cpu(), want_p) and torch.equal(w.scale.cpu(), want_s)
    moved = MXFP4LinearWeight.from_float(x).to(cuda)
    assert isinstance(moved, MXFP4LinearWeight) and moved.packed.is_cuda and torch.equal(moved.packed.cpu(), want_p)


def test_from_float_refuses_non_finite_on_device(cuda):
    from llx._lib import LlxError
    from subclasses.mxfp4 import MXFP4LinearWeight

    x = torch.ones(4, 64, device=cuda, dtype=BF16)
    x[1, 3] = float("inf")
    with pytest.raises(LlxError, match="non-finite"):
        MXFP4LinearWeight.from_float(x)


# ------------------------------------------------------------------------------------------------------------------------ dequantiser
@pytest.mark.parametrize("N,Kd", [(1, 32), (5, 64), (37, 2080), (300, 96)])
def test_dequantiser_plain_and_transposed(K, cuda, N, Kd):
    """All 16 codes under scale bytes from both ends and the middle; the image into a fresh tensor and into a slice of a wider one whose
    other columns keep their sentinel."""
    codes = O.randint(f"mxd_{N}_{Kd}", (N, Kd), 0, 16).to(torch.uint8)
    scale = torch.tensor([2, 3, 100, 126, 127, 128, 200, 251, 252], dtype=torch.uint8)[O.randint(f"mxd_s_{N}_{Kd}", (N, Kd // 32), 0, 9)]
    packed = C._pack(codes)
    want = C.dequantize(packed, scale)
    pd, sd = packed.to(cuda), scale.to(cuda)
    got = K.dequantize_mxfp4(pd, sd)
    assert got.dtype is BF16 and torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))
    got_t = K.dequantize_mxfp4(pd, sd, transpose=True)
    assert got_t.shape == (Kd, N) and torch.equal(got_t.cpu().view(torch.int16), want.T.contiguous().view(torch.int16))
    wide = torch.full((N, Kd + 16), C.SENTINEL, device=cuda, dtype=BF16)
    K.dequantize_mxfp4(pd, sd, out=wide[:, 8:8 + Kd])
    exp = torch.full((N, Kd + 16), C.SENTINEL, dtype=BF16)
    exp[:, 8:8 + Kd] = want
    assert torch.equal(wide.cpu().view(torch.int16), exp.view(torch.int16))
    wide_t = torch.full((Kd, N + 3), C.SENTINEL, device=cuda, dtype=BF16)
    K.dequantize_mxfp4(pd, sd, transpose=True, out=wide_t[:, 1:1 + N])
    exp_t = torch.full((Kd, N + 3), C.SENTINEL, dtype=BF16)
    exp_t[:, 1:1 + N] = want.T
    assert torch.equal(wide_t.cpu().view(torch.int16), exp_t.view(torch.int16))
    from subclasses.mxfp4 import MXFP4LinearWeight

    assert torch.equal(MXFP4LinearWeight(pd, sd).dequantize().cpu().view(torch.int16), want.view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------------ the GEMV
def _operands(K, d, cuda, seg=None, image=False):
    """(ws, x, keyword arguments, output buffers by name) of K.gemv for a case; seg: only that weight, as a GV_NONE launch; image: the
    bf16 call on the dequantised images instead of the packed rows."""
    c = d["case"]
    segs = range(len(c.ns)) if seg is None else [seg]
    if image:
        ws, kw = [C.dequantize(d["ws"][s].contiguous(), d["scales"][s].contiguous()).to(cuda) for s in segs], {}
    else:
        ws, kw = [_dev(d["ws"][s], cuda)[1] for s in segs], dict(mxscale=[_dev(d["scales"][s], cuda)[1] for s in segs])
    x = _dev(d["x"], cuda)[1]
    bufs = {}
    if c.norm:
        kw["norm"] = (d["norm_w"].to(cuda), C.EPS)
    if c.ranks:
        t = _dev(d["t"], cuda)[1]
        if seg is not None:
            off = sum(c.ranks[:seg])
            t = t[:, off:off + c.ranks[seg]]
        kw["lora"] = ([d["bext"][s].to(cuda) for s in segs], t, c.lscale)
    if seg is not None:
        return ws, x, kw, bufs
    kw["epilogue"] = {"none": K.GV_NONE, "res": K.GV_RESIDUAL, "qkv": K.GV_QKV, "swiglu": K.GV_SWIGLU}[c.epi]
    bufs["out"], kw["out"] = _dev(d["out"], cuda)
    if c.epi == "res":
        kw["res"] = _dev(d["res"], cuda)[1]
    if c.epi == "qkv":
        bufs["kc"], kc = _dev(d["kc"], cuda)
        bufs["vc"], vc = _dev(d["vc"], cuda)
        kw["qkv"] = (d["rope"].to(cuda), 256, (c.N - 256) // 2, kc, vc, d["pos"].to(cuda))
    return ws, x, kw, bufs


@pytest.mark.parametrize("cid", list(C.CASES))
def test_gemv_class(K, cuda, cid):
    d = C.build(cid)
    c = d["case"]
    want = C.reference(d)
    ws, x, kw, bufs = _operands(K, d, cuda)
    got = K.gemv(ws, x, **kw)
    assert got.data_ptr() == kw["out"].data_ptr() and got.shape == (c.M, c.n_out)
    out = bufs["out"].cpu()
    # the bf16 GEMV on the dequantised image: the same buffers, bit for bit
    ws_i, x_i, kw_i, bufs_i = _operands(K, d, cuda, image=True)
    K.gemv(ws_i, x_i, **kw_i)
    for name in bufs:
        assert torch.equal(bufs[name].cpu(), bufs_i[name].cpu()), f"{cid} {name}: differs from llx_gemv_bf16 on the image: " + _mismatch(bufs[name].cpu(), bufs_i[name].cpu())
    if c.epi == "qkv":
        for name in ("kc", "vc"):
            g = bufs[name].cpu()
            assert torch.equal(g, want[name]), f"{cid} {name}: " + _mismatch(g, want[name])
    if c.epi != "swiglu":
        exp = _whole(d, want["out"])
        assert torch.equal(out, exp), f"{cid}: " + _mismatch(out, exp)
        return
    # SwiGLU: gate and up through GV_NONE launches of the same operands are exact ...
    I = c.ns[0]
    gu = []
    for s, name in enumerate(("g", "u")):
        ws1, x1, kw1, _ = _operands(K, d, cuda, seg=s)
        v = K.gemv(ws1, x1, **kw1)
        assert torch.equal(v.cpu(), want[name]), f"{cid} {name}: " + _mismatch(v.cpu(), want[name])
        gu.append(torch.nn.functional.pad(v, (0, -I % 8)))
    # ... h equals the stand-alone kernel on them bit for bit, the gaps keep their sentinel ...
    h_alone = K.swiglu_fwd(gu[0], gu[1])[:, :I].cpu()
    exp = _whole(d, h_alone)
    assert torch.equal(out, exp), f"{cid}: " + _mismatch(out, exp)
    # ... and stays within the derived bar of float64
    err = (got.cpu().double() - want["h64"]).abs()
    ratio = (err / C.swiglu_bar(want["h64"])).max().item()
    print(f"[mxfp4 gemv {cid}] SwiGLU error / bar {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("what,Kd,M,rank", C.REJECTS)
def test_gemv_rejects(K, cuda, what, Kd, M, rank):
    """LlxError from the host checks, nothing written."""
    from llx._lib import LlxError

    assert rank or C.passes(Kd, M) is None
    w = torch.zeros(8, Kd // 2, device=cuda, dtype=torch.uint8)
    sc = torch.full((8, Kd // 32), 127, device=cuda, dtype=torch.uint8)
    x = torch.ones(M, Kd, device=cuda, dtype=BF16)
    out = torch.full((M, 8), C.SENTINEL, device=cuda, dtype=BF16)
    kw = {}
    if rank:
        kw["lora"] = ([torch.ones(8, rank, device=cuda, dtype=BF16)], torch.ones(M, rank, device=cuda, dtype=BF16), 1.0)
    with pytest.raises(LlxError, match=what):
        K.gemv([w], x, out=out, mxscale=[sc], **kw)
    assert (out.cpu().float() == C.SENTINEL).all()
    with pytest.raises(LlxError, match="excludes"):
        K.gemv([w], x[:1], mxscale=[sc], dynamic=True)
