"""GPU: the decode GEMV (csrc/decode.hip, csrc/wstream.h through llx.kernels.gemv) at every dispatch class of tests/gemv_cases.py, bit
for bit.  On those operands the kernel's fp32 sums do not depend on their order and every rounding point is a single correctly rounded
operation, so the float64 reference is the one correct answer and torch.equal is the bar (tests/test_gemv_cases.py shows on the CPU
that each case is exact and that the planted faults would fail here).  Output buffers are compared whole: the gaps of a strided `out`
and every cache element outside the written rows keep their sentinel.  SwiGLU, whose sigmoid is not exact, must equal the stand-alone
swiglu_fwd kernel applied to the (exact) gate and up outputs bit for bit and stay within the derived bar of float64."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gemv_cases as C  # noqa: E402


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


def _dev(t, cuda):
    """(the device copy of the whole underlying buffer, the same view of it)."""
    base = t._base if t._base is not None else t
    assert base.is_contiguous() and base.storage_offset() == 0
    bd = base.to(cuda)
    return bd, torch.as_strided(bd, t.size(), t.stride(), t.storage_offset())


def _operands(K, d, cuda, seg=None, epilogue=None):
    """(ws, x, keyword arguments, the output buffers by name) of K.gemv for a case; seg: only that weight, as a GV_NONE launch."""
    c = d["case"]
    segs = range(len(c.ns)) if seg is None else [seg]
    ws = [_dev(d["ws"][s], cuda)[1] for s in segs]
    x = _dev(d["x"], cuda)[1]
    kw, bufs = {}, {}
    if c.norm:
        kw["norm"] = (d["norm_w"].to(cuda), C.EPS)
    if c.kind in ("i8w", "i8d"):
        kw["wscale"] = [d["wscale"][s].to(cuda) for s in segs]
        kw["dynamic"] = c.kind == "i8d"
    if c.kind == "dora":
        kw["colscale"] = [d["colscale"][s].to(cuda) for s in segs]
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


def _whole(d, want):
    """The expected content of the whole `out` buffer: the reference inside the view, the sentinel in the gaps."""
    base = d["out"]._base.clone()
    torch.as_strided(base, d["out"].size(), d["out"].stride(), d["out"].storage_offset()).copy_(want)
    return base


def _mismatch(got, want):
    bad = torch.nonzero(got.float() != want.float())
    return f"{bad.shape[0]} of {want.numel()} elements differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])].item()} want {want[tuple(bad[0])].item()}"


@pytest.mark.parametrize("cid", list(C.CASES))
def test_gemv_class(K, cuda, cid):
    d = C.build(cid)
    c = d["case"]
    want = C.reference(d)
    ws, x, kw, bufs = _operands(K, d, cuda)
    got = K.gemv(ws, x, **kw)
    assert got.data_ptr() == kw["out"].data_ptr() and got.shape == (c.M, c.n_out)
    out = bufs["out"].cpu()
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
    print(f"[gemv {cid}] SwiGLU error / bar {ratio:.3f}; {(got.cpu() != want['out']).sum().item()} of {got.numel()} off the float64 rounding")
    assert ratio <= 1.0


@pytest.mark.parametrize("what,kind,Kd,M,rank", C.REJECTS)
def test_gemv_rejects(K, cuda, what, kind, Kd, M, rank):
    """LlxError from the host checks, nothing written."""
    from llx._lib import LlxError

    assert rank or C.passes(kind, Kd, M) is None
    i8 = kind == "i8w"
    w = torch.ones(8, Kd, device=cuda, dtype=torch.int8 if i8 else torch.bfloat16)
    x = torch.ones(M, Kd, device=cuda, dtype=torch.bfloat16)
    out = torch.full((M, 8), C.SENTINEL, device=cuda, dtype=torch.bfloat16)
    kw = dict(wscale=[torch.ones(8, device=cuda, dtype=torch.bfloat16)]) if i8 else {}
    if rank:
        kw["lora"] = ([torch.ones(8, rank, device=cuda, dtype=torch.bfloat16)], torch.ones(M, rank, device=cuda, dtype=torch.bfloat16), 1.0)
    with pytest.raises(LlxError, match=what):
        K.gemv([w], x, out=out, **kw)
    assert (out.cpu().float() == C.SENTINEL).all()
