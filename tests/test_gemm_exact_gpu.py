"""The GEMM family bit for bit: every case of tests/gemm_cases.py (operands on which the kernels' arithmetic has exactly one correct
answer) on the GPU with torch.equal as the bar - every tile class, loop shape, epilogue, stride and row limit of csrc/gemm_bf16.hip and
csrc/gemm_tn.hip.  Outputs sit in buffers with spare rows and columns prefilled with a sentinel bit pattern that must survive; operands
sit 16 bytes into allocations whose pad rows and pad columns hold NaN (int8: -128, a value no operand uses), which must reach no output.

Ids name the class (loop, rows, cols, strides, epilogue, tail, rowlimit, splitk, tn, ...), then kind, M x N x K + K2 and the epilogue.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gemm_cases as G  # noqa: E402

BF16 = torch.bfloat16
NAN = float("nan")


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


def _ids(cls):
    return [c.id for c in G.CASES + G.TN_CASES if c.cls == cls]


# ------------------------------------------------------------------------------------------------------------------------ buffers
def _embed(t, ld, dev, fill, col0=0, rows_after=2):
    """t [R, C] on the device as a view with row stride ld, 16 bytes into an allocation otherwise full of `fill` (pad columns, `rows_after`
    pad rows, the prefix); col0: t starts at column col0 of the ld-wide rows."""
    R, C = t.shape
    pre = 16 // t.element_size()
    buf = torch.full((pre + (R + rows_after) * ld + pre,), fill, dtype=t.dtype)
    buf.as_strided((R, C), (ld, 1), pre + col0).copy_(t)
    g = buf.to(dev)
    return g.as_strided((R, C), (ld, 1), pre + col0)


def _embed1(t, dev, fill):
    pre = 16 // t.element_size()
    buf = torch.full((t.numel() + 2 * pre,), fill, dtype=t.dtype)
    buf[pre : pre + t.numel()] = t
    return buf.to(dev)[pre : pre + t.numel()]


class Out:
    """An output [R, C] of 2-byte (bf16) or 4-byte (fp32) elements with row stride ld, spare rows and columns, prefilled with the sentinel."""

    def __init__(self, R, C, ld, dev, dtype=BF16, spare_rows=3):
        self.R, self.C, self.ld, self.dtype = R, C, ld, dtype
        self.idt = torch.int16 if dtype is BF16 else torch.int32
        self.pre = 16 // (2 if dtype is BF16 else 4)
        self.n = self.pre + (R + spare_rows) * ld + self.pre
        sent = G.SENT16 if dtype is BF16 else (G.SENT16 << 16 | G.SENT16)
        self.buf = torch.full((self.n,), sent, dtype=self.idt, device=dev)
        self.view = self.buf.view(dtype).as_strided((R, C), (ld, 1), self.pre)
        self.sent = sent

    def check(self, want, what, rows_exact=None, rows_kept_from=None):
        """Bits of [0:R, 0:C] equal `want`, everything else keeps the sentinel.  Row-limited launches: rows below rows_exact are exact,
        rows from rows_kept_from on keep the sentinel, the rows in between are unspecified by the ABI and not looked at."""
        got = self.buf.cpu()
        gv = got.as_strided((self.R, self.C), (self.ld, 1), self.pre)
        wv = want.contiguous().view(self.idt)
        lo = self.R if rows_exact is None else rows_exact
        hi = self.R if rows_kept_from is None else rows_kept_from
        if not torch.equal(gv[:lo], wv[:lo]):
            bad = (gv[:lo] != wv[:lo]).nonzero()
            r, q = bad[0].tolist()
            fl = (lambda t: t.view(self.dtype)[r, q].item())
            raise AssertionError(f"{what}: {len(bad)} of {wv[:lo].numel()} outputs differ in bits, in rows {bad[:, 0].min().item()}-{bad[:, 0].max().item()} "
                                 f"({bad[:, 0].unique().numel()} of them), columns {bad[:, 1].min().item()}-{bad[:, 1].max().item()} "
                                 f"({bad[:, 1].unique().numel()} of them); first at [{r}, {q}]: got {fl(gv[:lo].contiguous())}, expected {fl(wv[:lo])}")
        ref = torch.full((self.n,), self.sent, dtype=self.idt)
        rv = ref.as_strided((self.R, self.C), (self.ld, 1), self.pre)
        rv[:lo] = wv[:lo]
        rv[lo:hi] = gv[lo:hi]
        assert torch.equal(got, ref), f"{what}: {(got != ref).sum().item()} elements outside the output lost the sentinel"


def _bf(x):
    return x.to(BF16)


def _ordered(bits16):
    b = bits16.to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7FFF))


# ------------------------------------------------------------------------------------------------------------------------ NT
def _run_nt(K, dev, c):
    from llx import _lib as L

    d = G.operands(c.kind, c.M, c.N, c.K, c.K2, c.ext)
    s = G.strides(c)
    i8 = c.kind in ("i8", "i8f32")
    want = G.expected(c) if c.m_valid != 0 else {"out": torch.zeros(c.M, c.N, dtype=BF16)}
    a_t = d["a"].to(torch.int8) if i8 else _bf(d["a"])
    if c.m_valid is not None and c.m_valid < c.M:  # rows past the count hold NaN: the rows below it must not depend on them
        a_t = a_t.clone()
        a_t[c.m_valid:] = -128 if i8 else NAN
    fill = -128 if i8 else NAN
    a = _embed(a_t, s["lda"], dev, fill)
    b = _embed(d["b"].to(torch.int8) if i8 else _bf(d["b"]), s["ldb"], dev, fill)
    a2 = b2 = None
    if c.K2:
        a2 = _embed(_bf(d["a2"]), s["lda2"], dev, NAN, col0=s["a2_col0"])
        b2 = _embed(_bf(d["b2"]), s["ldb2"], dev, NAN)
    wide = 2 * c.N if c.epi == "swiglu_bwd" else c.N
    out = Out(c.M, wide, s["ldc"], dev, torch.float32 if c.kind == "i8f32" else BF16)
    e_cpu = G.epi_operand(c)
    e = h = None
    if e_cpu is not None:
        e = _embed1(_bf(e_cpu), dev, NAN) if e_cpu.dim() == 1 else _embed(_bf(e_cpu), s["lde"], dev, NAN)
    if c.epi == "swiglu_fwd":
        h = Out(c.M, c.N // 2, s["lde"], dev)
        e = h.view
    rope = None
    if c.epi == "rope":
        table = torch.cat([G.rope_table(), torch.full((3, 64, 2), NAN)]).to(dev)  # rows past rope_S are never a position
        rope = (table, G.ROPE_S, c.rope_cols)
    mv = None if c.m_valid is None else torch.tensor([c.m_valid], dtype=torch.int32, device=dev)
    code = 0 if c.epi == "rope" else G.EPI_CODE[c.epi]
    if c.kind == "bf16":
        K.gemm_nt(a, b, out=out.view, a2=a2, b2=b2, epilogue=code, e=e, rope=rope, m_valid=mv)
    elif c.kind == "i8":
        from subclasses.int8_mm import _launch

        _launch(a, b, _embed1(_bf(d["sa"]), dev, NAN), _embed1(_bf(d["sb"]), dev, NAN), out=out.view, a2=a2, b2=b2, epilogue=code, e=e, rope=rope)
    else:
        sa, sb = _embed1(d["sa"].float(), dev, NAN), _embed1(d["sb"].float(), dev, NAN)
        L.check(L.load().llx_int8_mm_dequant_f32(L.ptr(a), a.stride(0), L.ptr(b), b.stride(0), L.ptr(out.view), s["ldc"], c.M, c.N, c.K,
                                                 L.ptr(sa), L.ptr(sb), L.stream()), "llx_int8_mm_dequant_f32")
    torch.cuda.synchronize()
    rows_exact = rows_kept = None
    if c.m_valid is not None:
        rows_exact = min(c.m_valid, c.M)
        rows_kept = min(c.M, -(-c.m_valid // 256) * 256)
    if c.epi == "gelu":
        got = out.view.cpu()
        out.check(got, c.id)  # the sentinel around it
        dist = (_ordered(got.view(torch.int16)) - _ordered(want["out"].view(torch.int16))).abs()
        off1, far = (dist == 1).float().mean().item(), (dist > 1).float().mean().item()
        zfar = want["z"].float()[dist > 1]
        print(f"\n{c.id}: bias+GELU outputs one bf16 neighbour off {off1:.4%}, further off {far:.4%}"
              + (f" (all of them at z in [{zfar.min().item()}, {zfar.max().item()}])" if far else ""))
        assert far == 0, (f"{c.id}: {far:.4%} of the outputs are more than one bf16 neighbour from bf16(gelu_float64(z)), "
                          f"all at z in [{zfar.min().item()}, {zfar.max().item()}]; one neighbour off: {off1:.4%}")
        return
    if c.epi == "swiglu_bwd":
        # dg|du = the stand-alone kernel on the exact dh
        N = c.N
        ref = torch.empty(c.M, 2 * N, dtype=BF16, device=dev)
        eg = _bf(e_cpu).to(dev)
        K.swiglu_bwd(want["dh"].to(dev), eg[:, :N], eg[:, N:], ref[:, :N], ref[:, N:])
        out.check(ref.cpu(), c.id)
        return
    out.check(want["out"], c.id, rows_exact, rows_kept)
    if c.epi == "swiglu_fwd":
        gu = want["out"].to(dev)
        h.check(K.swiglu_fwd(gu[:, : c.N // 2], gu[:, c.N // 2:]).cpu(), c.id + " (h)")


@pytest.mark.parametrize("cid", _ids("loop"))
def test_loop(K, cuda, cid):
    """Zero, one and several steady iterations, both stage parities at the loop exit, 0-4 extension tiles; bf16, int8, int8 with f32 scales."""
    _run_nt(K, cuda, G.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids("rows"))
def test_rows(K, cuda, cid):
    _run_nt(K, cuda, G.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids("cols"))
def test_cols(K, cuda, cid):
    _run_nt(K, cuda, G.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids("strides"))
def test_strides(K, cuda, cid):
    _run_nt(K, cuda, G.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids("epilogue"))
def test_epilogue(K, cuda, cid):
    _run_nt(K, cuda, G.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids("gelu"))
def test_bias_gelu(K, cuda, cid):
    """Bias + GELU: the pre-activation z = bf16(bf16(acc) + bias) is exact (integers here), and the output is asked to lie within one bf16
    neighbour of bf16(gelu_float64(z)) - erff is not correctly rounded, so no tighter bar is free of the code under test.

    Measured on the MI355X: every output of the three shapes equals bf16(gelu_float64(z)) bit for bit (none one neighbour off).  The bar
    found a fault: with the epilogue's former 0.5 z (1 + erff(z / sqrt 2)) 0.26 % (256 x 256, 257 x 264) and 0.56 % (129 x 65792) of the
    outputs were further off, all at integer z in [-13, -5], where 1 + erff cancels in fp32 (-0 where float64 has -6e-9 ... -8e-38);
    gelu_erf (gemm_bf16.hip) now goes through erfcf."""
    _run_nt(K, cuda, G.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids("tail"))
def test_tail(K, cuda, cid):
    """The launcher's relaunch of the last columns with 256 x 128 half tiles, and the shapes just outside its conditions."""
    _run_nt(K, cuda, G.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids("rowlimit"))
def test_rowlimit(K, cuda, cid):
    _run_nt(K, cuda, G.BY_ID[cid])


# ------------------------------------------------------------------------------------------------------------------------ split-K
@pytest.mark.parametrize("cid", _ids("splitk"))
def test_splitk(K, cuda, cid):
    from llx import _lib as L

    c = G.BY_ID[cid]
    d = G.operands(c.kind, c.M, c.N, c.K, c.K2, False)
    a_t = _bf(d["a"])
    rows = c.M if c.m_valid is None else c.m_valid
    if rows < c.M:
        a_t = a_t.clone()
        a_t[rows:] = NAN
    a, b = _embed(a_t, c.K + 8, cuda, NAN), _embed(_bf(d["b"]), c.K + 8, cuda, NAN)
    part = Out(c.splits * c.M, c.N, c.N, cuda, torch.float32, spare_rows=1)   # [splits][M][N], row stride N
    out = Out(c.M, c.N, c.N + 8, cuda)
    mv = None if c.m_valid is None else torch.tensor([c.m_valid], dtype=torch.int32, device=cuda)
    inv = G.sk_inv(c).to(cuda) if c.inv else None
    sc = torch.tensor([G.SK_SCALE], dtype=torch.float32, device=cuda) if c.scale else None
    lib = L.load()
    L.check(lib.llx_gemm_nt_bf16_splitk(L.ptr(a), a.stride(0), L.ptr(b), b.stride(0), L.ptr(part.view), c.M, c.N, c.K, c.splits, L.ptr(mv), L.stream()),
            "llx_gemm_nt_bf16_splitk")
    L.check(lib.llx_splitk_combine(L.ptr(part.view), c.splits, c.M, c.N, L.ptr(inv), L.ptr(sc), L.ptr(out.view), c.N + 8, L.stream()), "llx_splitk_combine")
    torch.cuda.synchronize()
    kr = c.K // c.splits
    want_part = torch.stack([d["a"][:, i * kr:(i + 1) * kr] @ d["b"][:, i * kr:(i + 1) * kr].T for i in range(c.splits)]).float()
    got = part.buf.cpu().as_strided((c.splits, c.M, c.N), (c.M * c.N, c.N, 1), part.pre)
    kept = min(c.M, -(-rows // 256) * 256)
    assert torch.equal(got[:, :rows], want_part[:, :rows].view(torch.int32)), f"{cid}: fp32 partial products"
    assert bool((got[:, kept:] == part.sent).all()), f"{cid}: partial rows past the row limit's tile were written"
    head, tail = part.buf[: part.pre].cpu(), part.buf[part.pre + c.splits * c.M * c.N:].cpu()
    assert bool((head == part.sent).all()) and bool((tail == part.sent).all()), f"{cid}: bytes around the partial products"
    out.check(G.expected(c)["out"], cid)


# ------------------------------------------------------------------------------------------------------------------------ TN
def _run_tn(dev, c):
    from llx import _lib as L

    m = c.m_eff
    ops = []
    for which, n in (("a", c.N1), ("b", c.N2)):
        if c.form == "im2col":
            x, _ = G.tn_im2col_source(c, which)
            ops.append(_embed1(_bf(x), dev, NAN).as_strided((c.M, n), (88, 1)))
            continue
        t = _bf(G.tn_operands(c)[0 if which == "a" else 1]).clone()
        t[m:] = NAN      # rows past the count: NaN and Inf alternate
        t[m + 1:: 2] = float("inf")
        ops.append(_embed(t, n + (72 if c.form == "slice" else 8), dev, NAN))
    a, b = ops
    out = Out(c.N1, c.N2, c.N2 + 8, dev)
    mv = None if c.m_valid is None else torch.tensor([c.m_valid], dtype=torch.int32, device=dev)
    L.check(L.load().llx_gemm_tn_bf16_rows(L.ptr(a), a.stride(0), L.ptr(b), b.stride(0), L.ptr(out.view), c.N2 + 8, c.M, c.N1, c.N2, L.ptr(mv),
                                           L.stream()), "llx_gemm_tn_bf16_rows")
    torch.cuda.synchronize()
    out.check(G.tn_expected(c), c.id)


@pytest.mark.parametrize("cid", _ids("tn"))
def test_tn(cuda, cid):
    _run_tn(cuda, G.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids("tn-strided"))
def test_tn_strided(cuda, cid):
    _run_tn(cuda, G.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids("tn-rowlimit"))
def test_tn_rowlimit(cuda, cid):
    _run_tn(cuda, G.BY_ID[cid])
