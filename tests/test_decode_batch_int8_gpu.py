"""GPU: the batched decode stream on dynamic-int8 linears (csrc/decode_rows.hip: llx_gemm_rows16_i8) - the weight-streaming MFMA
product for 2..16 activation rows on int8 weight rows, the rows of x quantised in the prologue, against the oracle's int8 linear
(oracle/ref.py restating subclasses/int8.py:106-121 and int8_mm.py:93-118) and against the GEMV on the same operands.
Without a fused norm the target is bit-exact: the quantiser is int8_quant.hip's, int32 sums do not depend on their order and the
dequantisation has the reference's two fp32 products.  With the fused norm the on-chip sum of squares can move a normalised value by
one bf16 ulp and with it an int8 code: the bars of tests/test_decode_int8_gpu.py and tests/test_decode_batch_gpu.py."""
import functools

import pytest
import torch

from oracle import ref as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


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
def _operands(K_, ns):
    """Quantised weights, 16 activation rows, norm weight and residual of one (K, segments) case with the oracle's outputs for all 16
    rows, without and with the norm: computed once, shared by the M cases (row m of the product does not depend on M)."""
    qs = [_qweight(f"r8_w{i}_{K_}_{n}", n, K_) for i, n in enumerate(ns)]
    x = O.randn(f"r8_x_{K_}", (16, K_), 1.0).to(BF)
    nw = (1 + O.randn(f"r8_n{K_}", (K_,), 0.1)).to(BF)
    res = O.randn(f"r8_r_{sum(ns)}", (16, sum(ns)), 1.0).to(BF)
    wi, sc = torch.cat([q for q, _ in qs]), torch.cat([s for _, s in qs])
    def lin(xin):  # (in chunks of weight rows: the oracle's integer product goes through an fp64 image of the weights)
        return torch.cat([O.int8_linear(xin, wi[i : i + 4096], sc[i : i + 4096], dynamic=True) for i in range(0, wi.shape[0], 4096)], 1)

    want = {False: lin(x), True: lin(O.rmsnorm(x, nw, 1e-5))}
    return qs, x, nw, res, want


def _dev(qs, cuda):
    return dict(ws=[q.to(cuda) for q, _ in qs], wscale=[s.to(cuda) for _, s in qs])


# (K, segments): with M they fix every dispatch decision of the launcher (rows16_plan in csrc/decode_rows.hip, int8 sizes: batches of
# 512 elements, an LDS image of M x KS bytes):
#   tiles    ceil(N / 16), the last one partly filled (N = 36: 3 tiles, 4 live rows in the last; 33000: 2063 tiles) or all full;
#   slices   S = 1, no hand-off between workgroups (K = 512); S = 3 with slices of 512, 512 and 16 elements - a last batch that runs
#            past K and a k-step with 16 of 64 live elements (K = 1040); S = 8 equal slices of one batch (K = 4096 with 48 tiles in
#            three segments, and with 256 tiles: exactly 2048 wave items); S = 28, the floor of one batch per slice (K = 14336,
#            N = 36); K = 14336 with N = 4096: 8 slices asked, 14 is the first equal cut - slices of 1024 = 2 batches per item, so the
#            two register sets swap inside an item and across items; S = 2 in the SwiGLU and q|k|v tests;
#   tiles per wave: 1 (ntiles * S <= 2048) or 2 (N = 33000 at K = 512: 2063 items; N = 4096 at K = 14336: 3584 items);
#   LDS cap  at M = 16 a slice is at most 3584 elements (16 rows of codes within 60 KiB), at M = 2 whole rows fit.  It decides S only
#            where the tiles alone would ask for fewer slices: test_rows16_i8_lds_cap_decides_the_split below.
CASES = [(512, (36,)), (512, (33000,)), (1040, (36,)), (4096, (512, 128, 128)), (4096, (4096,)), (14336, (36,)), (14336, (4096,))]


def _check_case(K, cuda, M, K_, ns):
    qs, x, nw, res, want16 = _operands(K_, ns)
    w, xd, rd, nd = _dev(qs, cuda), x[:M].to(cuda), res[:M].to(cuda), (nw.to(cuda), 1e-5)
    want = want16[False][:M]
    got = K.gemm_rows16(x=xd, **w)
    assert got.dtype is BF and got.shape == want.shape
    assert torch.equal(got.cpu(), want), f"int8 rows16: {(got.cpu().float() - want.float()).abs().max().item():.4e} off the bit-exact target"
    got_r = K.gemm_rows16(x=xd, epilogue=K.GV_RESIDUAL, res=rd, **w)
    assert torch.equal(got_r.cpu(), (want.float() + res[:M].float()).to(BF)), "int8 rows16 + residual"
    want_n = want16[True][:M].float()
    got_n = K.gemm_rows16(x=xd, norm=nd, **w)
    _close(got_n.float().cpu(), want_n, 0.01, "norm + int8 rows16")
    got_nr = K.gemm_rows16(x=xd, norm=nd, epilogue=K.GV_RESIDUAL, res=rd, **w)
    _close(got_nr.float().cpu(), want_n.to(BF).float() + res[:M].float(), 0.01, "norm + int8 rows16 + residual")
    # repeat launches are bit-identical
    assert torch.equal(got, K.gemm_rows16(x=xd, **w)) and torch.equal(got_r, K.gemm_rows16(x=xd, epilogue=K.GV_RESIDUAL, res=rd, **w))
    assert torch.equal(got_n, K.gemm_rows16(x=xd, norm=nd, **w)) and torch.equal(got_nr, K.gemm_rows16(x=xd, norm=nd, epilogue=K.GV_RESIDUAL, res=rd, **w))


@pytest.mark.parametrize("K_,ns", CASES)
@pytest.mark.parametrize("M", [2, 5, 16])
def test_rows16_i8_plain_and_residual(K, cuda, M, K_, ns):
    """out = int8_linear([rmsnorm(x) | x], [W0; W1; W2]) (+ residual) for two rows, a partly filled operand and a full one: the
    oracle's bits without the norm, 1 % with it; a second launch is bit-identical."""
    _check_case(K, cuda, M, K_, ns)


@pytest.mark.parametrize("M", [2, 16])
def test_rows16_i8_lds_cap_decides_the_split(K, cuda, M):
    """K = 8192, N = 16400 (1025 full tiles): the tiles alone ask for 2 slices.  At M = 2 that is what runs (S = 2, slices of 4096); at
    M = 16 the image of 16 rows of codes allows slices of at most 3584 elements, so the cap asks for 3 and the launcher takes 4 equal
    slices of 2048 - the branch the 8B w2 product (K = 14336) takes at M = 16."""
    _check_case(K, cuda, M, 8192, (16400,))


@pytest.mark.parametrize("K_", [512, 1040])
def test_rows16_i8_row_scales_do_not_leak(K, cuda, K_):
    """One all-zero row (scale 0, divisor 1e-12: zero codes, a zero output) and one row 1000 times larger than the others: every row is
    quantised with its own absmax and dequantised with its own scale, in the main kernel (K = 512) and in the combine launch (1040)."""
    qs = [_qweight(f"r8_w0_{K_}_36", 36, K_)]
    x = O.randn(f"r8_xs_{K_}", (5, K_), 1.0)
    x[1] = 0
    x[3] *= 1000
    x = x.to(BF)
    res = O.randn("r8_rs", (5, 36), 1.0).to(BF)
    want = O.int8_linear(x, qs[0][0], qs[0][1], dynamic=True)
    assert torch.equal(want[1], torch.zeros(36, dtype=BF)) and want[3].abs().max() > 100 * want[0].abs().max()
    w, xd = _dev(qs, cuda), x.to(cuda)
    got = K.gemm_rows16(x=xd, **w)
    assert torch.equal(got.cpu(), want), f"{(got.cpu().float() - want.float()).abs().max(1).values.tolist()} per row off the bit-exact target"
    got_r = K.gemm_rows16(x=xd, epilogue=K.GV_RESIDUAL, res=res.to(cuda), **w)
    assert torch.equal(got_r.cpu(), (want.float() + res.float()).to(BF))
    assert torch.equal(got_r[1].cpu(), res[1])  # the zero row: the residual alone
    assert torch.equal(got, K.gemm_rows16(x=xd, **w))
    # with the norm the zero row stays zero (rstd = 1 / sqrt(eps) times zeros)
    nw = (1 + O.randn(f"r8_ns_{K_}", (K_,), 0.1)).to(BF)
    got_n = K.gemm_rows16(x=xd, norm=(nw.to(cuda), 1e-5), **w)
    _close(got_n.float().cpu(), O.int8_linear(O.rmsnorm(x, nw, 1e-5), qs[0][0], qs[0][1], dynamic=True).float(), 0.01, "norm + int8 rows16")
    assert torch.equal(got_n[1].cpu(), torch.zeros(36, dtype=BF))


@pytest.mark.parametrize("K_", [512, 1040])
def test_rows16_i8_agrees_with_the_gemv_bit_for_bit(K, cuda, K_):
    """Without a norm, row m of the batched stream is the GEMV's output for that row alone, bit for bit, through all four epilogues
    (integer sums are exact, both dequantise and round at the same points): K = 512 runs the epilogue in the main kernel, K = 1040 in
    the combine launch.  q|k|v: table row 5 handed in as row 0 (row 0 itself is the identity rotation), the GEMV writes row m into
    slot m of its own 16-slot caches; the caches are compared whole, so every element outside (m, pos[m]) - the slots >= M included -
    keeps the sentinel in both."""
    M = 5
    x = O.randn(f"r8_ag_x{K_}", (M, K_), 1.0).to(BF)
    xd = x.to(cuda)
    res = O.randn("r8_ag_r", (M, 36), 1.0).to(BF).to(cuda)
    w36 = _dev([_qweight(f"r8_w0_{K_}_36", 36, K_)], cuda)
    wsw = _dev([_qweight(f"r8_ag_w{i}_{K_}", 20, K_) for i in (1, 3)], cuda)
    H, KVH, hd, Smax, B = 1, 1, 128, 96, 16
    wqkv = _dev([_qweight(f"r8_ag_q{i}_{K_}", 128, K_) for i in range(3)], cuda)
    table = O.rope_table(O.TINY._replace(max_seq_len=Smax))[5:].contiguous().to(cuda)
    pos = torch.tensor([0, Smax - 1, 70, 3, 41]).to(cuda)
    sentinel = torch.full((B, KVH, Smax, hd), -7.25, dtype=BF)

    def rows(fn):
        return torch.cat([fn(m) for m in range(M)])

    for _ in range(2):  # the second round: repeat launches
        got = K.gemm_rows16(x=xd, **w36)
        assert torch.equal(got, rows(lambda m: K.gemv(x=xd[m : m + 1], dynamic=True, **w36))), "plain"
        got = K.gemm_rows16(x=xd, epilogue=K.GV_RESIDUAL, res=res, **w36)
        assert torch.equal(got, rows(lambda m: K.gemv(x=xd[m : m + 1], dynamic=True, epilogue=K.GV_RESIDUAL, res=res[m : m + 1], **w36))), "residual"
        got = K.gemm_rows16(x=xd, epilogue=K.GV_SWIGLU, **wsw)
        assert got.shape == (M, 20)
        assert torch.equal(got, rows(lambda m: K.gemv(x=xd[m : m + 1], dynamic=True, epilogue=K.GV_SWIGLU, **wsw))), "swiglu"
        kc_b, vc_b, kc_g, vc_g = (sentinel.to(cuda) for _ in range(4))
        got = K.gemm_rows16(x=xd, epilogue=K.GV_QKV, qkv=(table, H * hd, KVH * hd, kc_b, vc_b, pos), **wqkv)
        ref = rows(lambda m: K.gemv(x=xd[m : m + 1], dynamic=True, epilogue=K.GV_QKV,
                                    qkv=(table, H * hd, KVH * hd, kc_g[m : m + 1], vc_g[m : m + 1], pos[m : m + 1]), **wqkv))
        assert torch.equal(got, ref), "q rows"
        assert torch.equal(kc_b, kc_g) and torch.equal(vc_b, vc_g), "caches"
        assert torch.equal(kc_b[M:].cpu(), sentinel[M:]) and torch.equal(vc_b[M:].cpu(), sentinel[M:]), "slots >= M"
        written = kc_b.cpu()[torch.arange(M), :, pos.cpu()]
        assert not (written == -7.25).all(), "k rows were not written"


@pytest.mark.parametrize("M", [2, 16])
@pytest.mark.parametrize("D", [512, 1024])
def test_rows16_i8_swiglu(K, cuda, M, D):
    """gate|up on int8 rows with the norm and the SwiGLU epilogue (g, u and silu(g) rounded to bf16, then the product): a tile is the
    gate and up rows of 8 hidden units, each with its own weight scale; I = 1796 leaves 4 live units in the last tile.  D = 512 is one
    K slice (the epilogue runs in the main kernel), D = 1024 is split in two (the combine launch).  Bar: test_rows16_swiglu's."""
    I = 1796
    (q1, s1), (q3, s3) = (_qweight(f"r8_sw{i}_{D}", I, D) for i in (1, 3))
    x = O.randn(f"r8_swx{D}", (16, D), 1.0).to(BF)[:M]
    nw = (1 + O.randn(f"r8_swn{D}", (D,), 0.1)).to(BF)
    xb = O.rmsnorm(x, nw, 1e-5)
    g, u = O.int8_linear(xb, q1, s1, dynamic=True).float(), O.int8_linear(xb, q3, s3, dynamic=True).float()
    want = torch.nn.functional.silu(g.to(BF).float()).to(BF).float() * u.to(BF).float()
    kw = dict(ws=[q1.to(cuda), q3.to(cuda)], wscale=[s1.to(cuda), s3.to(cuda)], x=x.to(cuda), norm=(nw.to(cuda), 1e-5), epilogue=K.GV_SWIGLU)
    h = K.gemm_rows16(**kw)
    assert h.shape == (M, I)
    _close(h.float().cpu(), want, 0.02, "int8 swiglu")
    assert torch.equal(h, K.gemm_rows16(**kw))


@pytest.mark.parametrize("M", [2, 16])
@pytest.mark.parametrize("D", [512, 1024])
def test_rows16_i8_qkv_batched_rope_and_cache(K, cuda, M, D):
    """The q|k|v projection of a batched decode step on int8 rows: row m is sequence m at token index 0 of the call, so RoPE uses table
    row 0 on q and k; k / v go to cache[m] at pos[m] (distinct positions, 0 and Smax - 1 among them); every other element of every
    batch slot keeps its bits.  Bar: test_rows16_qkv_batched_rope_and_cache's."""
    H, KVH, hd, Smax, B = 4, 1, 128, 96, 16
    qs = [_qweight(f"r8_wq{D}", H * hd, D), _qweight(f"r8_wk{D}", KVH * hd, D), _qweight(f"r8_wv{D}", KVH * hd, D)]
    x = O.randn(f"r8_qx{D}", (16, D), 1.0).to(BF)[:M]
    nw = (1 + O.randn(f"r8_qn{D}", (D,), 0.1)).to(BF)
    table = O.rope_table(O.TINY._replace(max_seq_len=Smax))
    pos = torch.tensor([0, Smax - 1, 70, 3, 41, 95 - 7, 12, 13, 14, 50, 51, 52, 60, 61, 62, 63][:M])
    xb = O.rmsnorm(x, nw, 1e-5)
    q, k, v = (O.int8_linear(xb, wi, sc, dynamic=True).to(BF).view(M, 1, -1, hd) for wi, sc in qs)
    q, k = O.rope_apply(q, table), O.rope_apply(k, table)
    sentinel = torch.full((B, KVH, Smax, hd), -7.25, dtype=BF)
    outs = []
    for _ in range(2):
        kc_d, vc_d = sentinel.to(cuda), sentinel.to(cuda)
        got = K.gemm_rows16(x=x.to(cuda), norm=(nw.to(cuda), 1e-5), epilogue=K.GV_QKV, qkv=(table.to(cuda), H * hd, KVH * hd, kc_d, vc_d, pos.to(cuda)),
                            **_dev(qs, cuda))
        outs.append((got, kc_d, vc_d))
    got, kc_d, vc_d = outs[0]
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1])), "repeat launch"
    assert got.shape == (M, H * hd)
    _close(got.float().cpu().view(M, 1, H, hd), q.float(), 0.01, "q with RoPE row 0")
    kc, vc = kc_d.cpu(), vc_d.cpu()
    written = torch.zeros(B, Smax, dtype=torch.bool)
    written[torch.arange(M), pos] = True
    for name, c, want in (("k", kc, k), ("v", vc, v)):
        _close(c[torch.arange(M), :, pos].float(), want[:, 0].float(), 0.01, f"{name} cache rows")
        untouched = c.transpose(1, 2)[~written]
        assert torch.equal(untouched, torch.full_like(untouched, -7.25)), f"{name} cache: an element outside (m, pos[m]) changed"


def test_rows16_i8_rejects(K, cuda):
    from llx._lib import LlxError

    wi, sc = _qweight("r8_w_rej", 64, 1040)
    wb = O.randn("r8_wb_rej", (64, 1040), 0.05).to(BF)
    x = O.randn("r8_x_rej", (17, 1040), 1.0).to(BF).to(cuda)
    with pytest.raises(LlxError, match="one kind"):
        K.gemm_rows16([wb.to(cuda), wi.to(cuda)], x[:2], wscale=[sc.to(cuda), sc.to(cuda)])
    with pytest.raises(LlxError, match="multiple of 16"):
        K.gemm_rows16([wi[:, :1032].contiguous().to(cuda)], x[:2, :1032].contiguous(), wscale=[sc.to(cuda)])
    with pytest.raises(LlxError, match="outside 2..16"):
        K.gemm_rows16([wi.to(cuda)], x, wscale=[sc.to(cuda)])
