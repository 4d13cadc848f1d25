"""GPU: the adapter term of the batched weight stream (csrc/decode_rows.hip: rows16_adapter, llx_gemm_rows16_bf16_lora /
llx_gemm_rows16_i8_lora) against the GEMV's (csrc/decode.hip), bit for bit, in the manner of tests/test_stream_epilogue_gpu.py.

Weights, activations, B factors and t are integers in -2..2 and lora_scale is 0.5 or 2: |base| <= 4 K <= 2080 and
|scale * t . B| <= 2 * 4 * 64 = 512, every value is a multiple of 0.5 far below 2^24, so every fp32 sum is exact in any summation
order - the GEMV's lane-wise FMA chains and butterfly, the MFMA chain here - and the values that enter the shared epilogue are equal.
The test checks the exactness on the CPU (int64 against fp32) before it relies on it.  t is handed to both streams as data (it need
not be x @ A^T for this comparison).  No norm is fused.

Shapes: K = 256 is one K slice (the adapter term is computed in the main kernel's finish), K = 520 three slices with a ragged last
batch (in the combine launch); N = 36 leaves 4 live rows in the last tile.  The B factors and t are views of NaN-filled buffers
(rows behind the factor, rows >= M and columns >= sum r of t): a lane that should hold zeros and loads instead - a rank chunk past
the row's ranks, a column m >= M - puts a NaN into a stored output.  Ranks 16 (half an MFMA K chunk), 48 (one and a half); q|k|v with
ranks (16, 32, 16), SwiGLU with gate / up ranks (16, 32) at I = 20 hidden units."""
import pytest
import torch

from oracle import ref as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
KS = [256, 520]


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


def _ints(seed, shape, amp=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-amp, amp + 1, shape, generator=g, dtype=torch.int64)


def _operands(K_, ns, ranks, seed, M=3):
    """Integer weights [n_s, K], activations [M, K], B factors [n_s, r_s] and t [M, sum r] (int64), after the check that the base
    product and the adapter term are exact in fp32."""
    ws = [_ints(seed + 1 + i, (n, K_)) for i, n in enumerate(ns)]
    bs = [_ints(seed + 11 + i, (n, r)) for i, (n, r) in enumerate(zip(ns, ranks))]
    x, t = _ints(seed, (M, K_)), _ints(seed + 21, (M, sum(ranks)))
    base = x @ torch.cat(ws).T
    offs = [sum(ranks[:i]) for i in range(len(ranks))]
    lora = torch.cat([t[:, o : o + r] @ b.T for o, r, b in zip(offs, ranks, bs)], 1)
    assert int(base.abs().max()) <= 4 * K_ <= 2080 and int(lora.abs().max()) <= 4 * 64
    assert torch.equal((x.float() @ torch.cat(ws).float().T).to(torch.int64), base), "the fp32 base product of the test's operands is not exact"
    for o, r, b in zip(offs, ranks, bs):
        assert torch.equal((t[:, o : o + r].float() @ b.float().T).to(torch.int64), t[:, o : o + r] @ b.T), "the fp32 adapter term is not exact"
    return ws, x, bs, t, base, lora


def _factors(bs, cuda):
    """The B factors on the device, each the head of a buffer whose remaining rows are NaN."""
    out = []
    for b in bs:
        buf = torch.full((b.shape[0] + 16, b.shape[1]), float("nan"), dtype=BF, device=cuda)
        buf[: b.shape[0]] = b.to(BF)
        out.append(buf[: b.shape[0]])
    return out


def _tdev(t, cuda):
    """t on the device as the corner of a [16, sum r + 64] buffer of NaN (row stride sum r + 64)."""
    buf = torch.full((16, t.shape[1] + 64), float("nan"), dtype=BF, device=cuda)
    buf[: t.shape[0], : t.shape[1]] = t.to(BF)
    return buf[: t.shape[0], : t.shape[1]]


def _dev(ts, cuda):
    return [t.to(BF).to(cuda) for t in ts]


@pytest.mark.parametrize("K_,rank,scale,M", [(256, 16, 0.5, 3), (256, 48, 2.0, 3), (520, 16, 2.0, 3), (520, 48, 0.5, 3), (520, 48, 2.0, 2), (256, 16, 2.0, 16),
                                             (520, 32, 0.5, 16), (256, 64, 0.5, 3)])
def test_plain_and_residual_rows_equal_the_gemv(K, cuda, K_, rank, scale, M):
    ws, x, bs, t, base, lora = _operands(K_, (36,), (rank,), 100 + rank, M)
    res = _ints(7, (M, 36), 8).to(BF).to(cuda)
    wd, xd, td, bd = _dev(ws, cuda), x.to(BF).to(cuda), _tdev(t, cuda), _factors(bs, cuda)
    got = K.gemm_rows16(wd, xd, lora=(bd, td, scale))
    got_r = K.gemm_rows16(wd, xd, epilogue=K.GV_RESIDUAL, res=res, lora=(bd, td, scale))
    want = (base.double() + scale * lora.double()).float()  # exact: multiples of 0.5 below 2^24
    assert torch.equal(got.cpu(), want.to(BF)), "the batched stream's output is not bf16(exact base + scale * t B^T)"
    assert not torch.equal(got, K.gemm_rows16(wd, xd)), "the adapter term is zero"
    for m in range(M):
        lo = (bd, td[m : m + 1], scale)
        assert torch.equal(got[m : m + 1], K.gemv(wd, xd[m : m + 1], lora=lo)), f"plain: row {m}"
        assert torch.equal(got_r[m : m + 1], K.gemv(wd, xd[m : m + 1], epilogue=K.GV_RESIDUAL, res=res[m : m + 1], lora=lo)), f"+ residual: row {m}"


@pytest.mark.parametrize("K_", KS)
@pytest.mark.parametrize("scale", [0.5, 2.0])
def test_swiglu_rows_equal_the_gemv(K, cuda, K_, scale):
    M = 3
    ws, x, bs, t, _, _ = _operands(K_, (20, 20), (16, 32), 200)
    wd, xd, td, bd = _dev(ws, cuda), x.to(BF).to(cuda), _tdev(t, cuda), _factors(bs, cuda)
    got = K.gemm_rows16(wd, xd, epilogue=K.GV_SWIGLU, lora=(bd, td, scale))
    assert got.shape == (M, 20) and bool((got != 0).any()) and bool(torch.isfinite(got.float()).all())
    assert not torch.equal(got, K.gemm_rows16(wd, xd, epilogue=K.GV_SWIGLU))
    for m in range(M):
        assert torch.equal(got[m : m + 1], K.gemv(wd, xd[m : m + 1], epilogue=K.GV_SWIGLU, lora=(bd, td[m : m + 1], scale))), f"SwiGLU: row {m}"
    # the gate and up ranks the other way round: the up part of the chain starts inside the first MFMA chunk or behind it
    ws2, x2, bs2, t2, _, _ = _operands(K_, (20, 20), (32, 16), 250)
    wd, xd, td, bd = _dev(ws2, cuda), x2.to(BF).to(cuda), _tdev(t2, cuda), _factors(bs2, cuda)
    got = K.gemm_rows16(wd, xd, epilogue=K.GV_SWIGLU, lora=(bd, td, scale))
    for m in range(M):
        assert torch.equal(got[m : m + 1], K.gemv(wd, xd[m : m + 1], epilogue=K.GV_SWIGLU, lora=(bd, td[m : m + 1], scale))), f"SwiGLU (32, 16): row {m}"


def _qkv_case(K, cuda, K_, kw_of, ws, x, bs, t, scale, M=3):
    """q|k|v with segments (256, 128, 128) through both streams (kw_of(m): the further keyword arguments for rows m, or all rows for
    None): q, the whole caches and the untouched sentinel rows must be equal."""
    Smax, B, n_q, n_k = 8, 4, 256, 128
    wd, xd, td, bd = ws, x.to(BF).to(cuda), _tdev(t, cuda), _factors(bs, cuda)
    row = O.rope_table(O.TINY._replace(max_seq_len=Smax))[5:6].contiguous().to(cuda)  # [1, 64, 2]: position 5, not the identity
    pos = torch.tensor([0, Smax - 1, 3], device=cuda)
    sentinel = torch.full((B, 1, Smax, 128), -7.25, dtype=BF, device=cuda)
    kb, vb, kg, vg = (sentinel.clone() for _ in range(4))
    q = K.gemm_rows16(wd, xd, epilogue=K.GV_QKV, qkv=(row, n_q, n_k, kb, vb, pos), lora=(bd, td, scale), **kw_of(None))
    for m in range(M):
        qm = K.gemv(wd, xd[m : m + 1], epilogue=K.GV_QKV, qkv=(row, n_q, n_k, kg[m : m + 1], vg[m : m + 1], pos[m : m + 1]),
                    lora=(bd, td[m : m + 1], scale), **kw_of(m))
        assert torch.equal(q[m : m + 1], qm), f"q: row {m}"
    assert torch.equal(kb, kg) and torch.equal(vb, vg)
    written = torch.zeros(B, Smax, dtype=torch.bool, device=cuda)
    written[torch.arange(M, device=cuda), pos] = True
    for c in (kb, vb):
        assert torch.equal((c[:, 0] != -7.25).any(dim=-1), written)
    return q, kb, vb


@pytest.mark.parametrize("K_", KS)
def test_qkv_rows_and_caches_equal_the_gemv(K, cuda, K_):
    ws, x, bs, t, _, _ = _operands(K_, (256, 128, 128), (16, 32, 16), 300)
    wd = _dev(ws, cuda)
    q, kb, vb = _qkv_case(K, cuda, K_, lambda m: {}, wd, x, bs, t, 2.0)
    # and the adapters reached every segment
    sentinel = torch.full_like(kb, -7.25)
    k0, v0 = sentinel.clone(), sentinel.clone()
    row = O.rope_table(O.TINY._replace(max_seq_len=8))[5:6].contiguous().to(cuda)
    q0 = K.gemm_rows16(wd, x.to(BF).to(cuda), epilogue=K.GV_QKV, qkv=(row, 256, 128, k0, v0, torch.tensor([0, 7, 3], device=cuda)))
    assert not torch.equal(q, q0) and not torch.equal(kb, k0) and not torch.equal(vb, v0)


@pytest.mark.parametrize("K_", KS)
def test_dora_rows_equal_the_gemv(K, cuda, K_):
    """colscale random bf16 in 0.5 .. 1.5: the factor multiplies the rounded sum, one rounding more, in both streams."""
    M, scale = 3, 0.5
    g = torch.Generator().manual_seed(5)
    ws, x, bs, t, base, lora = _operands(K_, (36,), (48,), 400)
    cs = [(0.5 + torch.rand(36, generator=g)).to(BF).to(cuda)]
    wd, xd, td, bd = _dev(ws, cuda), x.to(BF).to(cuda), _tdev(t, cuda), _factors(bs, cuda)
    got = K.gemm_rows16(wd, xd, lora=(bd, td, scale), colscale=cs)
    want = ((base.double() + scale * lora.double()).float().to(BF).float() * cs[0].float().cpu()).to(BF)
    assert torch.equal(got.cpu(), want), "DoRA: not bf16(bf16(exact base + scale * t B^T) * c)"
    for m in range(M):
        assert torch.equal(got[m : m + 1], K.gemv(wd, xd[m : m + 1], lora=(bd, td[m : m + 1], scale), colscale=cs)), f"DoRA plain: row {m}"
    # SwiGLU and q|k|v take the factors of their own segments
    ws, x, bs, t, _, _ = _operands(K_, (20, 20), (16, 32), 410)
    cs = [(0.5 + torch.rand(20, generator=g)).to(BF).to(cuda) for _ in range(2)]
    wd, xd, td, bd = _dev(ws, cuda), x.to(BF).to(cuda), _tdev(t, cuda), _factors(bs, cuda)
    got = K.gemm_rows16(wd, xd, epilogue=K.GV_SWIGLU, lora=(bd, td, scale), colscale=cs)
    for m in range(M):
        assert torch.equal(got[m : m + 1], K.gemv(wd, xd[m : m + 1], epilogue=K.GV_SWIGLU, lora=(bd, td[m : m + 1], scale), colscale=cs)), f"DoRA SwiGLU: row {m}"
    ws, x, bs, t, _, _ = _operands(K_, (256, 128, 128), (16, 32, 16), 420)
    cs = [(0.5 + torch.rand(n, generator=g)).to(BF).to(cuda) for n in (256, 128, 128)]
    _qkv_case(K, cuda, K_, lambda m: dict(colscale=cs), _dev(ws, cuda), x, bs, t, 2.0)


@pytest.mark.parametrize("K_", [256, 1040])
def test_dynamic_int8_rows_equal_the_gemv(K, cuda, K_):
    """Dynamic int8 weights: the rows of x are quantised on chip (absmax 2 -> scale 2 / 127, the same in both streams), the int32 sums
    are exact, and the adapter term meets the dequantised bf16 base.  K = 256 is one slice of 512-element batches, 1040 three (520 is no multiple of 16)."""
    M, scale = 3, 2.0
    g = torch.Generator().manual_seed(9)
    ns, ranks = (36,), (48,)
    ws = [torch.randint(-127, 128, (n, K_), generator=g, dtype=torch.int8) for n in ns]
    sc = [(0.01 + 0.02 * torch.rand(n, generator=g)).to(BF).to(cuda) for n in ns]
    _, x, bs, t, _, _ = _operands(min(K_, 520), ns, ranks, 500)
    x = _ints(501, (M, K_))
    wd, xd, td, bd = [w.to(cuda) for w in ws], x.to(BF).to(cuda), _tdev(t, cuda), _factors(bs, cuda)
    res = _ints(7, (M, 36), 8).to(BF).to(cuda)
    got = K.gemm_rows16(wd, xd, wscale=sc, lora=(bd, td, scale))
    got_r = K.gemm_rows16(wd, xd, wscale=sc, lora=(bd, td, scale), epilogue=K.GV_RESIDUAL, res=res)
    assert not torch.equal(got, K.gemm_rows16(wd, xd, wscale=sc))
    for m in range(M):
        lo = (bd, td[m : m + 1], scale)
        assert torch.equal(got[m : m + 1], K.gemv(wd, xd[m : m + 1], wscale=sc, dynamic=True, lora=lo)), f"int8 plain: row {m}"
        assert torch.equal(got_r[m : m + 1], K.gemv(wd, xd[m : m + 1], wscale=sc, dynamic=True, lora=lo, epilogue=K.GV_RESIDUAL, res=res[m : m + 1])), f"int8 + residual: row {m}"
    # SwiGLU and q|k|v on int8 rows
    ws = [torch.randint(-127, 128, (20, K_), generator=g, dtype=torch.int8).to(cuda) for _ in range(2)]
    sc = [(0.002 + 0.002 * torch.rand(20, generator=g)).to(BF).to(cuda) for _ in range(2)]
    _, _, bs, t, _, _ = _operands(256, (20, 20), (16, 32), 510)
    td, bd = _tdev(t, cuda), _factors(bs, cuda)
    got = K.gemm_rows16(ws, xd, wscale=sc, epilogue=K.GV_SWIGLU, lora=(bd, td, 0.5))
    for m in range(M):
        assert torch.equal(got[m : m + 1], K.gemv(ws, xd[m : m + 1], wscale=sc, dynamic=True, epilogue=K.GV_SWIGLU, lora=(bd, td[m : m + 1], 0.5))), f"int8 SwiGLU: row {m}"
    ns = (256, 128, 128)
    ws = [torch.randint(-127, 128, (n, K_), generator=g, dtype=torch.int8).to(cuda) for n in ns]
    sc = [(0.01 + 0.02 * torch.rand(n, generator=g)).to(BF).to(cuda) for n in ns]
    _, _, bs, t, _, _ = _operands(256, ns, (16, 32, 16), 520)
    _qkv_case(K, cuda, K_, lambda m: dict(wscale=sc) if m is None else dict(wscale=sc, dynamic=True), ws, x, bs, t, 2.0)


def test_wrapper_rejections(K, cuda):
    from llx._lib import LlxError

    ws, x, bs, t, _, _ = _operands(256, (36,), (16,), 600)
    wd, xd, td, bd = _dev(ws, cuda), x.to(BF).to(cuda), _tdev(t, cuda), _factors(bs, cuda)
    with pytest.raises(LlxError, match="llx_gemm_rows16_bf16_lora"):  # rank 8: the batch-1 stream's rank
        K.gemm_rows16(wd, xd, lora=([bd[0][:, :8].contiguous()], td[:, :8], 2.0))
    with pytest.raises(LlxError):  # DoRA factors without adapter operands
        K.gemm_rows16(wd, xd, colscale=[torch.ones(36, dtype=BF, device=cuda)])
    with pytest.raises(LlxError):  # a float32 factor
        K.gemm_rows16(wd, xd, lora=(bd, td, 2.0), colscale=[torch.ones(36, dtype=torch.float32, device=cuda)])
    with pytest.raises(LlxError):  # DoRA on int8 rows
        K.gemm_rows16([torch.zeros(36, 256, dtype=torch.int8, device=cuda)], xd, wscale=[torch.ones(36, dtype=BF, device=cuda)], lora=(bd, td, 2.0),
                      colscale=[torch.ones(36, dtype=BF, device=cuda)])
