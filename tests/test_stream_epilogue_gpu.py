"""GPU: the two weight streams of the decode step are the same function.  llx_gemv_bf16 (csrc/decode.hip) and llx_gemm_rows16_bf16
(csrc/decode_rows.hip) share one epilogue (csrc/wstream.h), so row m of gemm_rows16(ws, x[:M]) must equal gemv(ws, x[m:m+1]) bit for bit
wherever the values that enter the epilogue are equal.

They are equal here by construction: weights and activations are integers in -2..2 and K <= 520, so every partial sum is an integer of
magnitude <= 4 K = 2080 < 2^24 - exact in fp32 in any summation order, whatever the kernels' orders are (the test checks this on the CPU:
an int64 product against the fp32 one).  No norm is fused (1 / rms is not an integer).  The library is built without floating-point
contraction, so the epilogue arithmetic on equal inputs gives equal bits.

Shapes: M = 3 rows; K = 256 is one K slice of the batched stream (its epilogue runs in the main kernel), K = 520 is three slices with a
ragged last batch (it runs in the combine launch); N = 36 leaves a partly filled tile and a ragged row group; I = 20 hidden units leave
4 live units in the last SwiGLU tile."""
import pytest
import torch

from oracle import ref as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
M = 3
KS = [256, 520]


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


def _ints(seed, shape, amp):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-amp, amp + 1, shape, generator=g, dtype=torch.int64)


def _operands(K_, ns, seed):
    """Integer weights [n_s, K] and activations [M, K] as bf16, after the check that their products are exact in fp32."""
    ws = [_ints(seed + 1 + i, (n, K_), 2) for i, n in enumerate(ns)]
    x = _ints(seed, (M, K_), 2)
    exact = x @ torch.cat(ws).T
    assert int(exact.abs().max()) <= 4 * K_ <= 2080
    assert torch.equal((x.float() @ torch.cat(ws).float().T).to(torch.int64), exact), "the fp32 product of the test's operands is not exact"
    return [w.to(BF) for w in ws], x.to(BF), exact


@pytest.mark.parametrize("K_", KS)
def test_plain_and_residual_rows_equal_the_gemv(K, cuda, K_):
    ws, x, exact = _operands(K_, (36,), 100)
    res = _ints(7, (M, 36), 8).to(BF)
    wd, xd, rd = [w.to(cuda) for w in ws], x.to(cuda), res.to(cuda)
    got = K.gemm_rows16(wd, xd)
    got_r = K.gemm_rows16(wd, xd, epilogue=K.GV_RESIDUAL, res=rd)
    assert torch.equal(got.cpu(), exact.float().to(BF)), "the batched stream's plain output is not the bf16 rounding of the exact product"
    for m in range(M):
        assert torch.equal(got[m : m + 1], K.gemv(wd, xd[m : m + 1])), f"plain: row {m}"
        assert torch.equal(got_r[m : m + 1], K.gemv(wd, xd[m : m + 1], epilogue=K.GV_RESIDUAL, res=rd[m : m + 1])), f"+ residual: row {m}"


@pytest.mark.parametrize("K_", KS)
def test_swiglu_rows_equal_the_gemv(K, cuda, K_):
    ws, x, _ = _operands(K_, (20, 20), 200)
    wd, xd = [w.to(cuda) for w in ws], x.to(cuda)
    got = K.gemm_rows16(wd, xd, epilogue=K.GV_SWIGLU)
    assert got.shape == (M, 20) and bool((got != 0).any())
    for m in range(M):
        assert torch.equal(got[m : m + 1], K.gemv(wd, xd[m : m + 1], epilogue=K.GV_SWIGLU)), f"SwiGLU: row {m}"


@pytest.mark.parametrize("K_", KS)
def test_qkv_rows_and_caches_equal_the_gemv(K, cuda, K_):
    """q|k|v with segments (256, 128, 128) and caches of 4 slots x Smax = 8: the batched stream rotates every row by table row 0 and
    writes row m to cache[m] at pos[m]; the gemv does the same for row m when it is given that table row, the slot cache[m:m+1] and
    pos[m].  The table row is that of position 5, so that the rotation is not the identity.  q and the whole caches - written and
    untouched elements alike - must be equal."""
    Smax, B, n_q, n_k = 8, 4, 256, 128
    ws, x, _ = _operands(K_, (n_q, n_k, 128), 300)
    wd, xd = [w.to(cuda) for w in ws], x.to(cuda)
    row = O.rope_table(O.TINY._replace(max_seq_len=Smax))[5:6].contiguous().to(cuda)  # [1, 64, 2]
    pos = torch.tensor([0, Smax - 1, 3], device=cuda)
    sentinel = torch.full((B, 1, Smax, 128), -7.25, dtype=BF, device=cuda)
    kb, vb, kg, vg = (sentinel.clone() for _ in range(4))
    q = K.gemm_rows16(wd, xd, epilogue=K.GV_QKV, qkv=(row, n_q, n_k, kb, vb, pos))
    for m in range(M):
        qm = K.gemv(wd, xd[m : m + 1], epilogue=K.GV_QKV, qkv=(row, n_q, n_k, kg[m : m + 1], vg[m : m + 1], pos[m : m + 1]))
        assert torch.equal(q[m : m + 1], qm), f"q: row {m}"
    assert torch.equal(kb, kg) and torch.equal(vb, vg)
    # and the writes happened: exactly the rows (m, pos[m]) differ from the sentinel
    written = torch.zeros(B, Smax, dtype=torch.bool, device=cuda)
    written[torch.arange(M, device=cuda), pos] = True
    for c in (kb, vb):
        assert torch.equal((c[:, 0] != -7.25).any(dim=-1), written)
