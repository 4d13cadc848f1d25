"""GPU: the GEMM main loop gives the same bits on every launch, at the training step's shapes.

The loop reads its fragments from LDS with hand-counted waits while the LDS-DMA of later K-tiles is in flight (gemm_bf16.hip); a read
that is not in before the barrier that releases its tile races the next fill of that stage.  Such a race does not fail every time:
it shows up as a rare mismatch between launches of the same problem.  So every shape of the step is launched REPEATS times and each
output must equal the first bit for bit; the first is also held against an fp32 restatement at the tolerance of
tests/test_kernels_gpu.py::test_gemm_nt (one bf16 ulp of the result magnitude), the fused epilogues against their stand-alone kernels
bit for bit as there."""
import pytest
import torch

pytestmark = pytest.mark.gpu

REPEATS = 20
M, D, I, QKV = 4096, 4096, 14336, 6144  # Llama-3.1-8B at T = 4096 tokens: hidden, MLP, q|k|v width


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


@pytest.fixture(scope="module")
def rn(cuda):
    g = torch.Generator(device=cuda)
    g.manual_seed(1234)
    return lambda *s, scale=1.0: (torch.randn(*s, device=cuda, generator=g) * scale).bfloat16()


def _repeat(run):
    """run() -> tuple of output tensors; launched REPEATS times, every output equal to the first launch's.  Returns the first."""
    first = tuple(t.clone() for t in run())
    for i in range(1, REPEATS):
        again = run()
        torch.cuda.synchronize()
        for j, (x, y) in enumerate(zip(first, again)):
            assert torch.equal(x, y), f"launch {i}, output {j}: {(x != y).sum().item()} elements differ from the first launch"
    return first


def _product(a, b, a2=None, b2=None):
    ref = a.float() @ b.float().T
    if a2 is not None:
        ref = ref + a2.float() @ b2.float().T
    return ref


def _close(c, ref):
    torch.testing.assert_close(c.float(), ref, atol=2 ** -7 * ref.abs().max().item(), rtol=2 ** -7)


@pytest.mark.parametrize("Kd", [D, I], ids=["wo", "w2"])
def test_residual(K, rn, Kd):
    """wo | w2 + residual: one round of 256 tiles, 64 | 224 K-tiles"""
    x, w, res = rn(M, Kd), rn(D, Kd, scale=0.05), rn(M, D)
    (c,) = _repeat(lambda: (K.gemm_nt(x, w, epilogue=K.EPI_RESIDUAL, e=res),))
    _close(c, _product(x, w).bfloat16().float() + res.float())


def test_w2_dgrad_swiglu_bwd(K, rn, cuda):
    """dh = dy . W2 with the SwiGLU backward in the epilogue: 896 tiles = 3 rounds of full tiles + a round of half tiles"""
    dy, wt, gu = rn(M, D), rn(I, D, scale=0.05), rn(M, 2 * I)
    out = torch.empty(M, 2 * I, device=cuda, dtype=torch.bfloat16)
    (dgu,) = _repeat(lambda: (K.gemm_nt(dy, wt, out=out, epilogue=K.EPI_SWIGLU_BWD, e=gu),))
    dh = K.gemm_nt(dy, wt)
    _close(dh, _product(dy, wt))
    ref = torch.empty_like(dgu)
    K.swiglu_bwd(dh, gu[:, :I], gu[:, I:], ref[:, :I], ref[:, I:])
    assert torch.equal(dgu, ref)


def test_qkv_rope_extension(K, rn, cuda):
    """q|k|v projection with the LoRA K-extension and RoPE in the epilogue (384 tiles: one round + a round of half tiles)"""
    B, S, heads = 2, M // 2, (QKV - 1024) // 128  # 32 q + 8 k heads rotated, 8 v heads not
    pos = torch.arange(S, device=cuda, dtype=torch.float32)[:, None] * (500000.0 ** (-torch.arange(64, device=cuda, dtype=torch.float32) / 64))[None, :]
    table = torch.stack([pos.cos(), pos.sin()], -1).contiguous()
    x, w, a2, b2 = rn(M, D), rn(QKV, D, scale=0.05), rn(M, 64), rn(QKV, 64, scale=0.05)
    out = torch.empty(M, QKV, device=cuda, dtype=torch.bfloat16)
    (c,) = _repeat(lambda: (K.gemm_nt(x, w, out=out, a2=a2, b2=b2, rope=(table, S, heads * 128)),))
    plain = K.gemm_nt(x, w, a2=a2, b2=b2)
    _close(plain, _product(x, w, a2, b2))
    K.rope_(plain.view(B, S, QKV), table, heads)
    assert torch.equal(c, plain)


def test_gate_up_swiglu_fwd_extension(K, rn, cuda):
    """gate|up projection with the LoRA K-extension and the SwiGLU forward in the epilogue (7 rounds)"""
    x, w, a2, b2 = rn(M, D), rn(2 * I, D, scale=0.05), rn(M, 64), rn(2 * I, 64, scale=0.05)
    gu = torch.empty(M, 2 * I, device=cuda, dtype=torch.bfloat16)
    h = torch.empty(M, I, device=cuda, dtype=torch.bfloat16)

    def run():
        K.gemm_nt(x, w, out=gu, a2=a2, b2=b2, epilogue=K.EPI_SWIGLU_FWD, e=h)
        return gu, h

    gu0, h0 = _repeat(run)
    _close(gu0, _product(x, w, a2, b2))
    assert torch.equal(h0, K.swiglu_fwd(gu0[:, :I], gu0[:, I:]))


def test_int8_extension(K, rn, cuda):
    """int8 q|k|v with dynamic activation scales and the LoRA K-extension (int8 K-tiles, in-place dequantisation, bf16 K-tiles)"""
    from subclasses.int8_mm import _launch

    g = torch.Generator(device=cuda)
    g.manual_seed(99)
    a = torch.randint(-127, 128, (M, D), device=cuda, generator=g, dtype=torch.int8)
    b = torch.randint(-127, 128, (QKV, D), device=cuda, generator=g, dtype=torch.int8)
    sa = (torch.rand(M, device=cuda, generator=g) * 0.009 + 0.001).bfloat16()
    sb = (torch.rand(QKV, device=cuda, generator=g) * 0.009 + 0.001).bfloat16()
    a2, b2 = rn(M, 64), rn(QKV, 64, scale=0.05)
    (c,) = _repeat(lambda: (_launch(a, b, sa, sb, a2=a2, b2=b2),))
    exact = (a.double() @ b.double().T).float()  # |sum| < 2^53: the integer product, rounded to fp32 as the kernel's int32 -> float
    ref = ((exact * sa.float()[:, None]) * sb.float()[None, :]).bfloat16().float() + a2.float() @ b2.float().T
    _close(c, ref)


def test_half_tile_split(K, rn):
    """plain 4096 x 6144 x 4096: 256 full tiles and 256 half tiles (256 x 128) in two launches"""
    x, w = rn(M, D), rn(QKV, D, scale=0.05)
    (c,) = _repeat(lambda: (K.gemm_nt(x, w),))
    _close(c, _product(x, w))
