"""GPU: the batched decode kernels (csrc/decode_rows.hip, the batch form of the cache scatter in csrc/decode.hip) - the weight-streaming
MFMA product for 2..16 activation rows with its prologue and epilogues, against fp32 references on the bf16-rounded operands.
Bars: those of tests/test_decode_gpu.py for the same quantities (max error against the reference's max magnitude)."""
import pytest
import torch

from oracle import ref as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
_REF: dict = {}


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


def _close(a, b, rel, name):
    scale = b.abs().max().item()
    err = (a - b).abs().max().item()
    assert err <= rel * scale + 1e-6, f"{name}: max err {err:.4e} vs scale {scale:.4e} (allowed {rel * scale:.4e})"


def _operands(K_, ns):
    """Weights, 16 activation rows, norm weight and residual of one (K, segments) case, with the fp32 products of all 16 rows with and
    without the norm: computed once, shared by the M cases (row m of the product does not depend on M)."""
    key = (K_, ns)
    if key not in _REF:
        ws = [O.randn(f"r16_w{i}_{K_}_{n}", (n, K_), 0.05).to(BF) for i, n in enumerate(ns)]
        x = O.randn(f"r16_x_{K_}", (16, K_), 1.0).to(BF)
        nw = (1 + O.randn(f"r16_n{K_}", (K_,), 0.1)).to(BF)
        res = O.randn(f"r16_r_{sum(ns)}", (16, sum(ns)), 1.0).to(BF)
        wcat = torch.cat(ws).float().T
        _REF[key] = (ws, x, nw, res, {False: x.float() @ wcat, True: O.rmsnorm(x, nw, 1e-5).float() @ wcat})
    return _REF[key]


# (K, segments): with M they fix every dispatch decision of the launcher (rows16_plan in csrc/decode_rows.hip):
#   tiles    ceil(N / 16), the last one partly filled (N = 36: 3 tiles, 4 live rows in the last; 33000: 2063 tiles) or all full;
#   slices   S = 1, no hand-off between workgroups (K = 256); S = 3 with slices of 256, 256 and 8 elements - a last batch that runs
#            past K and a k-step with 8 of 32 live elements (K = 520); S = 8 / 16 equal slices (K = 4096 with 256 / 48 tiles); S = 56,
#            the floor of 256 elements per slice, one batch per wave item (K = 14336, N = 36); K = 14336 with N = 4096: S = 8 slices
#            of 1792 = 7 batches per item, so the two register sets swap inside an item and across items; S = 2 in the SwiGLU test;
#   tiles per wave: 1 (ntiles * S <= 2048: N = 4096 with K = 4096 / 14336 is exactly 2048) or 2 (N = 33000, K = 256);
#   LDS cap  at M = 16 a slice is at most 1792 elements (the image of 16 rows within 60 KiB), at M = 2 whole rows fit.  It decides S
#            only where the tiles alone would ask for fewer slices: test_rows16_lds_cap_decides_the_split below (the 8B gate|up and
#            head products at M = 16 are of that kind).
CASES = [(256, (36,)), (256, (33000,)), (520, (36,)), (4096, (512, 128, 128)), (4096, (4096,)), (14336, (36,)), (14336, (4096,))]


@pytest.mark.parametrize("K_,ns", CASES)
@pytest.mark.parametrize("M", [2, 5, 16])
@pytest.mark.parametrize("norm", [False, True])
def test_rows16_plain_and_residual(K, cuda, M, K_, ns, norm):
    """out = [rmsnorm(x) | x] @ [W0; W1; W2]^T (+ residual) for two rows, a partly filled operand and a full one; a second launch is
    bit-identical (the K slices are summed in slice order, no atomics on floats)."""
    ws, x, nw, res, want16 = _operands(K_, ns)
    want = want16[norm][:M]
    wd, xd = [w.to(cuda) for w in ws], x[:M].to(cuda)
    nd = (nw.to(cuda), 1e-5) if norm else None
    got = K.gemm_rows16(wd, xd, norm=nd)
    assert got.shape == want.shape and got.dtype is BF
    _close(got.float().cpu(), want, 0.01, "rows16")
    got_r = K.gemm_rows16(wd, xd, norm=nd, epilogue=K.GV_RESIDUAL, res=res[:M].to(cuda))
    _close(got_r.float().cpu(), want.to(BF).float() + res[:M].float(), 0.01, "rows16 + residual")
    assert torch.equal(got, K.gemm_rows16(wd, xd, norm=nd))
    assert torch.equal(got_r, K.gemm_rows16(wd, xd, norm=nd, epilogue=K.GV_RESIDUAL, res=res[:M].to(cuda)))


@pytest.mark.parametrize("M", [2, 16])
def test_rows16_lds_cap_decides_the_split(K, cuda, M):
    """K = 4096, N = 16400 (1025 full tiles): the tiles alone ask for 2 slices.  At M = 2 that
    is what runs (S = 2, slices of 2048); at M = 16 the LDS image of 16 rows allows slices of at most 1792 elements, so the cap asks
    for 3 and the launcher takes 4 equal slices of 1024 - the branch the 8B gate|up and head products take at M = 16."""
    ws, x, nw, res, want16 = _operands(4096, (16400,))
    wd = [ws[0].to(cuda)]
    for norm in (False, True):
        nd = (nw.to(cuda), 1e-5) if norm else None
        got = K.gemm_rows16(wd, x[:M].to(cuda), norm=nd)
        _close(got.float().cpu(), want16[norm][:M], 0.01, f"rows16 norm={norm}")
        assert torch.equal(got, K.gemm_rows16(wd, x[:M].to(cuda), norm=nd))


@pytest.mark.parametrize("M", [2, 16])
@pytest.mark.parametrize("D,I", [(256, 1796), (512, 1796), (512, 14336)])
def test_rows16_swiglu(K, cuda, M, D, I):
    """gate|up with the SwiGLU epilogue (g, u and silu(g) rounded to bf16, then the product): a tile is the gate and up rows of 8 hidden
    units; I = 1796 leaves 4 live units in the last tile, I = 14336 is the 8B width (1792 tiles).  D = 256 is one K slice: the
    epilogue runs in the main kernel; D = 512 is split in two: it runs in the combine launch."""
    w1, w3 = (O.randn(f"r16_sw{i}_{I}_{D}", (I, D), 0.05).to(BF) for i in (1, 3))
    x = O.randn(f"r16_swx{D}", (16, D), 1.0).to(BF)[:M]
    nw = (1 + O.randn(f"r16_swn{D}", (D,), 0.1)).to(BF)
    xn = O.rmsnorm(x, nw, 1e-5).float()
    g, u = xn @ w1.float().T, xn @ w3.float().T
    want = torch.nn.functional.silu(g.to(BF).float()).to(BF).float() * u.to(BF).float()
    args = ([w1.to(cuda), w3.to(cuda)], x.to(cuda))
    h = K.gemm_rows16(*args, norm=(nw.to(cuda), 1e-5), epilogue=K.GV_SWIGLU)
    assert h.shape == (M, I)
    _close(h.float().cpu(), want, 0.02, "swiglu")
    assert torch.equal(h, K.gemm_rows16(*args, norm=(nw.to(cuda), 1e-5), epilogue=K.GV_SWIGLU))


@pytest.mark.parametrize("D", [256, 512])
@pytest.mark.parametrize("M", [2, 5, 16])
def test_rows16_qkv_batched_rope_and_cache(K, cuda, M, D):
    """The q|k|v projection of a batched decode step: row m is sequence m at token index 0 of the call, so RoPE uses table row 0 on q
    and k; k / v go to cache[m] at pos[m] (distinct positions, 0 and Smax - 1 among them); every other element of every batch slot
    keeps its bits.  The caches have 16 slots whatever M is: the slots past M must stay untouched too.  D = 256 is one K slice (the
    epilogue runs in the main kernel), D = 512 is split (it runs in the combine launch)."""
    H, KVH, hd, Smax, B = 4, 1, 128, 96, 16
    wq, wk, wv = O.randn(f"r16_wq{D}", (H * hd, D), 0.05).to(BF), O.randn(f"r16_wk{D}", (KVH * hd, D), 0.05).to(BF), O.randn(f"r16_wv{D}", (KVH * hd, D), 0.05).to(BF)
    x = O.randn(f"r16_qx{D}", (16, D), 1.0).to(BF)[:M]
    nw = (1 + O.randn(f"r16_qn{D}", (D,), 0.1)).to(BF)
    table = O.rope_table(O.TINY._replace(max_seq_len=Smax))
    pos = torch.tensor([0, Smax - 1, 70, 3, 41, 95 - 7, 12, 13, 14, 50, 51, 52, 60, 61, 62, 63][:M])
    xn = O.rmsnorm(x, nw, 1e-5).float()
    # every row is its own sequence of ONE token: [M, 1, heads, hd] through apply_rope takes table row 0 for each
    q = O.rope_apply((xn @ wq.float().T).to(BF).view(M, 1, H, hd), table)
    k = O.rope_apply((xn @ wk.float().T).to(BF).view(M, 1, KVH, hd), table)
    v = (xn @ wv.float().T).to(BF).view(M, 1, KVH, hd)
    sentinel = torch.full((B, KVH, Smax, hd), -7.25, dtype=BF)
    kc_d, vc_d = sentinel.to(cuda), sentinel.to(cuda)
    got = K.gemm_rows16([wq.to(cuda), wk.to(cuda), wv.to(cuda)], x.to(cuda), norm=(nw.to(cuda), 1e-5), epilogue=K.GV_QKV,
                        qkv=(table.to(cuda), H * hd, KVH * hd, kc_d, vc_d, pos.to(cuda)))
    assert got.shape == (M, H * hd)
    _close(got.float().cpu().view(M, 1, H, hd), q.float(), 0.01, "q with RoPE row 0")
    kc, vc = kc_d.cpu(), vc_d.cpu()
    written = torch.zeros(B, Smax, dtype=torch.bool)
    written[torch.arange(M), pos] = True
    for name, c, want in (("k", kc, k), ("v", vc, v)):
        rows = c[torch.arange(M), :, pos]  # [M, KVH, hd]
        _close(rows.float(), want[:, 0].float(), 0.01, f"{name} cache rows")
        untouched = c.transpose(1, 2)[~written]  # [B * Smax - M, KVH, hd]
        assert torch.equal(untouched, torch.full_like(untouched, -7.25)), f"{name} cache: an element outside (m, pos[m]) changed"


def test_kv_scatter_with_a_position_row_per_sequence(K, cuda):
    """KVCache.update with input_pos [B, L]: cache[b, :, input_pos[b, l]] = src[b, :, l] bit for bit from strided views of a fused q|k|v
    buffer, everything else untouched."""
    B, L_, H, KVH, hd, Smax = 3, 5, 4, 2, 128, 96
    qkv = O.randn("r16_sc_qkv", (B, L_, (H + 2 * KVH) * hd), 1.0).to(BF).to(cuda)
    k5 = qkv[..., H * hd : (H + KVH) * hd].unflatten(-1, (KVH, hd)).transpose(1, 2)
    v5 = qkv[..., (H + KVH) * hd :].unflatten(-1, (KVH, hd)).transpose(1, 2)
    pos = torch.tensor([[9, 0, 33, 95, 50], [0, 1, 2, 3, 4], [95, 94, 10, 9, 77]])
    kc = O.randn("r16_sc_kc", (B, KVH, Smax, hd), 1.0).to(BF)
    vc = O.randn("r16_sc_vc", (B, KVH, Smax, hd), 1.0).to(BF)
    kc_d, vc_d = kc.to(cuda), vc.to(cuda)
    K.kv_scatter(k5, v5, kc_d, vc_d, pos.to(cuda))
    kr, vr = kc.clone(), vc.clone()
    for b in range(B):
        kr[b, :, pos[b]] = k5[b].cpu()
        vr[b, :, pos[b]] = v5[b].cpu()
    assert torch.equal(kc_d.cpu(), kr) and torch.equal(vc_d.cpu(), vr)


def test_rows16_rejects(K, cuda):
    from llx._lib import LlxError

    w = O.randn("r16_w_rej", (64, 256), 0.05).to(BF).to(cuda)
    for M in (1, 17):
        with pytest.raises(LlxError, match="outside 2..16"):
            K.gemm_rows16([w], torch.zeros(M, 256, dtype=BF, device=cuda))
    with pytest.raises(LlxError, match="multiple of 8"):
        K.gemm_rows16([w[:, :100].contiguous()], torch.zeros(2, 100, dtype=BF, device=cuda))
