"""CPU self-test of tests/gemm_cases.py: the operands make every accumulation exact, the expected results exercise the rounding points
(enough outputs that need rounding, enough exact ties), every planted fault changes at least one expected bit where its class is live,
the launcher restatement agrees with llx.kernels.gemm_kernel_launches, and the table covers every dispatch class by the restatement."""
import pytest
import torch

from tests import gemm_cases as G

NT_IDS = [c.id for c in G.CASES]
TN_IDS = [c.id for c in G.TN_CASES]


def _shares(x: torch.Tensor):
    """(share of values bf16 cannot hold, share that lie exactly between two bf16 neighbours) of exact float64 values."""
    f = x.float()
    assert torch.equal(f.double(), x)
    inexact = f.bfloat16().double() != x
    tie = (f.contiguous().view(torch.int32) & 0xFFFF) == 0x8000   # the 16 bits bf16 drops are exactly one half of its last place
    return inexact.float().mean().item(), tie.float().mean().item()


def _contraction(c):
    return c.m_eff if isinstance(c, G.TnCase) else c.K + c.K2


def _check_data(c):
    assert G.bound(c) < 2 ** 24, (c.id, G.bound(c))
    grid = isinstance(c, G.TnCase) or c.kind in ("bf16", "splitk") or c.ext   # values on a grid of quanta (not: arbitrary int8 scales)
    if _contraction(c) >= 64 and not (isinstance(c, G.Case) and c.kind == "i8f32"):
        # shorter contractions (TN with under 64 token rows) keep most sums within the 256 integers bf16 holds: no share is asked of them
        inexact, ties = _shares(G.first_rounding(c))
        assert inexact >= 0.20, (c.id, inexact)
        if grid:
            assert ties >= 0.05, (c.id, ties)


@pytest.mark.parametrize("cid", NT_IDS)
def test_nt_case_is_exact_and_discriminating(cid):
    c = G.BY_ID[cid]
    _check_data(c)
    if c.m_valid == 0:
        return
    ref = G.expected(c)
    assert set(ref) >= {"out"} and ref["out"].shape == (c.M, c.N)
    for m in G.MUTANTS:
        if G.live(c, m):
            mut = G.expected(c, m)
            key = "z" if c.epi == "gelu" else "out"
            a, b = ref[key], mut[key]
            same = torch.equal(a.view(torch.int16), b.view(torch.int16)) if a.dtype is G.BF16 else torch.equal(a, b)
            assert not same, f"{cid}: the planted fault {m} leaves every expected bit as it is"


@pytest.mark.parametrize("cid", TN_IDS)
def test_tn_case_is_exact_and_discriminating(cid):
    c = G.BY_ID[cid]
    _check_data(c)
    ref = G.tn_expected(c)
    assert ref.shape == (c.N1, c.N2)
    if c.m_eff == 0:
        assert torch.equal(ref.view(torch.int16), torch.zeros(c.N1, c.N2, dtype=torch.int16))   # +0, not -0
    for m in G.MUTANTS:
        if G.live(c, m) and not (m in ("trunc", "away") and c.m_eff < 8):
            assert not torch.equal(ref, G.tn_expected(c, m)), f"{cid}: the planted fault {m} changes nothing"


def test_every_planted_fault_is_live_somewhere():
    for m in G.MUTANTS:
        assert any(G.live(c, m) for c in G.CASES), m


def test_launcher_restatement_agrees_with_the_package():
    from llx import kernels as K

    for c in G.CASES:
        gm, gn, nk1, nxt, split, tail_cols = G.dispatch(c)
        if c.kind != "splitk":
            assert K.gemm_kernel_launches(c.M, c.N, G.EPI_CODE[c.epi]) == (2 if split else 1), c.id
        assert nk1 >= 1 and nk1 * c.tk * c.splits == c.K and nxt * 64 == c.K2
        assert (tail_cols > 0) == split and tail_cols % 256 == 0 and tail_cols < c.N
    # the shapes the issue names, by hand: tail 1 / 128 split, 129 does not, a tail that is no multiple of grid_m does not, ragged N does not
    by = {(c.M, c.N): G.dispatch(c) for c in G.CASES if c.cls == "tail"}
    assert by[(129, 65792)][4:] == (True, 256) and by[(17, 98304)][4:] == (True, 128 * 256) and by[(300, 33024)][4:] == (True, 256)
    assert not by[(17, 98560)][4] and not by[(520, 22016)][4] and not by[(129, 65800)][4]


REQUIRED = {
    # main loop: zero, one, several steady iterations; both stage parities at the exit; 1-4 extension tiles; short K with and without
    "bf16:steady0", "bf16:steady1", "bf16:steady2", "bf16:exit_stage0", "bf16:exit_stage1", "bf16:ext0", "bf16:ext1", "bf16:ext2", "bf16:ext4",
    "bf16:nk1", "bf16:nk2", "bf16:nk3", "bf16:nk1+ext", "bf16:nk2+ext", "bf16:nk3+ext",
    "i8:steady0", "i8:steady1", "i8:steady2", "i8:exit_stage0", "i8:exit_stage1", "i8:ext0", "i8:ext1", "i8:ext2",
    "i8:nk1", "i8:nk2", "i8:nk3", "i8:nk1+ext", "i8:nk2+ext", "i8:nk3+ext", "i8f32:nk1", "i8f32:nk3", "i8f32:steady2",
    # every epilogue of the three entry points, and each one that has a half-tile instance on the half tile
    "bf16:none", "bf16:res", "bf16:bias", "bf16:gelu", "bf16:colscale", "bf16:swiglu_bwd", "bf16:swiglu_fwd", "bf16:rope",
    "i8:none", "i8:res", "i8:swiglu_fwd", "i8:rope", "i8f32:none",
    "bf16:none:half", "bf16:res:half", "bf16:bias:half", "bf16:gelu:half", "bf16:colscale:half", "bf16:swiglu_bwd:half", "bf16:rope:half",
    "i8:none:half", "i8:res:half", "i8:rope:half", "i8f32:none:half", "bf16:half+ext", "i8:half+ext", "half:rope_boundary_inside",
    # the launcher's split: tails 1, 2, 128; grid_m 1 and 2; ragged rows under it; and the three ways it does not split
    "half:tail1", "half:tail2", "half:tail128", "half:grid_m1", "half:grid_m2", "half:ragged_rows",
    "nosplit:tail>128", "nosplit:tail%grid_m", "nosplit:ragged_n",
    # rows and columns
    "rows:lt_tile", "rows:whole", "rows:ragged", "rows:group4+1", "xcd:remainder", "cols:lt_half", "cols:lt_tile", "cols:whole", "cols:ragged",
    "bf16:strided", "i8:strided", "i8f32:strided",
    "mv:zero", "mv:inside", "mv:tile_edge", "mv:eq_M", "mv:gt_M", "mv:split_grid_shrinks",
    "splitk:tiles_per_range1", "splitk:tiles_per_range2", "splitk:tiles_per_range3", "splitk:plain", "splitk:inv", "splitk:scale", "splitk:inv+scale",
    "splitk:inv+scale+mv",
    "tn:empty", "tn:lt64", "tn:eq64", "tn:ragged", "tn:multi", "tn:slice", "tn:im2col", "tn:mv<=0", "tn:mv", "tn:mv>M",
    "tn:grid1x1", "tn:grid1x2", "tn:grid2x3", "tn:grid3x1",
}


def test_the_table_covers_every_class():
    have = set()
    for c in G.CASES + G.TN_CASES:
        have |= G.classes(c)
    assert not REQUIRED - have, sorted(REQUIRED - have)


def test_strides_are_what_the_kernels_accept():
    for c in G.CASES:
        s = G.strides(c)
        unit = 16 if c.tk == 128 else 8
        assert s["lda"] % unit == 0 and s["ldb"] % unit == 0 and s["lda"] > c.K and s["ldb"] > c.K
        assert all(s[k] % 8 == 0 for k in ("ldc", "lde", "lda2", "ldb2")) and s["ldc"] > (2 * c.N if c.epi == "swiglu_bwd" else c.N)
