"""CPU checks of the LoRA rank cases (tests/lora_cases.py): every case reaches the plan class it is named for, the product's documented
rounding points sit inside the bars of the GPU tests (tests/test_lora_ranks_gpu.py), and structurally wrong products - a dropped rank
column, exchanged members, a lost scale, a lost in-place accumulation - land at least ten times outside them."""
import pytest
import torch

from oracle import ref as O
from tests import lora_cases as C


def _plans(case, cfg, which):
    from llx.ops import GroupPlan

    return GroupPlan(C.group_modules(C.group_data(case, cfg, which, M=16)))


@pytest.mark.parametrize("name", list(C.CASES))
def test_every_case_reaches_its_class(name):
    """The planner (llx.ops.GroupPlan, built on CPU modules) makes of every case what CASES says, at MID and at TINY dims."""
    from llx import kernels as K

    case = C.CASES[name]
    assert K.rmsnorm_skinny_ok(C.MID.embed_dim)
    for cfg, facts in ((C.MID, case.mid), (O.TINY, case.tiny)):
        for which, want in zip(("qkv", "gu"), facts):
            g = _plans(case, cfg, which)
            assert (g.fused, g.R) == (want.fused, want.R), (name, which, g.fused, g.R)
            assert g.ranks == list(case.group_ranks(which))
            assert g.rope_fusable() == want.fused and (which == "qkv" or g.swiglu_fusable() == want.fused)
            if want.fused:
                assert g.R <= 64 and (g._kranges() is not None) == want.kranges and (g._tn_segs() is not None) == want.segs, (name, which)
                assert want.nb == -(-g.R // 16)
            else:  # per-member plans: each member is its own skinny product
                assert all(m.rank <= 64 for m in g.members)


def test_nb_classes_of_the_skinny_kernels_are_covered():
    """ceil(R / 16) of every fused group at MID - the register tiling csrc/skinny.hip picks (NT kernels: 1 | 2 | 4, TN and the fused norm
    1..4) - and of the per-member products of the unfused ones."""
    nb = {n: tuple(p.nb if p.fused else None for p in c.mid) for n, c in C.CASES.items()}
    assert nb == {"r1": (1, 1), "r5": (1, 1), "r21": (4, 3), "r22": (None, 3), "r32": (None, 4), "r33": (None, None), "r64": (None, None),
                  "r8-32-8": (3, 2), "r16-none-16": (None, 2), "r16-scales": (None, 2)}
    per_member = sorted({-(-r // 16) for c in C.CASES.values() for p, rs in zip(c.mid, (c.qkv, (c.rest,) * 2)) if not p.fused for r in rs if r})
    assert per_member == [1, 2, 3, 4]  # ranks 16; 22, 32; 33; 64
    assert C.CASES["r21"].mid[0].R == 63 and C.CASES["r32"].mid[1].R == 64  # one clamped row; none and no zero column


def test_mid_group_descriptors():
    """The block-diagonal descriptors the fused cases hand to the kernels: at r21 every 16-row block of B^T but the first holds rows of
    two members and takes the union of their k ranges."""
    g = _plans(C.CASES["r21"], C.MID, "qkv")
    assert g._kranges() == [0, 1024, 0, 1280, 1024, 1536, 1280, 1536]
    assert g._tn_segs() == [(0, 1024, 0, 21), (1024, 1280, 21, 42), (1280, 1536, 42, 63)]
    g = _plans(C.CASES["r8-32-8"], C.MID, "qkv")  # wk's 32 ranks start at row 8: they straddle 16-row blocks 0, 1 and 2
    assert g._kranges() == [0, 1280, 1024, 1280, 1024, 1536, 0, 0]
    g = _plans(C.CASES["r32"], C.MID, "gu")
    assert g._kranges() == [0, 2048, 0, 2048, 2048, 4096, 2048, 4096] and g._tn_segs() == [(0, 2048, 0, 32), (2048, 4096, 32, 64)]


@pytest.mark.parametrize("which", ["qkv", "gu"])
@pytest.mark.parametrize("name", list(C.CASES))
def test_rounding_inside_the_bar_and_mutants_outside(name, which):
    """group_math(rounded=True) - the product's arithmetic with its rounding points - passes the GEMM bar (2^-7 of max|ref| plus 2^-7
    relative) against the float64 ground truth on y, dx, dA_i, dB_i; every mutant misses it by 10x or more on the output it corrupts."""
    case = C.CASES[name]
    d = C.group_data(case, C.MID, which)
    fused = (case.mid[0] if which == "qkv" else case.mid[1]).fused
    ref = C.group_math(d)
    got = C.group_math(d, rounded=True, fused=fused)
    base = d["x"].double() @ torch.cat(d["W"]).double().T
    share = ((ref["y"] - base).pow(2).mean().sqrt() / base.pow(2).mean().sqrt()).item()
    assert 0.5 <= share <= 2.0, share
    worst = {"y": C.over_bar(got["y"], ref["y"]), "dx": C.over_bar(got["dx"], ref["dx"])}
    for k in ("dA", "dB"):
        worst[k] = max(C.over_bar(g, r) for g, r in zip(got[k], ref[k]) if r is not None)
    margins = {}
    for mut in C.MUTANTS:
        bad = C.group_math(d, rounded=True, fused=fused, mutant=mut)
        key = "dx" if mut == "dx_last_only" else "y"
        margins[mut] = C.over_bar(bad[key], ref[key])
    print(f"[{name} {which}] share {share:.2f}; restated / bar " + " ".join(f"{k} {v:.2f}" for k, v in worst.items())
          + "; mutants / bar " + " ".join(f"{k} {v:.0f}x" for k, v in margins.items()))
    assert max(worst.values()) <= 1.0, worst
    assert min(margins.values()) >= 10.0, margins


@pytest.mark.parametrize("name", list(C.CASES))
def test_probe_columns_are_visible(name):
    """The first / last rank probes of the GPU test: with B zero except one column, taking the neighbouring column of t instead (an
    off-by-one in a clamp or a member offset) misses the bar by 10x or more - for ranks that have a neighbour."""
    case = C.CASES[name]
    d = C.group_data(case, C.MID, "qkv")
    for c_of in (lambda r: 0, lambda r: r - 1):
        B = C.probe_B(d, c_of)
        ref = C.group_math(d, B=B)["y"]
        assert C.over_bar(C.group_math(d, rounded=True, B=B)["y"], ref) <= 1.0
        shifted = [None if b is None else torch.roll(b, 1, dims=1) for b in B]
        if all(b is None or b.shape[1] > 1 for b in B):
            assert C.over_bar(C.group_math(d, rounded=True, B=shifted)["y"], ref) >= 10.0
        zeroed = [None if b is None else torch.zeros_like(b) for b in B]
        assert C.over_bar(C.group_math(d, rounded=True, B=zeroed)["y"], ref) >= 10.0


@pytest.mark.parametrize("name", list(C.CASES))
def test_layer_output_sees_adapter_and_scale(name):
    """O.layer at MID, S = 320: removing the adapters, or running them at scale 1 instead of 2, moves the output by at least 10x the
    layer test's output bar (0.02 of max|ref|) - unlike O.init_lora's B of std 0.01 at scale 1, which that bar cannot see."""
    case = C.CASES[name]
    cfg = C.MID
    base = {k: v.bfloat16().float() for k, v in O.init_params(cfg._replace(vocab_size=8)).items() if k.startswith("layers.0.")}
    p = dict(base)
    p.update({k: v.bfloat16().float() for k, v in C.layer_lora(case, cfg).items()})
    x = O.randn("x_full", (1, C.M_TOK, cfg.embed_dim), 0.5).bfloat16().float()
    table = O.rope_table(cfg)[: C.M_TOK]
    ref = O.layer(x, p, 0, cfg, table, None, C.SCALE)
    bar = 0.02 * ref.abs().max().item()
    d_none = (O.layer(x, base, 0, cfg, table, None, C.SCALE) - ref).abs().max().item()
    d_scale = (O.layer(x, p, 0, cfg, table, None, 1.0) - ref).abs().max().item()
    print(f"[{name}] layer output: no adapters {d_none / bar:.0f}x the bar, scale 1 {d_scale / bar:.0f}x")
    assert d_none >= 10 * bar and d_scale >= 10 * bar
