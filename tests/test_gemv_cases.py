"""CPU checks of the decode-GEMV cases (tests/gemv_cases.py): the restated dispatch puts every threshold where csrc/decode.hip has it
and the table holds every class of every axis for every weight kind; every case passes the exactness assertions of its float64
reference (so torch.equal is a fair bar for tests/test_gemv_classes_gpu.py); every planted fault changes at least one output of the
cases aimed at its class (so that bar would fail); and the bar the GEMV was held to before accepts three of those faults on Gaussian
data (which is why the exact operand families exist)."""
import pytest
import torch

from oracle import ref as O
from tests import gemv_cases as C


# ------------------------------------------------------------------------------------------------------------------ dispatch classes
def test_pass_thresholds():
    """Tokens per pass at both sides of every LDS threshold of gemv_run."""
    pc = C.pass_class
    for kind in ("bf16", "dora"):
        assert [pc(kind, 6144, m) for m in (1, 2, 3, 4)] == ["one"] * 4
        assert [pc(kind, 6152, m) for m in (1, 2, 3, 4)] == ["one", "one", "pairs", "pairs"]
        assert C.passes(kind, 6152, 3) == [(0, 2), (2, 1)] and C.passes(kind, 6152, 4) == [(0, 2), (2, 2)]
        assert [pc(kind, 14336, m) for m in (2, 3, 4)] == ["one", "pairs", "pairs"]
        assert [pc(kind, 14344, m) for m in (1, 2, 3, 4)] == ["one", "single", "single", "single"]
        assert pc(kind, 30720, 1) == "one" and pc(kind, 30728, 1) == "reject" and pc(kind, 520, 5) == "reject"
    assert [pc("i8d", 14336, m) for m in (3, 4)] == ["one", "one"] and [pc("i8d", 14352, m) for m in (2, 3, 4)] == ["one", "pairs", "pairs"]
    assert [pc("i8d", 30720, m) for m in (2, 4)] == ["one", "pairs"] and [pc("i8d", 30736, m) for m in (1, 2, 3, 4)] == ["one"] + ["single"] * 3
    assert pc("i8d", 32768, 4) == "single"
    assert [pc("i8w", 16, m) for m in (1, 2, 3, 4)] == ["one", "one", "pairs", "pairs"]
    assert [pc("i8w", 14336, m) for m in (2, 3)] == ["one", "pairs"] and [pc("i8w", 14352, m) for m in (1, 2, 3, 4)] == ["one"] + ["single"] * 3
    assert pc("i8w", 30720, 1) == "one" and pc("i8w", 30736, 1) == "reject"
    assert (C.lds_row("bf16", 8), C.lds_row("bf16", 2056), C.lds_row("i8w", 16), C.lds_row("i8d", 1024), C.lds_row("i8d", 1040)) == (2048, 4096, 2048, 2048, 3072)


def test_row_group_shapes():
    assert C.launch_shape(1) == (1, 1, 1, 4) and C.launch_shape(10) == (5, 1, 2, 8) and C.launch_shape(37) == (19, 1, 5, 20)
    assert C.launch_shape(4096) == (2048, 1, 512, 2048)
    assert C.launch_shape(4098) == (2049, 2, 257, 1028) and C.launch_shape(8194) == (4097, 3, 342, 1368)
    assert C.launch_shape(10, swiglu=True) == (5, 1, 2, 8) and C.launch_shape(4098, swiglu=True) == (2049, 2, 257, 1028)
    # waves with two / one groups at N = 4098, with three at N = 8194
    assert sum(1 for w in range(1028) if w + 1028 < 2049) == 1021 and sum(1 for w in range(1368) if w + 2 * 1368 < 4097) == 1361


@pytest.mark.parametrize("kind", C.KINDS)
def test_table_holds_every_class(kind):
    cs = [c for c in C.CASES.values() if c.kind == kind]
    i8 = kind in ("i8w", "i8d")
    _, piece, step, _ = C.geometry(kind)
    assert (piece, step) == ((1024, 4096) if i8 else (512, 2048))
    # K against PIECE and STEP; three steps = an odd count
    want_k = {16, 1008, 1024, 1040, 4096, 4112, 9216} if i8 else {8, 504, 512, 520, 2040, 2048, 2056, 4608}
    assert want_k <= {c.K for c in cs} and C.nsteps(kind, max(want_k)) == 3
    # tokens per pass: every multi-pass class with residual and with q|k|v, LoRA on each; M = 3 in one pass (the clamped fourth row)
    multi = {(C.pass_class(kind, c.K, c.M), c.M, c.epi) for c in cs if c.ranks and len(C.passes(kind, c.K, c.M)) > 1}
    assert {("pairs", m, e) for m in (3, 4) for e in ("res", "qkv")} | {("single", m, e) for m in (2, 3, 4) for e in ("res", "qkv")} <= multi
    assert {c.M for c in cs if C.pass_class(kind, c.K, c.M) == "one"} == ({1, 2} if kind == "i8w" else {1, 2, 3, 4})
    # rows
    plain = [c for c in cs if c.epi in ("none", "res")]
    assert {1, 10, 37, 4096, 4098, 8194} <= {c.N for c in plain}
    assert {C.launch_shape(c.N)[1] for c in plain} == {1, 2, 3}
    assert {C.nsteps(kind, c.K) for c in plain if c.N > 4096} >= {1, 2}
    assert {c.ns[0] for c in cs if c.epi == "swiglu"} == {5, 2049}
    # segments, epilogues, LoRA, strides
    assert {(4, 8, 5), (8, 3)} <= {c.ns for c in cs} and {len(c.ns) for c in cs if c.epi == "qkv"} == {1, 2, 3}
    assert {c.epi for c in cs} == {"none", "res", "qkv", "swiglu"}
    assert {(8,), (64,), (512,), (8, 24, 16)} <= {c.ranks for c in cs} and any(c.ranks and c.epi == "swiglu" for c in cs)
    assert {0.5, 2.0} == {c.lscale for c in cs if c.ranks}
    assert any(c.strided and c.ranks and c.epi == "res" for c in cs) and any(c.strided and c.epi == "qkv" for c in cs)
    assert {c.fam for c in cs} == ({"B", "G"} if kind == "i8d" else {"A", "B"}) and any(c.fam == "B" and not c.norm for c in cs)
    assert all(c.norm == (c.fam == "B") or not c.norm for c in cs)
    for c in cs:  # what stream_check_fill asks of the segments, so that no case is a reject by accident
        assert all(n % 4 == 0 for n in c.ns[:-1]) or c.epi == "swiglu"
        assert C.passes(kind, c.K, c.M) is not None and all(r % 8 == 0 and r <= 512 for r in c.ranks)


# ------------------------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("cid", list(C.CASES))
def test_case_is_exact(cid):
    """build + reference: the reference asserts that every fp32 intermediate is representable, the linear's sum fits bf16, no quantiser
    code sits on a tie - i.e. that the case has one correct answer."""
    d = C.build(cid)
    c = d["case"]
    ref = C.reference(d)
    assert ref["out"].shape == (c.M, c.n_out) and ref["out"].dtype is torch.bfloat16
    assert ref["out"].float().abs().max() > 0
    if c.fam == "A":
        assert ((d["x"] != 0).sum(1) <= 6).all() and (d["x"].float().abs() <= 2).all() and (d["x"][:, c.K - 1] != 0).all()
        if c.M > 1:
            assert not torch.equal(d["x"][0], d["x"][1])
    if c.strided:  # the gaps are poisoned
        assert torch.isnan(d["x"]._base.float()).any() and (d["out"]._base.float() == C.SENTINEL).all()
    if c.epi == "qkv":
        assert sorted(d["pos"].tolist()) != d["pos"].tolist() or c.M == 1
        for name in ("kc", "vc"):
            written = (ref[name].float() != C.SENTINEL).sum().item()
            assert written <= c.M * (c.N - 256) // 2 and ref[name].shape == d[name]._base.shape and d[name].stride()[1:] == (160, 160 * d[name].shape[1], 1)


@pytest.mark.parametrize("fault", C.FAULTS)
def test_fault_changes_its_cases(fault):
    assert C.FAULT_CASES[fault]
    for cid in C.FAULT_CASES[fault]:
        d = C.build(cid)
        good, bad = C.reference(d), C.reference(d, fault)
        assert any(not torch.equal(good[k], bad[k]) for k in ("out", "kc", "vc") if k in good), (fault, cid)


def test_every_kind_meets_the_faults_that_apply_to_it():
    kinds = {f: {C.CASES[cid].kind for cid in ids} for f, ids in C.FAULT_CASES.items()}
    assert set(kinds) == set(C.FAULTS)
    for f in ("drop_last8", "lds_pad", "pass2_stale", "group_repeat"):
        assert kinds[f] == set(C.KINDS), f
    assert kinds["i8w_halves_swapped"] == {"i8w"} and kinds["i8_adapter_before_round"] == {"i8w", "i8d"}
    assert kinds["scale_row_plus1"] == {"dora", "i8w", "i8d"} and kinds["res_before_round"] == {"dora", "i8w", "i8d"}


# ------------------------------------------------------------------------------------------------------------------ the old bar
def test_old_bar_accepts_a_dropped_column_and_two_wrong_rounding_points():
    """On Gaussian operands at the shape of the first plain-GEMV test (M 1, K 4096, N 4096) the former bar - max error within 1 % of the
    largest reference magnitude - accepts a dropped weight column (for about half of the columns tried: it depends on |x| there), a
    gain of 1.005 on every output, a residual added in front of the linear's bf16 rounding and an int8 adapter term added in front of
    the base's rounding, although each of them changes output bits."""
    K, N, M = 4096, 4096, 1
    x = O.randn("gc_old_x", (M, K), 1.0).bfloat16().double()
    w = O.randn("gc_old_w", (N, K), 0.05).bfloat16().double()
    want = x @ w.T
    accepted = 0
    for col in range(K - 16, K):  # whether a dropped column passes depends on |x[col]|: about a third of them do at this shape
        xd = x.clone()
        xd[:, col] = 0
        got = C.rbf(xd @ w.T)
        assert not torch.equal(got, C.rbf(want))
        accepted += C.old_bar_accepts(got, want)
    print(f"old bar: accepts {accepted} of 16 single dropped columns")
    assert accepted >= 1
    assert C.old_bar_accepts(C.rbf(1.005 * want), want) and not torch.equal(C.rbf(1.005 * want), C.rbf(want))
    res = O.randn("gc_old_r", (M, N), 1.0).bfloat16().double()
    want_r = C.rbf(want) + res  # what test_gemv_plain_and_residual compares with
    got_r = C.rbf(want + res)
    assert C.old_bar_accepts(got_r, want_r) and (got_r != C.rbf(want_r)).double().mean() > 0.1
    q, sc = O.quantize_int8_rowwise(w.bfloat16())
    lora = 2.0 * (x @ O.randn("gc_old_a", (16, K), 0.05).bfloat16().double().T) @ O.randn("gc_old_b", (N, 16), 0.05).bfloat16().double().T
    base = C.rbf(x @ q.double().T) * sc.double()
    want_l = C.rbf(C.rbf(base) + lora)
    got_l = C.rbf(base + lora)
    assert C.old_bar_accepts(got_l, want_l) and not torch.equal(got_l, want_l)
