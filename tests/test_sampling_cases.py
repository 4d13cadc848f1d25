"""CPU: the sampler's host side (llx.sampling) and the soundness of the cases and acceptance rule of tests/sampling_cases.py."""
import pytest
import torch

from tests import sampling_cases as C


def test_uniform_is_the_documented_hash():
    from llx.sampling import uniform

    us = [uniform(1234, p, 0) for p in range(100_000)]
    assert all(0.0 <= u < 1.0 for u in us)
    assert all((u * 2 ** 24) == int(u * 2 ** 24) for u in us[:1000])
    mean = sum(us) / len(us)
    print(f"mean of 100000 uniforms at seed 1234: {mean:.5f}")
    assert abs(mean - 0.5) < 0.005
    assert abs(mean - 0.50026) < 5e-6  # the value of exactly this hash
    base = uniform(1, 2, 3)
    assert base != uniform(2, 2, 3) and base != uniform(1, 3, 3) and base != uniform(1, 2, 4)
    assert uniform(1, 2, 3) == base
    assert uniform(2 ** 64 - 1, 2 ** 40, 8191) < 1.0


def test_check_params():
    from llx._lib import LlxError
    from llx.sampling import check_params

    check_params(0.0, 0, 1.0, 0)
    check_params(0.8, 50, 0.9, 2 ** 64 - 1)
    for bad in ((-0.1, 0, 1.0, 0), (float("nan"), 0, 1.0, 0), (1.0, -1, 1.0, 0), (1.0, 1.5, 1.0, 0), (1.0, 0, 0.0, 0), (1.0, 0, 1.5, 0), (1.0, 0, 1.0, -1)):
        with pytest.raises(LlxError):
            check_params(*bad)


def _unique_rows(s, x, T, top_k, top_p):
    n = 0
    for r in range(s.R):
        row = C.Row(x[r], T, top_k)
        groups = row.acceptable_groups(top_p)
        assert row.exact_group(top_p) in groups
        n += len(groups) == 1
    return n


def _smallest_kept(s, x, T, top_k):
    smallest = 1.0
    for r in range(s.R):
        row = C.Row(x[r], T, top_k)
        w, _, W = row.running(row.g_k)
        smallest = min(smallest, float(w[row.kept_mask(row.g_k)].min() / W))
    return smallest


@pytest.mark.parametrize("s", C.SHAPES, ids=lambda s: s.name)
def test_condition_on_every_point_of_the_case(s):
    """The acceptance rule cannot hide a wrong kernel behind EPS on any (case, parameters) point the GPU test runs."""
    x = C.make_logits(s)
    assert (0, 0.9, 1.0) in C.params_for(s) and len(C.params_for(s)) >= 18
    assert s.points or C.params_for(s) == C.PARAMS
    assert all((1, p, t) in C.params_for(s) for p in C.TOP_PS for t in C.TEMPS)  # top_k = 1 runs everywhere
    for k, p, T in C.params_for(s):
        if p < 1:
            n = _unique_rows(s, x, T, k, p)
            print(f"{s.name} T={T} top_k={k} top_p={p}: {n}/{s.R} rows with exactly one acceptable threshold")
            assert n >= 0.9 * s.R
        if 0 < k <= 50 and p == 1.0:
            smallest = _smallest_kept(s, x, T, k)
            print(f"{s.name} T={T} top_k={k}: smallest kept probability {smallest:.2e}")
            assert smallest > 100 * C.EPS


def test_condition_rows_of_the_issue():
    for name, T, k, p in C.CONDITION_TOP_P:
        s = C.SHAPE[name]
        assert (k, p, T) in C.params_for(s)
        assert _unique_rows(s, C.make_logits(s), T, k, p) >= 0.9 * s.R
    for name, T, k in C.CONDITION_TOP_K:
        s = C.SHAPE[name]
        assert (k, 1.0, T) in C.params_for(s)
        assert _smallest_kept(s, C.make_logits(s), T, k) > 100 * C.EPS


def test_restatement_is_accepted_and_greedy_is_argmax():
    from llx.sampling import uniform

    for name in ("v1000", "v1000_ties", "v4100_f32", "v20011_f32"):
        s = C.SHAPE[name]
        x = C.make_logits(s)
        for k, p, T in C.PARAMS:
            for r in range(min(s.R, 4)):
                u = uniform(5, 100 + r, r)
                tok, th, kept = C.restate(x[r], T, k, p, u)
                assert C.accepts(x[r], T, k, p, u, tok, th, kept) == [], (name, k, p, T, r)
    row = torch.tensor([1.0, 3.0, -float("inf"), 3.0, 2.0, 3.0])
    assert C.restate(row, 0.0, 0, 1.0, 0.5) == (1, 3.0, 3)
    assert C.restate(torch.full((5,), -float("inf")), 0.0, 0, 1.0, 0.5)[0] == 0
    # -inf is never drawn, whatever u is
    row = torch.tensor([-float("inf"), 0.0, -float("inf"), 0.0, -float("inf")])
    assert {C.restate(row, 1.0, 0, 1.0, u)[0] for u in (0.0, 0.3, 0.5, 0.75, 1 - 2 ** -24)} == {1, 3}


def test_restatement_meets_the_frequency_bound():
    r = C.Row(C.stat_logits(), 1.0, C.STAT_TOP_K)
    tokens = r.draw_many(r.g_k, C.stat_uniforms())
    assert C.stat_check(tokens) == []
    # and draw_many is draw
    us = C.stat_uniforms()
    assert all(int(tokens[i]) == r.draw(r.g_k, float(us[i])) for i in range(0, C.STAT_R, 512))
    # a sampler that ignores the weights (uniform over the top 8) does not
    kept = r.kept_mask(r.g_k).nonzero().flatten()
    assert C.stat_check(kept[(us * 8).long()]) != []


@pytest.mark.parametrize("mutant", ["scan_off_by_one", "top_p_ge", "top_k_exact"])
def test_mutants_are_rejected(mutant):
    from llx.sampling import uniform

    rejected = 0
    for name in ("v1000", "v1000_ties"):
        s = C.SHAPE[name]
        x = C.make_logits(s)
        for k, p, T in ((50, 1.0, 1.0), (0, 0.9, 1.0), (50, 0.9, 0.7)):
            for r in range(8):
                u = uniform(9, r, r)
                tok, th, kept = C.restate(x[r], T, k, p, u, mutant=mutant)
                rejected += C.accepts(x[r], T, k, p, u, tok, th, kept) != []
    print(f"{mutant}: rejected on {rejected} of 48 rows")
    assert rejected > 0
