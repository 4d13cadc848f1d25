"""CPU: the beam-search rule on the host (llx.sampling.beam_shortlist / beam_step).  The two-stage reference - a shortlist
of W + 1 per row, then the merge - equals a brute-force sort of all W * V candidates in fp64; the walk never reads a shortlist past its
W + 1 entries; and every case of tests/beam_cases.py keeps the decision margin the device tests rely on."""
import math

import pytest

from oracle import ref as O
from tests import beam_cases as BC


def _brute_step(st, rows, W, n_max, eos_id, lp, taken):
    """One step by the definition: every (row, token) is a candidate, ordered by (score descending, row ascending, logit descending =
    equal here, token ascending); `taken` receives how many candidates of one row the walk consumed, at most."""
    if st["done"]:
        return list(range(W))
    n, live_rows = st["steps"] + 1, (1 if st["steps"] == 0 else W)
    cands = []
    for r in range(live_rows):
        z = rows[r]
        zmax = max(z)
        lse = math.log(math.fsum(math.exp(v - zmax) for v in z))
        cands += [(-(st["s"][r] + ((v - zmax) - lse)), r, t) for t, v in enumerate(z)]
    cands.sort()
    parent, s, hist, per_row = [], [], [], [0] * W

    def offer(tokens, final):
        bank = st["bank"]
        if len(bank) < W:
            bank.append((tokens, final))
            return
        worst = min(range(W), key=lambda i: (bank[i][1], i))
        if final > bank[worst][1]:
            bank[worst] = (tokens, final)

    for neg, r, t in cands:
        if len(parent) == W:
            break
        per_row[r] += 1
        if eos_id is not None and t == eos_id:
            offer(st["hist"][r] + [t], -neg / n ** lp)
        else:
            parent.append(r)
            s.append(-neg)
            hist.append(st["hist"][r] + [t])
    taken.append(max(per_row))
    st.update(s=s, hist=hist, steps=n)
    if len(st["bank"]) == W or n == n_max:
        st["done"] = True
        for j in range(W):
            offer(hist[j], s[j] / n ** lp)
    return parent


@pytest.mark.parametrize("W,V,integer,eos_id,lp", [(2, 9, False, 3, 1.0), (3, 40, False, 5, 0.0), (3, 40, True, 5, 2.0), (4, 23, True, 0, 1.0),
                                                   (5, 64, True, None, 1.0), (16, 33, True, 2, 0.7), (16, 40, False, 1, 1.0)])
def test_two_stage_reference_equals_the_full_sort(W, V, integer, eos_id, lp):
    from llx import sampling as S

    n_max, a, b, taken, used = 7, S.beam_state(W), S.beam_state(W), [], []
    for k in range(n_max + 1):  # the last step finds both frozen
        z = O.randn(f"beam_brute_{W}_{V}_{k}", (W, V), 1.5 if integer else 3.0)
        z = (z.round() if integer else z).double()
        if k == 0:
            z[1:] = z[0]
        rows = z.tolist()
        pa = S.beam_step(a, rows, W, max_new_tokens=n_max, eos_id=eos_id, length_penalty=lp, used=used)
        pb = _brute_step(b, rows, W, n_max, eos_id, lp, taken)
        assert pa == pb, k
        assert a["hist"] == b["hist"] and a["done"] == b["done"] and a["steps"] == b["steps"], k
        assert [t for t, _ in a["bank"]] == [t for t, _ in b["bank"]], k
        assert a["s"] == pytest.approx(b["s"], abs=1e-12) and [f for _, f in a["bank"]] == pytest.approx([f for _, f in b["bank"]], abs=1e-12)
    assert a["done"] and S.beam_ranked(a)
    # W + 1 entries of a row are enough: the full sort never consumed more of one row, and the reference never looked past rank W
    assert max(taken) <= W + 1 and max(used) <= W


def test_shortlist_orders_ties_by_index():
    from llx.sampling import beam_shortlist

    z = [1.0, 3.0, 3.0, -2.0, 3.0, 1.0, 0.0]
    got = beam_shortlist(z, 4)
    assert [t for _, t in got] == [1, 2, 4, 0, 5]
    lse = math.log(sum(math.exp(v - 3.0) for v in z))
    assert got[0][0] == pytest.approx(-lse, abs=1e-15) and got[3][0] == pytest.approx(-2.0 - lse, abs=1e-15)
    assert got[0][0] == got[1][0] == got[2][0]


def test_first_step_takes_the_best_distinct_tokens_of_row_0():
    from llx import sampling as S

    st = S.beam_state(3)
    assert st["s"] == [0.0, S.BEAM_DEAD, S.BEAM_DEAD]
    row = [0.0, 5.0, 1.0, 4.0, 3.0]
    parent = S.beam_step(st, [row] * 3, 3, max_new_tokens=4, eos_id=3)
    assert parent == [0, 0, 0] and st["hist"] == [[1], [4], [2]]  # token 3 is the eos: a finished hypothesis, not a beam
    assert [t for t, _ in st["bank"]] == [[3]] and not st["done"]
    frozen = dict(st, done=True)
    assert S.beam_step(frozen, [row] * 3, 3, max_new_tokens=4) == [0, 1, 2] and frozen["hist"] == st["hist"]


@pytest.mark.parametrize("case", BC.CASES, ids=lambda c: c.name)
def test_cases_keep_the_decision_margin(case):
    """Every point where the walk chooses - between walked candidates up to the first one left out, at bank entry, between the worst
    bank entry and the others when it is replaced, and in the final ranking - is decided by at least MARGIN in fp64."""
    from llx import sampling as S

    margins, used = [], []
    trace = BC.run_reference(case, margins, used)
    assert len(trace) == case.steps and margins and max(used) <= case.W
    for z in BC.rows_of(case):
        assert z.abs().max() <= 64
    st = dict(bank=trace[-1]["bank"])
    S.beam_ranked(st, margins)
    assert min(margins) >= BC.MARGIN, (case.name, min(margins))


def test_cases_cover_what_the_device_tests_claim():
    traces = {c.name: BC.run_reference(c) for c in BC.CASES if c.V < 10_000}
    by = {c.name: c for c in BC.CASES}
    assert {c.W for c in BC.CASES} >= {2, 3, 16} and {c.dtype for c in BC.CASES} == {"bf16", "fp32"} and any(c.V == 128_256 for c in BC.CASES)
    assert by["odd_fp32"].ld == 1003 and by["odd_fp32"].offset % 4 and by["odd_bf16"].offset % 8
    # an eos inside a shortlist at the first step
    assert traces["odd_fp32"][0]["bank"] and traces["odd_fp32"][0]["bank"][0][0] == [7]
    # a replacement: the hypothesis that finished first is gone from the full bank
    rep = traces["replace"]
    assert rep[0]["bank"][0][0] == [5] and rep[-1]["done"] and [5] not in [t for t, _ in rep[-1]["bank"]] and len(rep[-1]["bank"]) == 2
    # the frozen state: the table drives a step past done
    for name in ("w16_fp32", "bank_full", "replace"):
        t = traces[name]
        assert t[-2]["done"] and t[-1]["parent"] == list(range(by[name].W)) and t[-1]["hist"] == t[-2]["hist"], name
    assert traces["bank_full"][-1]["steps"] < by["bank_full"].n
