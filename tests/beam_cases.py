"""The case table of the beam-search tests (tests/test_beam_cases.py on the host, tests/test_beam_gpu.py on the device): each case is a
short search - the logits rows of every step, given, not produced by a model - built so that every decision of the walk keeps an fp64
margin of at least MARGIN in log-probability, which test_beam_cases.py asserts.

A case's rows are normal draws of standard deviation `std` rounded to the case's dtype (|z| <= 64), then `force`d: (step, row, token,
delta) sets that logit to the row's maximum + delta (rounded to the dtype), which is how an eos_id gets into a shortlist at a chosen rank.
"""
from typing import NamedTuple

from oracle import ref as O

MARGIN = 1e-2
SCORE_TOL = 1e-3  # per accumulated step: fp32 on |z| <= 64 errs at the order of 1e-5 per step, two decades below MARGIN


class Case(NamedTuple):
    name: str
    W: int
    V: int
    dtype: str  # "bf16" | "fp32"
    n: int  # max_new_tokens
    steps: int  # steps the table drives (the last may find the state frozen)
    eos_id: int | None = None
    length_penalty: float = 1.0
    std: float = 3.0
    force: tuple = ()
    seed: int = 0  # chosen so that the case keeps MARGIN (test_beam_cases.py asserts it)
    ld: int | None = None  # row stride in elements (None: V)
    offset: int = 0  # elements in front of the first row
    integer: bool = False  # integer logits: rows full of exact ties


CASES = (
    # the odd vocabulary on a row stride and a start that are no multiple of 16 bytes; an eos second in row 0's shortlist at the init step
    Case("odd_fp32", 3, 1001, "fp32", 6, 4, eos_id=7, force=((0, 0, 7, -0.75), (2, 1, 7, 1.5)), ld=1003, offset=3),
    Case("odd_bf16", 3, 1001, "bf16", 6, 4, eos_id=7, force=((0, 0, 7, -0.75), (2, 1, 7, 1.5)), ld=1003, offset=3, seed=1),
    # the production vocabulary
    Case("vocab_bf16", 2, 128_256, "bf16", 4, 3, eos_id=128_001, force=((1, 1, 128_001, 2.0),), std=2.0),
    Case("vocab_fp32", 2, 128_256, "fp32", 3, 3, std=2.0),
    # the widest beam; the budget ends the search (no eos_id), and one more step finds it frozen
    Case("w16_fp32", 16, 4099, "fp32", 3, 4, std=12.0, seed=19),
    Case("w16_bf16_eos", 16, 1001, "bf16", 5, 4, eos_id=1000, force=((1, 3, 1000, 0.5), (2, 0, 1000, 1.0), (2, 9, 1000, -0.5)),
         std=8.0, seed=1),
    # a bank replacement: with length_penalty 2 a later, longer hypothesis beats the one that finished at step 0, inside one walk
    Case("replace", 2, 67, "fp32", 8, 5, eos_id=5, length_penalty=2.0,
         force=((0, 0, 5, -0.5), (2, 0, 5, 3.0), (2, 1, 5, 3.0))),
    # the bank fills (W hypotheses): done before the budget; two more steps are frozen
    Case("bank_full", 2, 67, "bf16", 9, 4, eos_id=66, length_penalty=0.0, force=((0, 0, 66, 1.0), (1, 0, 66, 2.0))),
    # integer logits: every row is full of exact ties, ordered by the token index alone
    Case("ties_fp32", 3, 257, "fp32", 4, 4, eos_id=11, std=1.2, integer=True, force=((1, 2, 11, 1.0),), seed=11),
    Case("ties_bf16", 4, 130, "bf16", 3, 3, std=1.0, integer=True, seed=1),
)


def rows_of(case: Case) -> list:
    """[steps] fp32 tensors [W, V]: the logits of every step, holding values of the case's dtype exactly."""
    out = []
    for k in range(case.steps):
        z = O.randn(f"beam_case_{case.name}_{k}", (case.W, case.V), case.std, seed=1234 + case.seed).clamp_(-60, 60)
        if case.integer:
            z = z.round()
        if k == 0:
            z[1:] = z[0]  # the rows after the prefill are one row
        if case.dtype == "bf16":
            z = z.bfloat16().float()
        for step, r, t, delta in case.force:
            if step == k:
                peak = z[r].max() + delta
                rows = range(case.W) if k == 0 else (r,)
                for rr in rows:
                    z[rr, t] = peak.bfloat16().float() if case.dtype == "bf16" else peak
        out.append(z)
    return out


def run_reference(case: Case, margins=None, used=None) -> list:
    """The host reference on the case: per step (parents, tokens fed next, scores, histories, bank, done) after the step."""
    from llx import sampling as S

    st, trace = S.beam_state(case.W), []
    for z in rows_of(case):
        parent = S.beam_step(st, z.double().tolist(), case.W, max_new_tokens=case.n, eos_id=case.eos_id, length_penalty=case.length_penalty,
                             margins=margins, used=used)
        trace.append(dict(parent=parent, s=list(st["s"]), hist=[list(h) for h in st["hist"]], bank=[(list(t), f) for t, f in st["bank"]],
                          done=st["done"], steps=st["steps"]))
    return trace
