"""CPU: the host restatement of the sampler's penalties (tests/sampling_penalty_cases.py), llx.sampling.check_penalties, and the
condition that keeps the GPU tests honest: on every shape they use, the penalties change the greedy pick of >= 90 % of the rows."""
import math

import pytest
import torch

from tests import sampling_cases as C
from tests import sampling_penalty_cases as PC


def test_zero_counts_keep_the_bits():
    x = C.make_logits(C.SHAPE["v1000"])
    x = x.clone()
    x[0, :4] = torch.tensor([0.0, -0.0, -math.inf, 3.0])
    got = PC.penalize(x, torch.zeros(x.shape, dtype=torch.int32), PC.THETA, PC.ALPHA_P, PC.ALPHA_F)
    assert got.dtype is torch.float32 and torch.equal(got.view(torch.int32), x.float().view(torch.int32))


def test_seen_logits_move_as_the_hf_rule_says():
    x = torch.tensor([2.6, -2.0, 0.0, -math.inf, 1.0, -1.0])
    c = torch.tensor([1, 1, 1, 4, 0, 0], dtype=torch.int32)
    got = PC.penalize(x, c, 1.3, 0.0, 0.0)
    f = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    assert got[0] == f(2.6) / f(1.3) and got[0] < x[0]     # a positive seen logit is divided: it shrinks
    assert got[1] == f(-2.0) * f(1.3) and got[1] < x[1]    # a negative one is multiplied: it falls further
    assert got[2] == 0.0 and got[3] == -math.inf           # 0 and -inf stay what they are
    assert torch.equal(got[4:], x[4:])                     # unseen: untouched
    both = PC.penalize(x, c, 1.3, 0.5, 0.25)
    assert both[0] == f(2.6) / f(1.3) - (f(0.5) + f(0.25) * f(1.0))
    assert both[3] == -math.inf                            # -inf - finite
    assert PC.penalize(x, c, 1.0, 0.0, -1.0)[1] == -1.0    # a negative frequency penalty rewards repetition


def test_check_penalties():
    from llx._lib import LlxError
    from llx.sampling import check_penalties, penalties_on

    check_penalties(1.0, 0.0, 0.0)
    check_penalties(1.3, -0.5, 2)
    for bad in ((0.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (math.nan, 0.0, 0.0), (math.inf, 0.0, 0.0), (1.0, math.nan, 0.0), (1.0, 0.0, math.inf),
                (1.0, -math.inf, 0.0), ("1", 0.0, 0.0), (1.0, None, 0.0)):
        with pytest.raises(LlxError):
            check_penalties(*bad)
    assert not penalties_on(1.0, 0.0, 0.0) and penalties_on(1.3, 0.0, 0.0) and penalties_on(1.0, -0.1, 0.0) and penalties_on(1.0, 0.0, 0.2)


def test_logprob64_is_log_softmax():
    x = C.make_logits(C.SHAPE["v1000"])[0]
    want = torch.log_softmax(x.double(), 0)
    for t in (0, 17, 999):
        assert abs(PC.logprob64(x, t) - float(want[t])) < 1e-12


@pytest.mark.parametrize("name", PC.CONDITION_SHAPES)
def test_condition_the_penalties_change_the_greedy_pick(name):
    x = C.make_logits(C.SHAPE[name])
    counts = PC.make_counts(name, x)
    assert counts.dtype is torch.int32 and counts.shape == x.shape and int(counts.min()) == 0 and int(counts.max()) <= 5
    share = (counts > 0).float().mean().item()
    assert 0.05 < share < 0.15
    plain = PC.lowest_argmax(x)
    pen = PC.lowest_argmax(PC.penalize(x, counts, PC.THETA, PC.ALPHA_P, PC.ALPHA_F))
    changed = (plain != pen).float().mean().item()
    print(f"{name}: greedy pick changed in {100 * changed:.0f} % of {x.shape[0]} rows")
    assert changed >= 0.9, (name, changed)
