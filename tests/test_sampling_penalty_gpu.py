"""GPU: the sampler with penalties, a count table and token log-probabilities (llx.kernels.sample -> llx_sample_rows_ext, csrc/sample.hip)
against the plain sampler on the host-penalised row - bit for bit - and the fp64 log-probability of tests/sampling_penalty_cases.py."""
import math

import pytest
import torch

from tests import sampling_cases as C
from tests import sampling_penalty_cases as PC
from tests.beam_cases import SCORE_TOL

pytestmark = pytest.mark.gpu
SEED = 11
GREEDY = (0, 1.0, 0.0)


@pytest.fixture(scope="module")
def K():
    from llx import kernels

    return kernels


_CASES: dict = {}


def _case(name, cuda):
    """(CPU logits view, device view with the same stride and offset, CPU counts, the host-penalised fp32 rows on the device), once."""
    if name not in _CASES:
        s = C.SHAPE[name]
        x = C.make_logits(s)
        counts = PC.make_counts(name, x)
        pen = PC.penalize(x, counts, PC.THETA, PC.ALPHA_P, PC.ALPHA_F).contiguous().to(cuda)
        _CASES[name] = (x, C.to_device(x, s, cuda), counts, pen)
    return _CASES[name]


def _pos(R, cuda):
    return torch.arange(R, dtype=torch.int64, device=cuda) * 7 + 1000


def _kw(point):
    k, p, T = point
    return dict(temperature=T, top_k=k, top_p=p, seed=SEED)


def _same(a, b):
    """tokens, u, threshold and kept count, bit for bit (the threshold by its bits: -0.0 and 0.0 differ)."""
    return (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
            and torch.equal(a[3], b[3]))


@pytest.mark.parametrize("name", PC.GPU_SHAPES)
def test_bit_for_bit_against_the_plain_sampler_on_the_penalised_row(K, cuda, name):
    """The extended sampler on (logits, counts, penalties) = the plain sampler on penalize(logits, counts): tokens and aux, no tolerance,
    at count strides V and V + 5; and the table afterwards is the table before plus one at (r, token_r), the padding untouched."""
    x, xd, counts, pen = _case(name, cuda)
    R, V = x.shape
    pos = _pos(R, cuda)
    for point in (GREEDY,) + PC.POINTS:
        want = K.sample(pen, pos=pos, aux=True, **_kw(point))
        plain = K.sample(xd, pos=pos, aux=True, **_kw(point))
        if point == GREEDY:
            assert (want[0] != plain[0]).float().mean().item() >= 0.9  # the penalties matter (CONDITION), so ignoring the counts fails below
        for ldc in (V, V + 5):
            table = PC.strided_counts(counts, ldc, cuda)
            got = K.sample(xd, pos=pos, aux=True, counts=table, **PC.PENALTIES, **_kw(point))
            assert _same(got, want), (name, point, ldc)
            after = PC.strided_counts(counts, ldc, cuda)
            after[torch.arange(R, device=cuda), want[0]] += 1
            assert torch.equal(table, after), (name, point, ldc)


def test_finished_rows_touch_nothing(K, cuda):
    """A finished row repeats eos and leaves its counts row and its logprob_history row as they were; the others are updated."""
    x, xd, counts, pen = _case("v1000", cuda)
    R, V = x.shape
    pos = torch.arange(R, dtype=torch.int64, device=cuda) + 1000
    want = K.sample(pen, pos=pos, **_kw(PC.POINTS[0]))
    eos = int(want[20])
    fin = torch.zeros(R, dtype=torch.int32, device=cuda)
    fin[[12, 40]] = 1
    was = fin.bool().clone()
    table = counts.to(cuda)
    hist = torch.full((R, R), -7, dtype=torch.int64, device=cuda)
    lp = torch.full((R, R), -7.0, dtype=torch.float32, device=cuda)
    got = K.sample(xd, pos=pos, counts=table, history=hist, hist_base=1000, logprob_history=lp, eos_id=eos, finished=fin, **PC.PENALTIES,
                   **_kw(PC.POINTS[0]))
    assert torch.equal(got, torch.where(was, torch.tensor(eos, device=cuda), want))
    after = counts.to(cuda)
    live = (~was).nonzero().flatten()
    after[live, want[live]] += 1
    assert torch.equal(table, after)
    # row r writes column r (pos - base) of both histories, a finished row nothing
    d = torch.arange(R, device=cuda)
    assert torch.equal(hist[d, d], torch.where(was, torch.tensor(-7, device=cuda), want))
    assert bool((lp[d, d][was] == -7.0).all()) and bool((lp[d, d][~was] < 0).all())
    off = ~torch.eye(R, dtype=torch.bool, device=cuda)
    assert bool((hist[off] == -7).all()) and bool((lp[off] == -7.0).all())
    assert torch.equal(fin.bool(), was | (want == eos))


@pytest.mark.parametrize("name", ["v1001_stride1003", "v8197"])
def test_off_means_off(K, cuda, name):
    x, xd, counts, _ = _case(name, cuda)
    R, V = x.shape
    pos = _pos(R, cuda)
    for point in (GREEDY,) + PC.POINTS:
        plain = K.sample(xd, pos=pos, aux=True, **_kw(point))
        # non-zero counts, every penalty at "off": the plain sampler's bits, and the counts are still kept
        table = counts.to(cuda)
        got = K.sample(xd, pos=pos, aux=True, counts=table, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, **_kw(point))
        assert _same(got, plain), (name, point)
        after = counts.to(cuda)
        after[torch.arange(R, device=cuda), plain[0]] += 1
        assert torch.equal(table, after)
        # no counts, only the log-probability
        hist = torch.zeros(R, 7 * R, dtype=torch.int64, device=cuda)  # row r writes column 7 r
        lp = torch.zeros(R, 7 * R, dtype=torch.float32, device=cuda)
        got = K.sample(xd, pos=pos, aux=True, history=hist, hist_base=1000, logprob_history=lp, **_kw(point))
        assert _same(got, plain), (name, point)
        assert int((lp != 0).sum()) == R


@pytest.mark.parametrize("name", PC.GPU_SHAPES)
def test_log_probability(K, cuda, name):
    """|logp - fp64 restatement| <= SCORE_TOL on the RAW row, whatever the penalties; the same bits with and without penalties when the
    token is the same; two launches are bit-identical."""
    x, xd, counts, pen = _case(name, cuda)
    R, V = x.shape
    pos = torch.full((R,), 1000, dtype=torch.int64, device=cuda)  # one column for all rows
    runs = {}
    for point in (GREEDY, PC.POINTS[0]):
        for label, extra in (("raw", {}), ("off", dict(counts=True)), ("pen", dict(counts=True, **PC.PENALTIES))):
            extra = dict(extra)
            if extra.pop("counts", False):
                extra["counts"] = counts.to(cuda)
            hist = torch.zeros(R, 3, dtype=torch.int64, device=cuda)
            lp = torch.full((R, 3), 9.0, dtype=torch.float32, device=cuda)
            tok = K.sample(xd, pos=pos, history=hist, hist_base=999, logprob_history=lp, **extra, **_kw(point))
            assert bool((lp[:, [0, 2]] == 9.0).all()) and torch.equal(hist[:, 1], tok)
            runs[label] = (tok.cpu(), lp[:, 1].cpu())
            worst = 0.0
            for r in range(R):
                worst = max(worst, abs(float(lp[r, 1]) - PC.logprob64(x[r], int(tok[r]))))
            print(f"{name} {point} {label}: max |logp - fp64| = {worst:.3e}")
            assert worst <= SCORE_TOL, (name, point, label, worst)
            lp2 = torch.zeros_like(lp)
            if "counts" in extra:
                extra["counts"] = counts.to(cuda)
            K.sample(xd, pos=pos, history=hist, hist_base=999, logprob_history=lp2, **extra, **_kw(point))
            assert torch.equal(lp2[:, 1].view(torch.int32), lp[:, 1].view(torch.int32))
        # counts with every penalty off pick the raw run's tokens: the same log-probabilities, bit for bit
        assert torch.equal(runs["off"][0], runs["raw"][0]) and torch.equal(runs["off"][1].view(torch.int32), runs["raw"][1].view(torch.int32))
        same = runs["pen"][0] == runs["raw"][0]
        assert torch.equal(runs["pen"][1][same].view(torch.int32), runs["raw"][1][same].view(torch.int32))


def test_the_second_launch_sees_the_first_ones_count(K, cuda):
    """One row, its two largest logits 5.0 and 4.5, greedy, frequency_penalty 1, an empty table: the first launch picks the larger and
    counts it, so the second picks the other."""
    V, hi, lo = 4100, 3001, 77
    x = torch.zeros(1, V, dtype=torch.bfloat16)
    x[0, hi], x[0, lo] = 5.0, 4.5
    xd = x.to(cuda)
    table = torch.zeros(1, V, dtype=torch.int32, device=cuda)
    pos = torch.zeros(1, dtype=torch.int64, device=cuda)
    first = K.sample(xd, temperature=0.0, pos=pos, counts=table, frequency_penalty=1.0)
    assert int(first) == hi and int(table[0, hi]) == 1 and int(table.sum()) == 1
    second = K.sample(xd, temperature=0.0, pos=pos, counts=table, frequency_penalty=1.0)
    assert int(second) == lo and int(table[0, lo]) == 1 and int(table.sum()) == 2


def test_wrapper_rejects(K, cuda):
    from llx._lib import LlxError

    x, xd, counts, _ = _case("v1000", cuda)
    R, V = x.shape
    pos = torch.zeros(R, dtype=torch.int64, device=cuda)
    table = counts.to(cuda)
    before = table.clone()
    hist = torch.zeros(R, 2, dtype=torch.int64, device=cuda)
    lp = torch.zeros(R, 2, dtype=torch.float32, device=cuda)
    for kw in (dict(counts=table, repetition_penalty=0.0), dict(counts=table, repetition_penalty=-1.0), dict(counts=table, presence_penalty=math.nan),
               dict(counts=table, frequency_penalty=math.nan), dict(counts=table, frequency_penalty=math.inf),
               dict(counts=table.long()), dict(counts=table[:, : V - 1]), dict(counts=table[: R - 1]), dict(counts=table[0]),
               dict(counts=table.cpu()), dict(counts=table.t().contiguous().t()), dict(repetition_penalty=1.3),
               dict(logprob_history=lp), dict(history=hist, logprob_history=lp.double()), dict(history=hist, logprob_history=lp[:, :1]),
               dict(history=hist, logprob_history=torch.zeros(R, 4, dtype=torch.float32, device=cuda)[:, :2])):
        with pytest.raises(LlxError):
            K.sample(xd, temperature=1.0, pos=pos, **kw)
    assert torch.equal(table, before) and not bool(lp.any())  # nothing was launched
