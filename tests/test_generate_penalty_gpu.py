"""GPU: generate() with sampler penalties and return_logprobs on the tiny model - token for token against hand loops that keep the count
table on the host and penalise each logits row with tests/sampling_penalty_cases.penalize.  Both arms see the same logits from the same
model calls and the penalty arithmetic is exact fp32, so the tokens are equal, not close."""
import math

import pytest
import torch

from oracle import ref as O
from tests import sampling_penalty_cases as PC
from tests.beam_cases import SCORE_TOL
from tests.util import bf16_params, build_model

pytestmark = pytest.mark.gpu
P, N = 40, 12
LENS = (40, 17, 29)
V = O.TINY.vocab_size
SAMPLED = dict(temperature=0.8, top_p=0.9, seed=3)
GREEDY_PEN = dict(repetition_penalty=1.3, frequency_penalty=0.25)
_MODELS: dict = {}


def _model(B, cuda, audio=False):
    if (B, audio) not in _MODELS:
        pb, _ = bf16_params(O.init_params(O.TINY, audio=True) if audio else O.init_params(O.TINY))
        model = build_model(O.TINY, pb, "cpu", audio=True) if audio else build_model(O.TINY, pb, "cpu")
        model.build_cache(inference=True, batch_size=B)
        _MODELS[(B, audio)] = model.to(cuda).eval()
    return _MODELS[(B, audio)]


def _prompt(cuda):
    return O.randint("generate_prompt", (1, P), 0, V).to(cuda)


def _prompts(B, cuda):
    return O.randint("generate_batch_prompts", (16, P), 0, V)[:B].to(cuda), [LENS[b % 3] for b in range(B)]


def _seeded(prompt, lens, on):
    """The host count table: each row's own prompt tokens (pads not counted), or zeros."""
    table = torch.zeros(prompt.shape[0], V, dtype=torch.int32)
    if on:
        for b, n in enumerate(lens):
            for t in prompt[b, :n].tolist():
                table[b, t] += 1
    return table


def _pick(row, table_row, pen, pos, r, sampling):
    """One token from the fp32 CPU logits row under the host-kept counts: penalise on the host, then the lowest-index argmax or the plain
    sampler (row index r and counter pos: what generate()'s launch uses for this row)."""
    from llx import kernels as K

    x = PC.penalize(row, table_row, pen.get("repetition_penalty", 1.0), pen.get("presence_penalty", 0.0), pen.get("frequency_penalty", 0.0))
    if sampling is None:
        return int((x == x.max()).nonzero()[0])
    dev = torch.device("cuda")
    rows = torch.zeros(r + 1, x.numel(), device=dev)  # the draw hashes the row index: put the row where generate() has it
    rows[r] = x.to(dev)
    return int(K.sample(rows, pos=torch.full((r + 1,), pos, dtype=torch.int64, device=dev), **sampling)[r])


def _hand_loop(model, first, step, lens, n, pen, table, sampling=None, eos=None):
    """The loop a user writes, for B rows.  first: the [B, V] logits of the prefill; step(tok [B, 1], pos [B]) -> the next [B, V].  Per row
    and token: penalise on the host with `table` (updated here), pick, record the RAW logits row.  A finished row feeds eos at its frozen
    position and its counts stay.  Returns (tokens per row, raw rows per row)."""
    B = len(lens)
    dev = first.device
    pos = [v - 1 for v in lens]
    fin, toks, rows = [False] * B, [[] for _ in range(B)], [[] for _ in range(B)]
    logits = first
    for k in range(n):
        x = logits.float().cpu()
        cur = []
        for b in range(B):
            if fin[b]:
                cur.append(eos)
                continue
            t = _pick(x[b], table[b], pen, pos[b], b, sampling)
            table[b, t] += 1
            toks[b].append(t)
            rows[b].append(x[b])
            pos[b] += 1
            fin[b] = eos is not None and t == eos
            cur.append(t)
        if all(fin) or k == n - 1:
            break
        logits = step(torch.tensor(cur, device=dev).view(B, 1), torch.tensor(pos, device=dev))
    return toks, rows


def _single(model, prompt, n, pen, table, sampling=None, eos=None):
    with torch.no_grad():
        first = model(prompt, input_pos=torch.arange(P, device=prompt.device))[0, -1:]
        return _hand_loop(model, first, lambda tok, pos: model(tok, input_pos=pos)[0], [P], n, pen, table, sampling, eos)


def _batch(model, prompt, lens, n, pen, table, sampling=None, eos=None):
    from llx.generate import prefill

    with torch.no_grad():
        first = prefill(model, prompt, lens)[:, 0]
        return _hand_loop(model, first, lambda tok, pos: model(tok, input_pos=pos[:, None])[:, 0], lens, n, pen, table, sampling, eos)


def _padded(toks, pad):
    T = max(len(r) for r in toks)
    return torch.tensor([r + [pad] * (T - len(r)) for r in toks])


def _looping_prompt(model, cuda):
    """P tokens: P - N random ones and the model's own greedy continuation of them.  The tiny model's greedy output repeats itself (runs of
    one token), so the plain continuation of this prompt goes on with a token the prompt is full of - which a table seeded from the prompt
    penalises from the first pick on and an empty table only once it has been drawn."""
    head = _prompt(cuda)[:, : P - N]
    return torch.cat((head, model.generate(head, N)), 1)


def test_greedy_equals_the_hand_loop(cuda):
    model = _model(1, cuda)
    prompt = _looping_prompt(model, cuda)
    plain = model.generate(prompt, N)
    runs = {}
    for seeded in (True, False):
        table = _seeded(prompt, [P], seeded)
        want, _ = _single(model, prompt, N, GREEDY_PEN, table)
        stats = {}
        got = model.generate(prompt, N, penalize_prompt=seeded, stats=stats, **GREEDY_PEN)
        assert isinstance(got, torch.Tensor) and got.shape == (1, N) and got.dtype is torch.int64
        assert got[0].tolist() == want[0], seeded
        assert stats["counts"].dtype is torch.int32 and torch.equal(stats["counts"].cpu(), table), seeded
        assert stats["tokens"] == N
        runs[seeded] = got
    print("plain   ", plain[0].tolist(), "\nseeded  ", runs[True][0].tolist(), "\nunseeded", runs[False][0].tolist())
    # on this prompt the penalties matter, and so does seeding the table from the prompt
    assert not torch.equal(runs[True], plain) and not torch.equal(runs[False], plain) and not torch.equal(runs[True], runs[False])
    stats = {}
    model.generate(prompt, N, stats=stats)
    assert stats["counts"] is None


def test_sampled_equals_the_hand_loop(cuda):
    model, prompt = _model(1, cuda), _prompt(cuda)
    table = _seeded(prompt, [P], True)
    want, _ = _single(model, prompt, N, PC.PENALTIES, table, SAMPLED)
    stats = {}
    got = model.generate(prompt, N, stats=stats, **PC.PENALTIES, **SAMPLED)
    assert got[0].tolist() == want[0]
    assert torch.equal(stats["counts"].cpu(), table)
    assert not torch.equal(got, model.generate(prompt, N, **SAMPLED))


def test_batch_with_eos_and_logprobs(cuda):
    """B = 3 ragged prompts, an eos_id that occurs: tokens equal the hand loop over the same batched calls, each row's counts start from
    its own prompt without pads, a finished row's counts are frozen; the log-probabilities follow the hand loop's raw logits rows."""
    B = 3
    model = _model(B, cuda)
    prompt, lens = _prompts(B, cuda)
    free = model.generate(prompt, N, prompt_lens=lens, **GREEDY_PEN)
    assert isinstance(free, torch.Tensor) and free.shape == (B, N)  # without the flag: the bare tensor
    eos = int(free[0, 5])
    table = _seeded(prompt, lens, True)
    want, rows = _batch(model, prompt, lens, N, GREEDY_PEN, table, eos=eos)
    assert len(want[0]) <= 6 and max(len(r) for r in want) > len(want[0])  # row 0 ends early, another row goes on
    for every in (1, 16):
        stats = {}
        out = model.generate(prompt, N, prompt_lens=lens, eos_id=eos, check_every=every, return_logprobs=True, stats=stats, **GREEDY_PEN)
        assert isinstance(out, tuple) and len(out) == 2
        tokens, logprobs = out
        T = max(len(r) for r in want)
        assert tokens.shape == (B, T) and logprobs.shape == (B, T) and logprobs.dtype is torch.float32
        assert torch.equal(tokens.cpu(), _padded(want, eos)), every
        assert torch.equal(stats["counts"].cpu(), table), every
        lp = logprobs.cpu()
        worst = 0.0
        for b in range(B):
            for k, t in enumerate(want[b]):
                worst = max(worst, abs(float(lp[b, k]) - PC.logprob64(rows[b][k], t)))
            assert bool((lp[b, len(want[b]):] == 0.0).all()), (b, every)  # after the row's eos
        print(f"check_every {every}: max |logp - fp64| = {worst:.3e}")
        assert worst <= SCORE_TOL


def test_logprobs_of_one_sequence(cuda):
    model, prompt = _model(1, cuda), _prompt(cuda)
    for pen, sampling in ((dict(), None), (PC.PENALTIES, SAMPLED)):
        table = _seeded(prompt, [P], True)
        want, rows = _single(model, prompt, N, pen, table, sampling)
        tokens, logprobs = model.generate(prompt, N, return_logprobs=True, **pen, **(sampling or {}))
        assert tokens[0].tolist() == want[0] and logprobs.shape == (1, N) and logprobs.dtype is torch.float32
        worst = max(abs(float(logprobs[0, k]) - PC.logprob64(rows[0][k], t)) for k, t in enumerate(want[0]))
        print(f"penalties {bool(pen)}: max |logp - fp64| = {worst:.3e}")
        assert worst <= SCORE_TOL
    # eos: the result is cut at it, and the log-probabilities with it
    eos = want[0][4]
    first = want[0].index(eos)
    tokens, logprobs = model.generate(prompt, N, return_logprobs=True, eos_id=eos, check_every=1, **PC.PENALTIES, **SAMPLED)
    assert tokens[0].tolist() == want[0][: first + 1] and logprobs.shape == (1, first + 1)
    assert isinstance(model.generate(prompt, N, eos_id=eos), torch.Tensor)


def test_audio_counts_come_from_the_text_prompt_only(cuda):
    Pa, Na, samples = 20, 8, 3200
    model = _model(1, cuda, audio=True)
    audio = O.uniform("generate_audio_clips", (3, samples), -0.1, 0.1)[:1].to(cuda)
    prompt = O.randint("generate_audio_prompts", (3, Pa), 0, V, seed=1234)[:1].to(cuda)
    A = model.audio_positions(samples)
    pen = dict(repetition_penalty=1.3)
    table = _seeded(prompt, [Pa], True)
    assert int(table.sum()) == Pa  # the text prompt only: the clip's positions contribute nothing
    with torch.no_grad():
        first = model(audio, prompt, input_pos=torch.arange(A + Pa, device=cuda))[:, -1]
        want, _ = _hand_loop(model, first, lambda tok, pos: model(None, tok, input_pos=pos)[:, 0], [A + Pa], Na, pen, table)
    stats = {}
    got = model.generate(audio, prompt, Na, stats=stats, **pen)
    assert got[0].tolist() == want[0]
    assert torch.equal(stats["counts"].cpu(), table) and int(table.sum()) == Pa + Na
    assert not torch.equal(got, model.generate(audio, prompt, Na))


def test_refusals_before_any_launch(cuda):
    from llx._lib import LlxError

    model, prompt = _model(1, cuda), _prompt(cuda)
    for kw, names in ((dict(num_beams=2, repetition_penalty=1.3), ("num_beams", "repetition_penalty")),
                      (dict(num_beams=2, frequency_penalty=0.5), ("num_beams", "frequency_penalty")),
                      (dict(num_beams=2, return_logprobs=True), ("num_beams", "return_logprobs")),
                      (dict(draft_tokens=1, presence_penalty=0.5), ("draft_tokens", "presence_penalty")),
                      (dict(draft_tokens=1, return_logprobs=True), ("draft_tokens", "return_logprobs"))):
        with pytest.raises(LlxError) as e:
            model.generate(prompt, N, **kw)
        assert all(n in str(e.value) for n in names), (kw, str(e.value))
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=math.inf), dict(presence_penalty=math.nan), dict(frequency_penalty=math.nan)):
        with pytest.raises(LlxError):
            model.generate(prompt, N, **bad)


@pytest.mark.parametrize("B", [1, 3])
def test_no_host_sync_inside_a_token(cuda, monkeypatch, B):
    model = _model(B, cuda)
    prompt, lens = (_prompt(cuda), None) if B == 1 else _prompts(B, cuda)
    kw = dict(prompt_lens=lens, return_logprobs=True, **PC.PENALTIES)
    want = model.generate(prompt, N, **kw, **SAMPLED)
    unused = next(t for t in range(V) if t not in set(model.generate(prompt, N, prompt_lens=lens, **PC.PENALTIES).flatten().tolist()))
    calls = []
    item, sync = torch.Tensor.item, torch.cuda.synchronize
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (calls.append("item"), item(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (calls.append("sync"), sync(*a, **k))[1])
    out = model.generate(prompt, N, **kw, **SAMPLED)
    assert calls == []  # prefill and the seeding of the count table included
    model.generate(prompt, N, eos_id=unused, check_every=4, **kw)
    assert len(calls) <= math.ceil(N / 4), calls
    monkeypatch.undo()
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1]) and out[0].shape == (B, N)
