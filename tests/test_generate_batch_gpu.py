"""GPU: generate() for a batch of right-padded prompts on the tiny model - token for token against a hand-written loop, the cache rows
it leaves, row isolation, per-row eos, argument errors and the absence of host syncs inside a token."""
import math

import pytest
import torch

from oracle import ref as O
from tests.util import bf16_params, build_model

pytestmark = pytest.mark.gpu
P, N = 40, 12
LENS = (40, 17, 29)
SAMPLED = dict(temperature=0.8, top_p=0.9, seed=3)
_MODELS: dict = {}


def _model(B, cuda):
    if B not in _MODELS:
        pb, _ = bf16_params(O.init_params(O.TINY))
        model = build_model(O.TINY, pb, "cpu")
        model.build_cache(inference=True, batch_size=B)
        _MODELS[B] = model.to(cuda).eval()
    return _MODELS[B]


def _prompts(B, cuda):
    return O.randint("generate_batch_prompts", (16, P), 0, O.TINY.vocab_size)[:B].to(cuda), [LENS[b % 3] for b in range(B)]


def _hand_loop(model, prompt, lens, n, sampling):
    """The loop a user writes: prefill once, then per token one model(tok [B, 1], input_pos=pos[:, None]) call and one sampler call on
    the [B, V] logits with the per-row counters pos."""
    from llx import kernels as K
    from llx.generate import prefill

    dev, B = prompt.device, prompt.shape[0]
    pos = torch.tensor(lens, device=dev) - 1
    with torch.no_grad():
        logits = prefill(model, prompt, lens)[:, 0]
        toks = []
        for k in range(n):
            t = K.sample(logits, pos=pos + k, **sampling)
            toks.append(t.clone())
            if k == n - 1:
                break
            logits = model(t.view(B, 1), input_pos=(pos + k + 1)[:, None])[:, 0]
    return torch.stack(toks, 1)


def _caches(model, lens, n):
    """The cache rows a run leaves that belong to its sequences: positions 0 .. len_b + n - 2 of row b, per layer."""
    out = []
    for l in model.layers:
        c = l.attention.kv_cache
        out.append([(c.k_cache[b, :, : lens[b] + n - 1].clone(), c.v_cache[b, :, : lens[b] + n - 1].clone()) for b in range(len(lens))])
    return out


def _same_caches(a, b):
    return all(torch.equal(k0, k1) and torch.equal(v0, v1) for la, lb in zip(a, b) for (k0, v0), (k1, v1) in zip(la, lb))


@pytest.mark.parametrize("B", [3, 16])
def test_generate_equals_the_hand_loop(cuda, B):
    model = _model(B, cuda)
    prompt, lens = _prompts(B, cuda)
    greedy = dict(temperature=0.0)
    want = _hand_loop(model, prompt, lens, N, greedy)
    cache_want = _caches(model, lens, N)
    got = model.generate(prompt, N, prompt_lens=lens)
    assert got.shape == (B, N) and got.dtype is torch.int64 and got.device == prompt.device
    assert torch.equal(got, want)
    assert _same_caches(cache_want, _caches(model, lens, N))
    assert got.unique().numel() > 1

    want_s = _hand_loop(model, prompt, lens, N, SAMPLED)
    cache_want = _caches(model, lens, N)
    got_s = model.generate(prompt, N, prompt_lens=torch.tensor(lens), **SAMPLED)
    assert torch.equal(got_s, want_s) and not torch.equal(got_s, got)
    assert _same_caches(cache_want, _caches(model, lens, N))
    rope = model.rope
    for chunk in (None, 16):
        for every in (1, 16):
            assert torch.equal(model.generate(prompt, N, prompt_lens=lens, prefill_chunk=chunk, check_every=every, **SAMPLED), got_s), (chunk, every)
            assert _same_caches(cache_want, _caches(model, lens, N)), (chunk, every)
            assert model.rope is rope
            assert torch.equal(model.generate(prompt, N, prompt_lens=lens, prefill_chunk=chunk, check_every=every), got), (chunk, every)


def _close(a, b, rel, name):
    scale = b.abs().max().item()
    err = (a - b).abs().max().item()
    assert err <= rel * scale + 1e-6, f"{name}: max err {err:.4e} vs scale {scale:.4e} (allowed {rel * scale:.4e})"


@pytest.mark.parametrize("lens", [[40, 17, 29], [17, 29, 29]])
def test_prefill_against_the_plain_forward(cuda, lens):
    """prefill() - which the hand loop above shares with generate() - against the call it stands for, on its own: the logits it returns
    for row b are those of model(prompt, input_pos=arange(P))[b, len_b - 1] (0.03, the logits bar: the head runs on other rows
    through another kernel), whole and in chunks of 16 (the last row of a sequence then lies in the first, second or third chunk),
    and the cache rows 0 .. len_b - 1 it leaves are the same bits.  [17, 29, 29]: no row is P long, the all-pad columns are not run."""
    from llx.generate import prefill

    B = 3
    model = _model(B, cuda)
    prompt, _ = _prompts(B, cuda)
    with torch.no_grad():
        full = model(prompt, input_pos=torch.arange(P, device=cuda))  # [B, P, V]
    want = torch.stack([full[b, lens[b] - 1] for b in range(B)]).float().cpu()
    cache_want = _caches(model, lens, 1)  # rows 0 .. len_b - 1
    rope = model.rope
    for chunk in (None, 16):
        for layer in model.layers:
            layer.attention.kv_cache.k_cache.zero_()
            layer.attention.kv_cache.v_cache.zero_()
        got = prefill(model, prompt, lens, chunk)
        assert got.shape == (B, 1, O.TINY.vocab_size) and model.rope is rope
        for b in range(B):
            _close(got[b, 0].float().cpu(), want[b], 0.03, f"prefill logits, row {b}, chunk {chunk}")
        assert _same_caches(cache_want, _caches(model, lens, 1)), chunk


def test_rows_do_not_see_each_other(cuda):
    """Row 0's prompt fixed, every other row's tokens replaced at unchanged lengths (so the mask extent and every split are the same):
    row 0's greedy output keeps its bits."""
    B = 3
    model = _model(B, cuda)
    prompt, lens = _prompts(B, cuda)
    a = model.generate(prompt, N, prompt_lens=lens)
    other = prompt.clone()
    other[1:] = O.randint("generate_batch_other", (B - 1, P), 0, O.TINY.vocab_size).to(cuda)
    b = model.generate(other, N, prompt_lens=lens)
    assert torch.equal(a[0], b[0]) and not torch.equal(a[1:], b[1:])


# Per-row eos.  The greedy run of the B = 3 prompts above (lengths 40 / 17 / 29) on an MI355X gives
#   row 0: 703 279 356 126 126  15 427 153 730 418 907 854
#   row 1: 249 808 975 461 975 928  96 249 556  96 556 373
#   row 2: 774 170 372 117 112 211 112 576 372 644 153 644
# so eos_id = 153 stops row 0 after 8 tokens, row 2 after 11, and never stops row 1.
EOS_ID, EOS_FIRST = 153, [7, None, 10]


def test_per_row_eos(cuda):
    """Each row equals its greedy prefix up to and including its first eos_id, then eos_id padding; T is the longest row; the same at
    every check_every.  Two rows stop at different steps and one never stops (the choice above, re-checked against the greedy run)."""
    B = 3
    model = _model(B, cuda)
    prompt, lens = _prompts(B, cuda)
    greedy = model.generate(prompt, N, prompt_lens=lens).tolist()
    choice = EOS_ID
    assert [r.index(choice) if choice in r else None for r in greedy] == EOS_FIRST, greedy
    f = EOS_FIRST
    want = [r[: f[b] + 1] + [choice] * (N - f[b] - 1) if f[b] is not None else r for b, r in enumerate(greedy)]
    for every in (1, 5, 16):
        got = model.generate(prompt, N, prompt_lens=lens, eos_id=choice, check_every=every)
        assert got.shape == (B, N) and got.tolist() == want, every  # a row that never stops keeps T = N
    # all rows stop: T is the longest row
    rows2 = [b for b in range(B) if f[b] is not None]
    sub = prompt.clone()
    spare = next(b for b in range(B) if f[b] is None)
    sub[spare], lens2 = prompt[rows2[0]], list(lens)
    lens2[spare] = lens[rows2[0]]
    g2 = model.generate(sub, N, prompt_lens=lens2).tolist()
    f2 = [r.index(choice) if choice in r else None for r in g2]
    assert all(v is not None for v in f2)  # (a row's greedy tokens depend on its own prompt only)
    T = max(f2) + 1
    for every in (1, 5, 16):
        got = model.generate(sub, N, prompt_lens=lens2, eos_id=choice, check_every=every)
        assert got.shape == (B, T), every
        assert got.tolist() == [r[: f2[b] + 1] + [choice] * (T - f2[b] - 1) for b, r in enumerate(g2)], every


@pytest.mark.parametrize("every", [1, 16])
def test_no_host_sync_inside_a_token(cuda, monkeypatch, every):
    B = 3
    model = _model(B, cuda)
    prompt, lens = _prompts(B, cuda)
    greedy = model.generate(prompt, N, prompt_lens=lens)
    unused = next(t for t in range(O.TINY.vocab_size) if t not in set(greedy.flatten().tolist()))
    calls = []
    item, sync = torch.Tensor.item, torch.cuda.synchronize
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (calls.append("item"), item(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (calls.append("sync"), sync(*a, **k))[1])
    out = model.generate(prompt, N, prompt_lens=lens, check_every=every, **SAMPLED)
    assert calls == []  # prefill included
    out_eos = model.generate(prompt, N, prompt_lens=lens, eos_id=unused, check_every=every)
    assert len(calls) <= math.ceil(N / every), calls
    monkeypatch.undo()
    assert out.shape == (B, N) and torch.equal(out_eos, greedy)


def test_errors_before_any_launch(cuda):
    from llx._lib import LlxError

    B = 3
    model = _model(B, cuda)
    prompt, lens = _prompts(B, cuda)
    with pytest.raises(LlxError, match="batch_size=2"):
        model.generate(prompt[:2], N, prompt_lens=lens[:2])
    for bad in ([40, 17], [40, 17, 29, 5], [40, 0, 29], [40, 17, P + 1], [40.0, 17, 29]):
        with pytest.raises(LlxError, match="prompt_lens"):
            model.generate(prompt, N, prompt_lens=bad)
    long = torch.zeros(B, O.TINY.max_seq_len - N + 1, dtype=torch.int64, device=cuda)
    with pytest.raises(LlxError, match="max_seq_len"):
        model.generate(long, N)
    model.generate(long, N, prompt_lens=[5, 6, O.TINY.max_seq_len - N])  # the budget counts the longest REAL prompt
    wide = torch.zeros(B, O.TINY.max_seq_len + 8, dtype=torch.int64, device=cuda)  # padding may run past max_seq_len, prompts may not
    with pytest.raises(LlxError, match="max_seq_len"):
        model.generate(wide, N)
    assert model.generate(wide, N, prompt_lens=[5, 6, 7]).shape == (B, N)
    with pytest.raises(LlxError, match="max_seq_len"):
        model.generate(long, N, prompt_lens=[5, 6, O.TINY.max_seq_len - N + 1])
