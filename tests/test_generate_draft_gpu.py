"""GPU: generate(draft_tokens=k) on the tiny model - bit for bit against a host-written speculative loop of the same model calls,
against the plain greedy generate() on three prompts, at the cache bound, and without a host read inside a step."""
import math

import pytest
import torch

from oracle import ref as O
from tests.util import bf16_params, build_model

pytestmark = pytest.mark.gpu
P, N, G = 40, 48, 3
_MODELS: dict = {}


def _model(kind, cuda, max_seq_len=None):
    key = (kind, max_seq_len)
    if key not in _MODELS:
        cfg = O.TINY if max_seq_len is None else O.TINY._replace(max_seq_len=max_seq_len)
        p = O.init_params(cfg)
        if kind == "int8_lora":
            p.update(O.init_lora(cfg, 8))
        pb, _ = bf16_params(p)
        if kind == "int8_lora":
            model = build_model(cfg, pb, "cpu", lora_rank=8, quantize="int8", quantize_kwargs=dict(dynamic_int8_act=False))
        else:
            model = build_model(cfg, pb, "cpu")
        model.build_cache(inference=True)
        _MODELS[key] = model.to(cuda).eval()
    return _MODELS[key]


def _prompt(cuda, name="generate_prompt"):
    return O.randint(name, (1, P), 0, O.TINY.vocab_size).to(cuda)


def _caches(model):
    return [(l.attention.kv_cache.k_cache[:, :, : P + N - 1].clone(), l.attention.kv_cache.v_cache[:, :, : P + N - 1].clone()) for l in model.layers]


def _argmax(row):
    x = row.float()
    return int((x == x.max()).nonzero()[0])  # lowest index among ties


def _plain_rows(model, prompt, tokens):
    """The one-row path: the logits row behind each of `tokens` and the one that follows them, prefill in one call, then a call per token."""
    dev = prompt.device
    with torch.no_grad():
        rows = [model(prompt, input_pos=torch.arange(P, device=dev))[0, -1].float()]
        for i, t in enumerate(tokens):
            rows.append(model(torch.tensor([[t]], device=dev), input_pos=torch.tensor([P + i], device=dev))[0, 0].float())
    return rows


def _spec_hand_loop(model, prompt, n, k, g=G, eos=None):
    """The speculative loop written on the host: the same model calls as generate(draft_tokens=k), everything else in Python.
    -> (tokens, steps, for each token the logits row it is the argmax of, for each token whether it is a confirmed draft token)."""
    from llx.generate import decode_rope
    from llx.sampling import lookup_accept, lookup_draft

    dev = prompt.device
    with torch.no_grad():
        last = model(prompt, input_pos=torch.arange(P, device=dev))[0, -1]
        seq = prompt[0].tolist()
        seq.append(_argmax(last))
        rows, drafted, steps, fin = [last.float()], [False], 1, seq[-1] == eos
        with decode_rope(model):
            while not fin and len(seq) < P + n:
                L = len(seq)
                fed = [seq[-1]] + lookup_draft(seq, g, k)
                logits = model(torch.tensor([fed], device=dev), input_pos=torch.arange(L - 1, L + k, device=dev))[0]
                emitted, fin = lookup_accept(fed, [_argmax(r) for r in logits], k, eos, P + n - L)
                seq += emitted
                rows += [logits[i].float() for i in range(len(emitted))]
                drafted += [i < k and fed[1 + i] == emitted[i] for i in range(len(emitted))]  # (the output stops at the first mismatch)
                steps += 1
    return seq[P:], steps, rows, drafted


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("kind", ["bf16", "int8_lora"])
def test_generate_equals_the_speculative_hand_loop(cuda, kind, k):
    from llx.generate import generate

    model, prompt = _model(kind, cuda), _prompt(cuda)
    rope = model.rope
    want, steps, _, _ = _spec_hand_loop(model, prompt, N, k)
    assert len(want) == N and model.rope is rope
    cache_want = _caches(model)
    stats = {}
    got = model.generate(prompt, N, draft_tokens=k, draft_ngram=G, stats=stats)
    assert got.shape == (1, N) and got.dtype is torch.int64 and got.device == prompt.device
    assert got[0].tolist() == want
    for (k0, v0), (k1, v1) in zip(cache_want, _caches(model)):  # cache rows 0 .. P + N - 2: the frozen steps rewrote what was there
        assert torch.equal(k0, k1) and torch.equal(v0, v1)
    assert stats["draft_tokens"] == k and stats["tokens"] == N and stats["steps"] == steps and stats["accepted"] == N - steps
    assert stats["steps"] < stats["tokens"]  # a draft was accepted
    assert model.rope is rope
    unused = next(t for t in range(O.TINY.vocab_size) if t not in want)
    eos = want[9]
    want_eos = want[: want.index(eos) + 1]
    assert _spec_hand_loop(model, prompt, N, k, eos=eos)[0] == want_eos
    for chunk in (None, 16):
        for every in (1, 5, 16):
            assert generate(model, prompt, N, draft_tokens=k, prefill_chunk=chunk, check_every=every)[0].tolist() == want, (chunk, every)
            stats = {}
            assert generate(model, prompt, N, draft_tokens=k, prefill_chunk=chunk, check_every=every, eos_id=eos, stats=stats)[0].tolist() == want_eos
            assert stats["tokens"] == len(want_eos) and bool(stats["state"]["finished"].item())
            assert generate(model, prompt, N, draft_tokens=k, prefill_chunk=chunk, check_every=every, eos_id=unused)[0].tolist() == want
            assert model.rope is rope
    # the default keyword is the plain loop
    assert model.generate(prompt, N, draft_tokens=0)[0].tolist() == model.generate(prompt, N)[0].tolist()


def test_decode_rope_restores_the_table_on_an_exception(cuda):
    from llx.generate import decode_rope

    model = _model("bf16", cuda)
    rope = model.rope
    with pytest.raises(RuntimeError, match="inside"):
        with decode_rope(model):
            assert tuple(model.rope.shape) == (4, 64, 2) and model.rope.dtype is torch.float32 and model.rope.is_contiguous()
            assert all(torch.equal(model.rope[i], rope[0].float()) for i in range(4))
            raise RuntimeError("inside")
    assert model.rope is rope


@pytest.mark.parametrize("kind", ["bf16", "int8_lora"])
def test_drafting_gives_the_plain_greedy_tokens(cuda, kind):
    """generate(draft_tokens=3) against the plain loop on three prompts.  The logits of a row are not claimed to be bit-identical between
    a one-row and a four-row step, so the two outputs must agree up to the first index d where they differ, if any; there each path's
    token must be the argmax of its own logits row on the common prefix, and the two rows must agree to the project's bar between two
    decode paths, max |r1 - rM| <= 0.03 max |r1|: a divergence passes only as a near-tie between paths that agree.  So that this rule
    cannot hide a failure, a draft token must have been accepted before d (or before the end) on at least two of the three prompts."""
    model = _model(kind, cuda)
    k, conclusive = 3, 0
    for name in ("generate_prompt", "spec_prompt_a", "spec_prompt_b"):
        prompt = _prompt(cuda, name)
        plain = model.generate(prompt, N)[0].tolist()
        stats = {}
        got = model.generate(prompt, N, draft_tokens=k, draft_ngram=G, stats=stats)[0].tolist()
        assert len(plain) == len(got) == N
        d = next((i for i in range(N) if plain[i] != got[i]), N)
        hand, _, rows, drafted = _spec_hand_loop(model, prompt, N, k)
        assert hand == got, name
        print(f"[{kind} {name}] steps {stats['steps']} for {N} tokens, accepted {stats['accepted']}, first difference at {d if d < N else None}, "
              f"first accepted draft token at {drafted.index(True) if True in drafted else None}")
        conclusive += any(drafted[:d])
        if d < N:
            r1, rM = _plain_rows(model, prompt, plain[:d])[d], rows[d]
            err, scale = (r1 - rM).abs().max().item(), r1.abs().max().item()
            print(f"[{kind} {name}] at {d}: one-row token {plain[d]}, four-row token {got[d]}, max |r1 - rM| {err:.4e} against max |r1| {scale:.4e}")
            assert _argmax(r1) == plain[d] and _argmax(rM) == got[d], (name, d)
            assert err <= 0.03 * scale, (name, d, err, scale)
    assert conclusive >= 2, f"inconclusive: a draft was accepted before the first difference on {conclusive} of 3 prompts only"


@pytest.mark.parametrize("kind", ["bf16", "int8_lora"])
def test_the_last_step_stays_inside_the_cache(cuda, kind):
    """P + n + k == max_seq_len exactly: the positions of every step, the frozen ones after the end included, stay inside the cache."""
    from llx._lib import LlxError

    S, k = 128, 3
    model, prompt = _model(kind, cuda, max_seq_len=S), _prompt(cuda)
    n = S - P - k
    greedy = _spec_hand_loop(model, prompt, n, k)[0]
    with pytest.raises(LlxError, match="max_seq_len"):
        model.generate(prompt, n + 1, draft_tokens=k)
    stats = {}
    assert model.generate(prompt, n, draft_tokens=k, stats=stats)[0].tolist() == greedy  # runs to the last position
    st = stats["state"]
    assert int(st["len"]) == P + n == S - k and int(st["step_pos"].max()) == S - 1 and int(st["step_pos"].min()) == S - 1 - k
    eos = greedy[9]
    first = greedy.index(eos)
    stats = {}
    got = model.generate(prompt, n, draft_tokens=k, eos_id=eos, check_every=16, stats=stats)  # frozen steps until the next look
    assert got[0].tolist() == greedy[: first + 1]
    st = stats["state"]
    assert int(st["step_pos"].max()) < S and int(st["len"]) == P + first + 1 and int(st["step_pos"].max()) == P + first + k
    assert stats["tokens"] == first + 1
    assert got[0].tolist() == model.generate(prompt, n, eos_id=eos)[0].tolist()  # the plain loop's result


@pytest.mark.parametrize("every", [1, 16])
def test_no_host_sync_inside_a_step(cuda, monkeypatch, every):
    model, prompt = _model("bf16", cuda), _prompt(cuda)
    want = model.generate(prompt, N, draft_tokens=3)[0].tolist()
    unused = next(t for t in range(O.TINY.vocab_size) if t not in want)
    calls = []
    item, tolist, sync = torch.Tensor.item, torch.Tensor.tolist, torch.cuda.synchronize
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (calls.append("item"), item(self))[1])
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (calls.append("tolist"), tolist(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (calls.append("sync"), sync(*a, **k))[1])
    stats = {}
    out = model.generate(prompt, N, draft_tokens=3, check_every=every, stats=stats)
    looks = len(calls)
    out_eos = model.generate(prompt, N, draft_tokens=3, eos_id=unused, check_every=every)
    monkeypatch.undo()
    # the host looks once every `every` steps and at the end; the statistics come from the last look
    assert set(calls) <= {"tolist"} and looks <= math.ceil(stats["steps"] / every) + 1 and looks <= math.ceil(N / every), calls
    assert len(calls) <= 2 * looks
    assert out[0].tolist() == want and out_eos[0].tolist() == want
