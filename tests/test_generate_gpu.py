"""GPU: llx.generate.generate / Llama.generate on the tiny model - token for token against a hand-written loop of model(...) + sampler,
the KV cache it leaves, eos handling, argument errors and the absence of host syncs inside a token."""
import math

import pytest
import torch

from oracle import ref as O
from tests.util import bf16_params, build_model

pytestmark = pytest.mark.gpu
P, N = 40, 24
SAMPLED = dict(temperature=0.8, top_p=0.9, seed=3)
_MODELS: dict = {}


def _model(kind, cuda):
    if kind not in _MODELS:
        cfg = O.TINY
        p = O.init_params(cfg)
        if kind == "int8_lora":
            p.update(O.init_lora(cfg, 8))
        pb, _ = bf16_params(p)
        if kind == "int8_lora":
            model = build_model(cfg, pb, "cpu", lora_rank=8, quantize="int8", quantize_kwargs=dict(dynamic_int8_act=False))
        else:
            model = build_model(cfg, pb, "cpu")
        model.build_cache(inference=True)
        _MODELS[kind] = model.to(cuda).eval()
    return _MODELS[kind]


def _prompt(cuda):
    return O.randint("generate_prompt", (1, P), 0, O.TINY.vocab_size).to(cuda)


def _greedy(logits_row, _pos):
    x = logits_row.float()
    return (x[0] == x[0].max()).nonzero()[0]  # lowest index among ties


def _hand_loop(model, prompt, n, pick):
    """The loop a user writes: prefill in one call, then one model(...) call per token; pick(logits [1, V], position of that row) -> [1]."""
    dev = prompt.device
    with torch.no_grad():
        last = model(prompt, input_pos=torch.arange(P, device=dev))[0, -1:]
        toks = []
        for k in range(n):
            t = pick(last, P - 1 + k)
            toks.append(t.view(1))
            if k == n - 1:
                break
            last = model(t.view(1, 1), input_pos=torch.tensor([P + k], device=dev))[0]
    return torch.cat(toks)[None]


def _caches(model):
    return [(l.attention.kv_cache.k_cache[:, :, : P + N - 1].clone(), l.attention.kv_cache.v_cache[:, :, : P + N - 1].clone()) for l in model.layers]


@pytest.mark.parametrize("kind", ["bf16", "int8_lora"])
def test_generate_equals_the_hand_loop(cuda, kind):
    from llx import kernels as K

    model, prompt = _model(kind, cuda), _prompt(cuda)
    want = _hand_loop(model, prompt, N, _greedy)
    cache_want = _caches(model)
    got = model.generate(prompt, N)
    assert got.shape == (1, N) and got.dtype is torch.int64 and got.device == prompt.device
    assert torch.equal(got, want)
    for (k0, v0), (k1, v1) in zip(cache_want, _caches(model)):  # cache rows 0 .. P+N-2
        assert torch.equal(k0, k1) and torch.equal(v0, v1)
    assert len(set(got[0].tolist())) > 1

    def pick(last, pos):
        return K.sample(last, pos=torch.tensor([pos], device=cuda), **SAMPLED)

    want_s = _hand_loop(model, prompt, N, pick)
    cache_want = _caches(model)
    from llx.generate import generate

    got_s = generate(model, prompt, N, **SAMPLED)
    assert torch.equal(got_s, want_s)
    for (k0, v0), (k1, v1) in zip(cache_want, _caches(model)):
        assert torch.equal(k0, k1) and torch.equal(v0, v1)
    assert not torch.equal(got_s, got)  # the sampled run is not the greedy one
    rope = model.rope
    for chunk in (None, 16):
        for every in (1, 16):
            assert torch.equal(model.generate(prompt, N, prefill_chunk=chunk, check_every=every, **SAMPLED), got_s), (chunk, every)
            for (k0, v0), (k1, v1) in zip(cache_want, _caches(model)):  # the chunked prefill leaves the same cache rows, bit for bit
                assert torch.equal(k0, k1) and torch.equal(v0, v1), (chunk, every)
            assert model.rope is rope  # the table a chunk ran with is gone again
            assert torch.equal(model.generate(prompt, N, prefill_chunk=chunk, check_every=every, eos_id=None), got), (chunk, every)
    assert not torch.equal(model.generate(prompt, N, **{**SAMPLED, "seed": 4}), got_s)


@pytest.mark.parametrize("kind", ["bf16", "int8_lora"])
def test_eos_cuts_the_output(cuda, kind):
    model, prompt = _model(kind, cuda), _prompt(cuda)
    greedy = model.generate(prompt, N)[0].tolist()
    eos = greedy[9]
    first = greedy.index(eos)
    for every in (1, 16, 5):
        got = model.generate(prompt, N, eos_id=eos, check_every=every)
        assert got[0].tolist() == greedy[: first + 1], every
    # an eos that never comes leaves the full length
    unused = next(t for t in range(O.TINY.vocab_size) if t not in greedy)
    assert model.generate(prompt, N, eos_id=unused)[0].tolist() == greedy


def test_errors_before_any_launch(cuda):
    from llx._lib import LlxError
    from modelling import Llama
    from tests.util import to_model_config

    model, prompt = _model("bf16", cuda), _prompt(cuda)
    cfg = O.TINY
    with pytest.raises(LlxError, match="max_seq_len"):
        model.generate(torch.zeros(1, cfg.max_seq_len - N + 1, dtype=torch.int64, device=cuda), N)
    model.train()
    try:
        with pytest.raises(LlxError, match="eval"):
            model.generate(prompt, N)
    finally:
        model.eval()
    bare = Llama(to_model_config(cfg._replace(num_layers=1))).bfloat16()
    bare.build_cache()  # no inference cache
    bare = bare.to(cuda).eval()
    with pytest.raises(LlxError, match="build_cache"):
        bare.generate(prompt, N)
    for bad in (dict(temperature=-1.0), dict(top_p=0.0), dict(top_k=-1), dict(check_every=0), dict(prefill_chunk=0), dict(eos_id=cfg.vocab_size)):
        with pytest.raises(LlxError):
            model.generate(prompt, N, **bad)
    with pytest.raises(LlxError):
        model.generate(prompt.cpu(), N)
    with pytest.raises(LlxError):
        model.generate(prompt[0], N)
    with pytest.raises(LlxError):
        model.generate(prompt, 0)


@pytest.mark.parametrize("every", [1, 16])
def test_no_host_sync_inside_a_token(cuda, monkeypatch, every):
    model, prompt = _model("bf16", cuda), _prompt(cuda)
    greedy = model.generate(prompt, N)[0].tolist()
    unused = next(t for t in range(O.TINY.vocab_size) if t not in greedy)
    calls = []
    item, sync = torch.Tensor.item, torch.cuda.synchronize
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (calls.append("item"), item(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (calls.append("sync"), sync(*a, **k))[1])
    out = model.generate(prompt, N, check_every=every, **SAMPLED)
    assert calls == []  # prefill included
    out_eos = model.generate(prompt, N, eos_id=unused, check_every=every)
    assert len(calls) <= math.ceil(N / every), calls
    monkeypatch.undo()
    assert out.shape == (1, N) and out_eos[0].tolist() == greedy
