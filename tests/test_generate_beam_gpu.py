"""GPU: generate(num_beams=W) on the tiny model, token for token against a host loop that makes the same model calls, applies the
reference functions (llx.sampling.beam_step) and moves the cache slots with index_select.  The model's logits are the same bits on both
sides, so only the scoring arithmetic differs; the prompts are seeded so that every decision keeps MARGIN, which is asserted here."""
import pytest
import torch

from oracle import ref as O
from tests.beam_cases import MARGIN, SCORE_TOL
from tests.util import bf16_params, build_model

pytestmark = pytest.mark.gpu
P, N = 24, 8
HEAD_GAIN = 16.0  # the tiny model's random head gives logits of std ~0.5: next to flat.  x16 spreads the candidates (|z| stays < 64)
DYN = dict(quantize="int8", quantize_kwargs=dict(dynamic_int8_act=True))
SEEDS = {("bf16", 2): 2, ("bf16", 4): 5, ("int8", 2): 6, ("int8", 4): 0}  # prompt seeds that keep MARGIN at every decision
_MODELS: dict = {}


def _model(kind, B, cuda):
    if (kind, B) not in _MODELS:
        pb, _ = bf16_params(O.init_params(O.TINY))
        model = build_model(O.TINY, pb, "cpu", **(DYN if kind == "int8" else {}))
        with torch.no_grad():
            model.output.weight.mul_(HEAD_GAIN)
        if B:  # (B = 0: no KV cache - the model that scores with token_logprobs)
            model.build_cache(inference=True, batch_size=B)
        _MODELS[kind, B] = model.to(cuda).eval()
    return _MODELS[kind, B]


def _prompt(kind, W, cuda, seed=None):
    seed = SEEDS[kind, W] if seed is None else seed
    return O.randint(f"beam_prompt_{kind}_{W}", (1, P), 0, O.TINY.vocab_size, seed=1234 + seed).to(cuda)


def _host_beam(model, prompt, n, W, eos_id, lp, margins):
    """The search as a user would write it on the host: the same prefill and the same model(tok [W, 1], input_pos=[pos]) calls as
    generate(), the reference rule on the logits read back, the cache slots moved with index_select."""
    from llx import sampling as S
    from llx.generate import prefill

    caches = [c for layer in model.layers for c in (layer.attention.kv_cache.k_cache, layer.attention.kv_cache.v_cache)]
    st = S.beam_state(W)
    with torch.no_grad():
        logits = prefill(model, prompt.expand(W, -1).contiguous())[:, 0]
        for k in range(1, n + 1):
            parent = S.beam_step(st, logits.double().tolist(), W, max_new_tokens=n, eos_id=eos_id, length_penalty=lp, margins=margins)
            if k > 1:
                idx = torch.tensor(parent, device=prompt.device)
                for c in caches:
                    c[:W, :, : P + k - 1] = c[:, :, : P + k - 1].index_select(0, idx)
            if st["done"]:
                break
            tok = torch.tensor([[h[-1]] for h in st["hist"]], device=prompt.device)
            logits = model(tok, input_pos=torch.arange(P + k - 1, P + k, device=prompt.device))[:, 0]
    return S.beam_ranked(st, margins)


def _check_run(model, prompt, W, eos_id, lp, want, check_every):
    stats = {}
    got = model.generate(prompt, N, num_beams=W, eos_id=eos_id, length_penalty=lp, check_every=check_every, stats=stats)
    assert got.dtype is torch.int64 and got.device == prompt.device and got.shape == (1, len(want[0][0]))
    assert got[0].tolist() == want[0][0], (eos_id, check_every)
    beams = stats["beams"]
    assert [t for t, _ in beams] == [t for t, _ in want], (eos_id, check_every)
    scores = [f for _, f in beams]
    assert scores == sorted(scores, reverse=True)  # rank order
    assert max(abs(a - b) for a, (_, b) in zip(scores, want)) <= SCORE_TOL * N
    assert stats["num_beams"] == W and stats["tokens"] == got.shape[1]
    return got


@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("kind", ["bf16", "int8"])
def test_generate_beams_equal_the_host_loop(cuda, kind, W):
    from llx import decode as D

    model = _model(kind, W, cuda)
    prompt = _prompt(kind, W, cuda)
    # the beams are on the batched weight stream: the first decode step's layers and head pass the fast path's own test
    x = torch.empty(W, 1, O.TINY.embed_dim, device=cuda, dtype=torch.bfloat16)
    mask = model.causal_mask[None, None, torch.arange(P, P + 1, device=cuda)]
    assert all(D.layer_ok(layer, x, mask) for layer in model.layers) and D.head_ok(model, x)

    margins: list = []
    free = _host_beam(model, prompt, N, W, None, 1.0, margins)
    assert len(free) == W and all(len(t) == N for t, _ in free)
    eos_id = free[0][0][2]  # the best free hypothesis's third token ends hypotheses in the second run
    ended = _host_beam(model, prompt, N, W, eos_id, 1.0, margins)
    assert any(t[-1] == eos_id for t, _ in ended)
    print(f"{kind} W={W}: min margin {min(margins):.4f} over {len(margins)} decisions")
    assert min(margins) >= MARGIN, min(margins)
    for eos, want in ((None, free), (eos_id, ended)):
        a = _check_run(model, prompt, W, eos, 1.0, want, 1)
        b = _check_run(model, prompt, W, eos, 1.0, want, 16)
        assert torch.equal(a, b)
        if eos is not None and want[0][0][-1] == eos:
            assert a[0, -1].item() == eos and eos not in a[0, :-1].tolist()  # ends at its eos, inclusive


def test_beams_are_not_below_greedy(cuda):
    """length_penalty 0 ranks by the total log-probability: the hypothesis returned is not below the greedy continuation, scored by
    token_logprobs, minus the bar of SCORE_TOL per step."""
    W = 4
    model, single = _model("bf16", W, cuda), _model("bf16", 1, cuda)
    prompt = _prompt("bf16", W, cuda)
    greedy = single.generate(prompt, N)
    stats = {}
    best = model.generate(prompt, N, num_beams=W, length_penalty=0.0, stats=stats)
    seq = torch.cat((prompt, greedy), 1)
    labels = torch.full_like(seq, -100)
    labels[:, P - 1 : -1] = seq[:, P:]
    with torch.no_grad():
        total = _model("bf16", 0, cuda).token_logprobs(seq, labels).sum().item()
    score = stats["beams"][0][1]
    print(f"beam {score:.4f} ({best[0].tolist()}) greedy {total:.4f} ({greedy[0].tolist()})")
    assert score >= total - SCORE_TOL * N, (score, total)


def test_one_beam_is_the_greedy_loop(cuda):
    """num_beams=1 is the loop as it was: the tokens of a hand loop of model calls and greedy sampler launches."""
    from llx import kernels as K

    model = _model("bf16", 1, cuda)
    prompt = _prompt("bf16", 2, cuda)
    pos = torch.tensor([P - 1], device=cuda)
    toks = []
    with torch.no_grad():
        logits = model(prompt, input_pos=torch.arange(P, device=cuda))[0, -1:]
        for k in range(N):
            t = K.sample(logits, temperature=0.0, pos=pos + k)
            toks.append(t.clone())
            logits = model(t.view(1, 1), input_pos=pos + k + 1)[0]
    want = torch.stack(toks, 1)
    assert torch.equal(model.generate(prompt, N), want)
    assert torch.equal(model.generate(prompt, N, num_beams=1, length_penalty=2.0), want)
