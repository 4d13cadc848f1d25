"""GPU: generate() for the audio model (LlamaAudio.generate(audio, prompt, n)) on the tiny model - greedy, a batch with prompt_lens and
beams, token for token against hand loops of model(audio, ...) / model(None, ...) calls, and the text-only call of an audio model."""
import pytest
import torch

from oracle import ref as O
from tests.beam_cases import MARGIN, SCORE_TOL
from tests.util import bf16_params, build_model

pytestmark = pytest.mark.gpu
P, N, SAMPLES = 20, 8, 3200  # 3200 samples = 20 frames -> 10 audio positions
LENS = (20, 9, 14)
HEAD_GAIN = 16.0  # as in test_generate_beam_gpu.py: spreads the candidates of the tiny model's flat head
BEAM_SEED = 5  # prompt seed that keeps MARGIN at every decision of the beam test
_MODELS: dict = {}


def _model(B, cuda):
    if B not in _MODELS:
        pb, _ = bf16_params(O.init_params(O.TINY, audio=True))
        model = build_model(O.TINY, pb, "cpu", audio=True)
        with torch.no_grad():
            model.output.weight.mul_(HEAD_GAIN)
        model.build_cache(inference=True, batch_size=B)
        _MODELS[B] = model.to(cuda).eval()
    return _MODELS[B]


def _inputs(B, cuda, seed=0):
    audio = O.uniform("generate_audio_clips", (3, SAMPLES), -0.1, 0.1)[:B]
    return audio.to(cuda), O.randint("generate_audio_prompts", (3, P), 0, O.TINY.vocab_size, seed=1234 + seed)[:B].to(cuda)


def _hand_loop(model, audio, prompt, lens, n):
    """Prefill the clip and the prompt as one call, then one text-only call and one greedy sampler launch per token."""
    from llx import kernels as K

    B = prompt.shape[0]
    with torch.no_grad():
        if audio is None:
            A, full = 0, model(None, prompt, input_pos=torch.arange(P, device=prompt.device))
        else:
            A = model.audio_positions(audio.shape[1])
            full = model(audio, prompt, input_pos=torch.arange(A + P, device=prompt.device))
        assert full.shape[:2] == (B, P)  # the audio positions are dropped before the head
        pos = A + torch.tensor(lens, device=prompt.device) - 1
        logits = torch.stack([full[b, lens[b] - 1] for b in range(B)])
        toks = []
        for k in range(n):
            t = K.sample(logits, temperature=0.0, pos=pos + k)
            toks.append(t.clone())
            logits = model(None, t.view(B, 1), input_pos=(pos + k + 1)[:, None] if B > 1 else pos + k + 1)[:, 0]
    return torch.stack(toks, 1)


def test_greedy_with_a_clip_equals_the_hand_loop(cuda):
    from llx._lib import LlxError

    model = _model(1, cuda)
    audio, prompt = _inputs(1, cuda)
    assert model.audio_positions(SAMPLES) == 10
    want = _hand_loop(model, audio, prompt, [P], N)
    got = model.generate(audio, prompt, N)
    assert got.shape == (1, N) and torch.equal(got, want) and got.unique().numel() > 1
    assert torch.equal(model.generate(audio, prompt, N, check_every=1, eos_id=int(want[0, 3]))[0], want[0, : want[0].tolist().index(int(want[0, 3])) + 1])
    # the clip changes the continuation, and without one the audio model generates as a text model
    text = _hand_loop(model, None, prompt, [P], N)
    assert torch.equal(model.generate(None, prompt, N), text) and not torch.equal(text, want)
    from llx.generate import generate

    assert torch.equal(generate(model, prompt, N), text)
    room = O.TINY.max_seq_len - 10 - P
    with pytest.raises(LlxError, match=rf"audio \(10 positions\) \+ prompt \({P}\) \+ max_new_tokens \({room + 1}\) exceeds max_seq_len"):
        model.generate(audio, prompt, room + 1)


def test_a_batch_with_prompt_lens_equals_the_hand_loop(cuda):
    model = _model(3, cuda)
    audio, prompt = _inputs(3, cuda)
    want = _hand_loop(model, audio, prompt, list(LENS), N)
    got = model.generate(audio, prompt, N, prompt_lens=list(LENS))
    assert got.shape == (3, N) and torch.equal(got, want)
    sampled = dict(temperature=0.8, top_p=0.9, seed=5)
    a = model.generate(audio, prompt, N, prompt_lens=list(LENS), **sampled)
    assert torch.equal(a, model.generate(audio, prompt, N, prompt_lens=list(LENS), check_every=1, **sampled)) and not torch.equal(a, got)


def test_beams_with_a_clip_equal_the_host_loop(cuda):
    from llx import sampling as S

    W = 2
    model = _model(W, cuda)
    audio, prompt = _inputs(1, cuda, BEAM_SEED)
    A = model.audio_positions(SAMPLES)
    caches = [c for layer in model.layers for c in (layer.attention.kv_cache.k_cache, layer.attention.kv_cache.v_cache)]
    st, margins = S.beam_state(W), []
    with torch.no_grad():
        logits = model(audio.expand(W, -1).contiguous(), prompt.expand(W, -1).contiguous(), input_pos=torch.arange(A + P, device=cuda))[:, -1]
        for k in range(1, N + 1):
            parent = S.beam_step(st, logits.double().tolist(), W, max_new_tokens=N, margins=margins)
            if k > 1:
                idx = torch.tensor(parent, device=cuda)
                for c in caches:
                    c[:W, :, : A + P + k - 1] = c[:, :, : A + P + k - 1].index_select(0, idx)
            if st["done"]:
                break
            tok = torch.tensor([[h[-1]] for h in st["hist"]], device=cuda)
            logits = model(None, tok, input_pos=torch.arange(A + P + k - 1, A + P + k, device=cuda))[:, 0]
    want = S.beam_ranked(st, margins)
    print(f"audio beams: min margin {min(margins):.4f} over {len(margins)} decisions")
    assert min(margins) >= MARGIN, min(margins)
    stats = {}
    got = model.generate(audio, prompt, N, num_beams=W, stats=stats)
    assert got[0].tolist() == want[0][0] and [t for t, _ in stats["beams"]] == [t for t, _ in want]
    assert max(abs(f - g) for (_, f), (_, g) in zip(stats["beams"], want)) <= SCORE_TOL * N
