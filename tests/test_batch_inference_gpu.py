"""GPU: inference with a KV cache of batch B - build_cache(inference=True, batch_size=B), shared [L] and per-sequence [B, L] positions -
against the oracle run once per sequence with that sequence's own batch-1 cache (the sequences of a batch are independent), on the
weight-streaming path (2 <= B <= 16, bf16 un-adapted linears) and on the generic one (B = 17, LoRA, int8)."""
import pytest
import torch

from oracle import ref as O
from tests.util import bf16_params, build_model

pytestmark = pytest.mark.gpu
LENS, STEPS = (40, 17, 29), 3
_PARAMS: dict = {}
_ORACLE: dict = {}


def _close(a, b, rel, name):
    scale = b.abs().max().item()
    err = (a - b).abs().max().item()
    assert err <= rel * scale + 1e-6, f"{name}: max err {err:.4e} vs scale {scale:.4e} (allowed {rel * scale:.4e})"


def _params(kind):
    if kind not in _PARAMS:
        p = O.init_params(O.TINY)
        if kind == "lora":
            p.update(O.init_lora(O.TINY, 8))
        _PARAMS[kind] = bf16_params(p)
    return _PARAMS[kind]


def _model(kind, B, cuda):
    pb, _ = _params("lora" if kind == "lora" else "bf16")
    if kind == "lora":
        model = build_model(O.TINY, pb, "cpu", lora_rank=8)
    elif kind == "int8":
        model = build_model(O.TINY, pb, "cpu", quantize="int8", quantize_kwargs=dict(dynamic_int8_act=False))
    else:
        model = build_model(O.TINY, pb, "cpu")
    model.build_cache(inference=True, batch_size=B)
    return model.to(cuda).eval()


def _tokens(B):
    """Right-padded prompts [B, 40] of lengths 40 / 17 / 29 cycling, and the tokens fed at the three decode steps [B, 3]."""
    lens = [LENS[b % 3] for b in range(B)]
    return O.randint("batch_prompts", (17, max(LENS)), 0, O.TINY.vocab_size)[:B], O.randint("batch_steps", (17, STEPS), 0, O.TINY.vocab_size)[:B], lens


def _oracle_seq(b):
    """Sequence b alone through O.llama_forward_cached with its own cache: the logits at its last prompt row and at each decode step."""
    if b not in _ORACLE:
        _, pf = _params("bf16")
        prompts, steps, lens = _tokens(17)
        n, cache = lens[b], O.new_cache(O.TINY)
        out = [O.llama_forward_cached(prompts[b : b + 1, :n], pf, O.TINY, cache, torch.arange(n))[0, -1]]
        for t in range(STEPS):
            out.append(O.llama_forward_cached(steps[b : b + 1, t : t + 1], pf, O.TINY, cache, torch.tensor([n + t]))[0, 0])
        _ORACLE[b] = torch.stack(out)  # [1 + STEPS, V]
    return _ORACLE[b]


def _run_batched(model, B, cuda):
    """Batched prefill with shared positions, then three decode steps with input_pos [B, 1] -> [B, 1 + STEPS, V] (fp32, cpu)."""
    prompts, steps, lens = _tokens(B)
    lens_t = torch.tensor(lens, device=cuda)
    with torch.no_grad():
        logits = model(prompts.to(cuda), input_pos=torch.arange(prompts.shape[1], device=cuda))  # [B, P, V]
        out = [logits[torch.arange(B, device=cuda), lens_t - 1]]
        for t in range(STEPS):
            out.append(model(steps[:, t : t + 1].to(cuda), input_pos=(lens_t + t)[:, None])[:, 0])
    return torch.stack(out, 1).float().cpu()


@pytest.mark.parametrize("B", [3, 16, 17])
def test_batched_model_against_the_per_sequence_oracle(cuda, B):
    """Ragged right-padded prompts: no real token attends to a pad (pads come later), and the keys / values the pads leave at positions
    >= len_b are overwritten by sequence b's own decode step before anything attends to them.  B = 17 is past the fast path."""
    import llx.decode as D

    model = _model("bf16", B, cuda)
    x1 = torch.zeros(B, 1, O.TINY.embed_dim, device=cuda, dtype=torch.bfloat16)
    m1 = model.causal_mask[torch.zeros(B, 1, dtype=torch.int64, device=cuda)][:, None]
    assert D.layer_ok(model.layers[0], x1, m1) == (B <= 16) and D.head_ok(model, x1) == (B <= 16)
    got = _run_batched(model, B, cuda)
    for b in range(B):
        _close(got[b], _oracle_seq(b), 0.03, f"B={B}: logits of sequence {b}")
    if B <= 16:  # the generic inference path (MFMA GEMMs, kv_scatter, attn_decode) on the same inputs
        for layer in model.layers:
            layer.attention.kv_cache.k_cache.zero_()
            layer.attention.kv_cache.v_cache.zero_()
        D.BATCHED = False
        try:
            assert not D.layer_ok(model.layers[0], x1, m1) and not D.head_ok(model, x1)
            slow = _run_batched(model, B, cuda)
        finally:
            D.BATCHED = True
        _close(got, slow, 0.03, f"B={B}: weight-streaming path vs generic inference path")


@pytest.mark.parametrize("kind", ["lora", "int8"])
def test_adapted_and_int8_models_take_the_generic_path(cuda, kind):
    """LoRA (r 8) and int8 linears at B = 3 are outside the batched fast path: correct everywhere, against 3 batch-1 forwards of the same
    model through the same positions."""
    import llx.decode as D

    B = 3
    model = _model(kind, B, cuda)
    x1 = torch.zeros(B, 1, O.TINY.embed_dim, device=cuda, dtype=torch.bfloat16)
    assert not D.layer_ok(model.layers[0], x1, model.causal_mask[torch.zeros(B, 1, dtype=torch.int64, device=cuda)][:, None])
    got = _run_batched(model, B, cuda)
    prompts, steps, lens = _tokens(B)
    one = _model(kind, 1, cuda)
    for b in range(B):
        n, out = lens[b], []
        with torch.no_grad():
            out.append(one(prompts[b : b + 1, :n].to(cuda), input_pos=torch.arange(n, device=cuda))[0, -1])
            for t in range(STEPS):
                out.append(one(steps[b : b + 1, t : t + 1].to(cuda), input_pos=torch.tensor([n + t], device=cuda))[0, 0])
        _close(got[b], torch.stack(out).float().cpu(), 0.03, f"{kind}: sequence {b} in the batch vs alone")


def test_shared_positions_at_batch_two(cuda):
    """input_pos [L] with x [2, L] against a batch-2 cache: plain reference semantics (the reference's KVCache and attention are written
    for a batch), prefill of 29 tokens then two single-token steps, per sequence against the oracle."""
    B, n = 2, 29
    model = _model("bf16", B, cuda)
    _, pf = _params("bf16")
    prompts, steps, _ = _tokens(B)
    with torch.no_grad():
        got = [model(prompts[:, :n].to(cuda), input_pos=torch.arange(n, device=cuda))[:, -1]]
        for t in range(2):
            got.append(model(steps[:, t : t + 1].to(cuda), input_pos=torch.tensor([n + t], device=cuda))[:, 0])
    got = torch.stack(got, 1).float().cpu()
    for b in range(B):
        cache = O.new_cache(O.TINY)
        want = [O.llama_forward_cached(prompts[b : b + 1, :n], pf, O.TINY, cache, torch.arange(n))[0, -1]]
        for t in range(2):
            want.append(O.llama_forward_cached(steps[b : b + 1, t : t + 1], pf, O.TINY, cache, torch.tensor([n + t]))[0, 0])
        _close(got[b], torch.stack(want), 0.03, f"shared positions: sequence {b}")


def test_several_tokens_per_call_at_per_sequence_positions(cuda):
    """input_pos [B, 5] at a different offset per row after the ragged prefill: five tokens per sequence in one call, written at
    input_pos[b] and attending through causal_mask[input_pos[b]] (the generic path: the batch form of the cache scatter and the
    mask-driven attention with a mask per batch element), against the oracle per sequence with its own cache and positions."""
    B, L_ = 3, 5
    model = _model("bf16", B, cuda)
    _, pf = _params("bf16")
    prompts, _, lens = _tokens(B)
    more = O.randint("batch_more", (B, L_), 0, O.TINY.vocab_size)
    pos = torch.tensor(lens)[:, None] + torch.arange(L_)  # [B, 5]: rows start at 40 / 17 / 29
    with torch.no_grad():
        model(prompts.to(cuda), input_pos=torch.arange(prompts.shape[1], device=cuda))
        got = model(more.to(cuda), input_pos=pos.to(cuda)).float().cpu()  # [B, 5, V]
    for b in range(B):
        cache = O.new_cache(O.TINY)
        O.llama_forward_cached(prompts[b : b + 1, : lens[b]], pf, O.TINY, cache, torch.arange(lens[b]))
        want = O.llama_forward_cached(more[b : b + 1], pf, O.TINY, cache, pos[b])[0]
        _close(got[b], want, 0.03, f"[B, 5] positions: sequence {b}")


def test_batch_mismatch_names_build_cache(cuda):
    from llx._lib import LlxError

    model = _model("bf16", 2, cuda)
    with pytest.raises(LlxError, match=r"build_cache\(inference=True, batch_size=3\)"):
        model(torch.zeros(3, 1, dtype=torch.int64, device=cuda), input_pos=torch.tensor([0], device=cuda))
