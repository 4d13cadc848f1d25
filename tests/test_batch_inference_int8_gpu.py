"""GPU: batched decode (2 <= B <= 16 sequences, one token each) on dynamic-int8 linears - the weight-streaming path of llx/decode.py
with llx_gemm_rows16_i8 - against the generic inference path on the same model and against B batch-1 forwards, on the tiny model, in
generate(), and as one Llama-3.1-8B-dimension layer + bf16 head against a 4k-token cache.  Bar: 0.03 x scale, the project's bar for
the fast path against the generic one (tests/test_decode_int8_gpu.py, tests/test_batch_inference_gpu.py)."""
import functools

import pytest
import torch

from oracle import ref as O
from tests.util import bf16_params, build_model

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
LENS, STEPS = (40, 17, 29), 3
DYN = dict(quantize="int8", quantize_kwargs=dict(dynamic_int8_act=True))


def _close(a, b, rel, name):
    scale = b.abs().max().item()
    err = (a - b).abs().max().item()
    assert err <= rel * scale + 1e-6, f"{name}: max err {err:.4e} vs scale {scale:.4e} (allowed {rel * scale:.4e})"


@functools.lru_cache(maxsize=None)
def _params(lora=False):
    p = O.init_params(O.TINY)
    if lora:
        p.update(O.init_lora(O.TINY, 8))
    return bf16_params(p)[0]


def _model(B, cuda, kind="dynamic"):
    """The tiny model with a cache of batch B: every linear of the layers dynamic int8 | q|k|v dynamic int8, the rest bf16 ("mixed") |
    dynamic int8 under a LoRA adapter; the head stays bf16."""
    from subclasses import quantize_linear_

    if kind == "mixed":
        model = build_model(O.TINY, _params(), "cpu")
        for layer in model.layers:
            for m in (layer.attention.wq, layer.attention.wk, layer.attention.wv):
                quantize_linear_(m, "int8", dynamic_int8_act=True)
    elif kind == "lora":
        model = build_model(O.TINY, _params(True), "cpu", lora_rank=8, **DYN)
    else:
        model = build_model(O.TINY, _params(), "cpu", **DYN)
    model.build_cache(inference=True, batch_size=B)
    return model.to(cuda).eval()


def _tokens(B):
    """Right-padded prompts [B, 40] of lengths 40 / 17 / 29 cycling, and the tokens fed at the three decode steps [B, 3]."""
    lens = [LENS[b % 3] for b in range(B)]
    return O.randint("batch8_prompts", (16, max(LENS)), 0, O.TINY.vocab_size)[:B], O.randint("batch8_steps", (16, STEPS), 0, O.TINY.vocab_size)[:B], lens


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


def _run_generic(model, B, cuda):
    import llx.decode as D

    for layer in model.layers:
        layer.attention.kv_cache.k_cache.zero_()
        layer.attention.kv_cache.v_cache.zero_()
    x1, m1 = _probe(model, B, cuda)
    D.BATCHED = False
    try:
        assert not D.layer_ok(model.layers[0], x1, m1) and not D.head_ok(model, x1)
        return _run_batched(model, B, cuda)
    finally:
        D.BATCHED = True


def _probe(model, B, cuda):
    x1 = torch.zeros(B, 1, O.TINY.embed_dim, device=cuda, dtype=BF)
    return x1, model.causal_mask[torch.zeros(B, 1, dtype=torch.int64, device=cuda)][:, None]


@pytest.mark.parametrize("B", [3, 16])
def test_dynamic_int8_batch_takes_the_weight_stream(cuda, B):
    """Ragged right-padded prefill + three decode steps at per-sequence positions: the dynamic-int8 model is on the batched fast path, a
    weight-only member in a fused pair or a LoRA adapter takes the layer off it; fast against generic on the same model, and each
    sequence in the batch against the same sequence alone (batch-1 forwards of the same model: the GEMV path)."""
    import llx.decode as D

    model = _model(B, cuda)
    x1, m1 = _probe(model, B, cuda)
    assert D.layer_ok(model.layers[0], x1, m1) and D.layer_ok(model.layers[1], x1, m1) and D.head_ok(model, x1)
    w1 = model.layers[0].feed_forward.w1.weight
    w1.dynamic_int8_act = False  # (w1, w3) of two kinds
    try:
        assert D._plain(model.layers[0].feed_forward.w1) == D.KIND_I8W and not D.layer_ok(model.layers[0], x1, m1)
    finally:
        w1.dynamic_int8_act = True
    assert D.layer_ok(model.layers[0], x1, m1)
    lora = _model(B, cuda, "lora")
    assert not D.layer_ok(lora.layers[0], *_probe(lora, B, cuda))
    del lora

    got = _run_batched(model, B, cuda)
    _close(got, _run_generic(model, B, cuda), 0.03, f"B={B}: weight-streaming path vs generic inference path")
    prompts, steps, lens = _tokens(B)
    one = _model(1, cuda)
    for b in range(B):
        n, out = lens[b], []
        with torch.no_grad():
            out.append(one(prompts[b : b + 1, :n].to(cuda), input_pos=torch.arange(n, device=cuda))[0, -1])
            for t in range(STEPS):
                out.append(one(steps[b : b + 1, t : t + 1].to(cuda), input_pos=torch.tensor([n + t], device=cuda))[0, 0])
        _close(got[b], torch.stack(out).float().cpu(), 0.03, f"B={B}: sequence {b} in the batch vs alone")


def test_mixed_layer_takes_the_weight_stream(cuda):
    """q|k|v dynamic int8, wo / w1|w3 / w2 bf16: groups of different kinds next to each other in a layer, as at batch 1."""
    import llx.decode as D

    B = 3
    model = _model(B, cuda, "mixed")
    att = model.layers[0].attention
    assert D._plain(att.wq) == D.KIND_I8D and D._plain(att.wo) == D.KIND_BF16
    assert D.layer_ok(model.layers[0], *_probe(model, B, cuda))
    got = _run_batched(model, B, cuda)
    _close(got, _run_generic(model, B, cuda), 0.03, "mixed layer: weight-streaming path vs generic inference path")


def test_generate_on_the_dynamic_int8_model(cuda):
    """generate(prompts [3, P], 8, prompt_lens=...) greedy = a hand-written loop of model(...) calls and lowest-index argmax."""
    from llx.generate import prefill

    B, P, N = 3, 40, 8
    model = _model(B, cuda)
    prompt = O.randint("generate8_prompts", (B, P), 0, O.TINY.vocab_size).to(cuda)
    lens = list(LENS)
    V = O.TINY.vocab_size

    def lowest_argmax(logits):  # [B, V]
        top = logits.max(-1, keepdim=True).values
        return torch.where(logits == top, torch.arange(V, device=cuda), V).min(-1).values

    pos = torch.tensor(lens, device=cuda) - 1
    with torch.no_grad():
        logits = prefill(model, prompt, lens)[:, 0]
        toks = []
        for k in range(N):
            t = lowest_argmax(logits)
            toks.append(t)
            if k < N - 1:
                logits = model(t.view(B, 1), input_pos=(pos + k + 1)[:, None])[:, 0]
    want = torch.stack(toks, 1)
    got = model.generate(prompt, N, prompt_lens=lens)
    assert got.shape == (B, N) and torch.equal(got, want)
    assert got.unique().numel() > 1


@functools.lru_cache(maxsize=None)
def _layer_params():
    """The bf16 parameters of one Llama-3.1-8B-dimension layer + head, drawn once for the module; every case builds its own model."""
    cfg = O.LLAMA31_8B._replace(num_layers=1, max_seq_len=4352, vocab_size=8)
    return cfg, bf16_params(O.init_params(cfg))[0]


@pytest.mark.parametrize("B", [2, 16])
def test_batched_int8_layer_at_8b_dimensions(cuda, B):
    """One decode step of B sequences at positions around 4100 of a filled cache, at the shapes where the LDS cap (gate|up, w2 at
    B = 16) and the K = 14336 split decide: the layer and the head take the weight stream, and the generic inference path on the same
    device state agrees within 3 %."""
    import llx.decode as D

    t0 = 4100
    cfg, pb = _layer_params()
    model = build_model(cfg, pb, "cpu", **DYN)  # the layer quantised dynamic, the head bf16
    model.build_cache(inference=True, batch_size=B)
    model = model.to(cuda).eval()
    layer = model.layers[0]
    Smax = cfg.max_seq_len
    kc0 = O.randn("bl8_kc", (1, cfg.num_kv_heads, Smax, 128), 1.0).to(BF).to(cuda)
    vc0 = O.randn("bl8_vc", (1, cfg.num_kv_heads, Smax, 128), 1.0).to(BF).to(cuda)
    kc0[:, :, t0:], vc0[:, :, t0:] = 0, 0
    cache = layer.attention.kv_cache
    tok = O.randint("bl8_tok", (16, 1), 0, 8)[:B].to(cuda)
    pos = (t0 + torch.arange(B) % 3)[:, None].to(cuda)  # [B, 1]: 4100 / 4101 / 4102 cycling

    def run():
        for b in range(B):  # every slot its own history: the shared rows rolled along the head dimension
            cache.k_cache[b].copy_(kc0[0].roll(b, 2))
            cache.v_cache[b].copy_(vc0[0].roll(b, 2))
        with torch.no_grad():
            return model(tok, input_pos=pos).float().cpu()

    x1 = model.tok_embeddings(tok)
    assert D.layer_ok(layer, x1, model.causal_mask[pos][:, None]) and D.head_ok(model, x1), "the int8 layer is not on the batched fast path"
    fast = run()
    D.BATCHED = False
    try:
        assert not D.layer_ok(layer, x1, model.causal_mask[pos][:, None])
        slow = run()
    finally:
        D.BATCHED = True
    assert fast.shape == (B, 1, 8)
    _close(fast, slow, 0.03, f"B={B}: weight-streaming path vs generic inference path")
