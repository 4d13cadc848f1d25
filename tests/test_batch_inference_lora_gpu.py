"""GPU: batched decode (2 <= B <= 16 sequences, one token each) on LoRA / DoRA linears - the weight-streaming path of llx/decode.py
with llx_gemm_rows16_bf16_lora / llx_gemm_rows16_i8_lora - against the generic inference path on the same model and against B batch-1
forwards, on the tiny model (LoRA r = 16 on bf16, DoRA r = 16 on bf16, LoRA r = 16 on dynamic int8, one model with q|k|v ranks
16 / 32 / 16), in generate(), and as one Llama-3.1-8B-dimension layer + head against a 4k-token cache.  Bar: 0.03 x scale, the
project's bar for the fast path against the generic one (tests/test_batch_inference_gpu.py).  The helpers are those of
tests/test_batch_inference_int8_gpu.py, restated.  The B factors are drawn with std 0.05 (O.init_lora's default is 0.01) so that the
adapter term is a visible part of every linear's output."""
import functools

import pytest
import torch

from oracle import ref as O
from tests.util import bf16_params, to_model_config

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
LENS, STEPS = (40, 17, 29), 3
KINDS = ("lora16", "dora16", "lora16-int8")
MIXED = {"attention.wk": 32}  # the mixed-rank model: wk rank 32, every other linear 16


def _close(a, b, rel, name):
    scale = b.abs().max().item()
    err = (a - b).abs().max().item()
    assert err <= rel * scale + 1e-6, f"{name}: max err {err:.4e} vs scale {scale:.4e} (allowed {rel * scale:.4e})"


@functools.lru_cache(maxsize=None)
def _params(cfg=O.TINY):
    """bf16 base parameters, factors of rank 16 and - under the keys "<linear>.r32.lora_a/b" - of rank 32, and DoRA magnitudes."""
    p = O.init_params(cfg)
    p.update(O.init_dora_m(p, cfg))
    p.update(O.init_lora(cfg, 16, b_std=0.05))
    p.update({k.replace(".lora_", ".r32.lora_"): v for k, v in O.init_lora(cfg, 32, seed=4321, b_std=0.05).items()})
    return bf16_params(p)[0]


def _adapted(cfg, pb, kind, B, cuda, ranks=None):
    """Llama(cfg) with every layer linear dressed: kind = "lora16" | "dora16" | "lora16-int8" (quantised dynamic first, then adapted, the
    training script's order); ranks: {linear suffix: 32} for the members that take the rank-32 factors.  alpha = 2 r: one scale, 2."""
    from modelling import Llama, apply_linear_adapter_
    from subclasses import quantize_linear_

    model = Llama(to_model_config(cfg)).bfloat16()
    model.load_state_dict({k: v for k, v in pb.items() if "lora_" not in k and not k.endswith(".m")})
    if kind.endswith("-int8"):
        quantize_linear_(model.layers, "int8", dynamic_int8_act=True)
    adapter = "dora" if kind.startswith("dora") else "lora"
    with torch.no_grad():
        for name, mod in model.layers.named_modules():
            key = f"layers.{name}"
            if key + ".lora_a" not in pb:
                continue
            r = next((v for suf, v in (ranks or {}).items() if name.endswith(suf)), 16)
            apply_linear_adapter_(mod, adapter, rank=r, alpha=2.0 * r)
            src = key + (".r32" if r == 32 else "")
            mod.lora_a.copy_(pb[src + ".lora_a"])
            mod.lora_b.copy_(pb[src + ".lora_b"])
            if adapter == "dora":
                mod.m.copy_(pb[key + ".m"])
    model.build_cache(inference=True, batch_size=B)
    return model.to(cuda).eval()


def _tokens(B):
    """Right-padded prompts [B, 40] of lengths 40 / 17 / 29 cycling, and the tokens fed at the three decode steps [B, 3]."""
    lens = [LENS[b % 3] for b in range(B)]
    return O.randint("batchl_prompts", (16, max(LENS)), 0, O.TINY.vocab_size)[:B], O.randint("batchl_steps", (16, STEPS), 0, O.TINY.vocab_size)[:B], lens


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


def _probe(model, B, cuda):
    x1 = torch.zeros(B, 1, O.TINY.embed_dim, device=cuda, dtype=BF)
    return x1, model.causal_mask[torch.zeros(B, 1, dtype=torch.int64, device=cuda)][:, None]


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


def _check_model(model, one, B, cuda, name):
    import llx.decode as D

    x1, m1 = _probe(model, B, cuda)
    assert D.layer_ok(model.layers[0], x1, m1) and D.layer_ok(model.layers[1], x1, m1) and D.head_ok(model, x1), f"{name}: not on the batched fast path"
    got = _run_batched(model, B, cuda)
    _close(got, _run_generic(model, B, cuda), 0.03, f"{name} B={B}: weight-streaming path vs generic inference path")
    prompts, steps, lens = _tokens(B)
    for b in range(B):
        n, out = lens[b], []
        with torch.no_grad():
            out.append(one(prompts[b : b + 1, :n].to(cuda), input_pos=torch.arange(n, device=cuda))[0, -1])
            for t in range(STEPS):
                out.append(one(steps[b : b + 1, t : t + 1].to(cuda), input_pos=torch.tensor([n + t], device=cuda))[0, 0])
        _close(got[b], torch.stack(out).float().cpu(), 0.03, f"{name} B={B}: sequence {b} in the batch vs alone")
    return got


@pytest.mark.parametrize("B", [3, 16])
@pytest.mark.parametrize("kind", KINDS)
def test_adapted_batch_takes_the_weight_stream(cuda, kind, B):
    """Ragged right-padded prefill + three decode steps at per-sequence positions: the adapted model is on the batched fast path; fast
    against generic on the same model, and each sequence in the batch against the same sequence alone (batch-1 forwards: the GEMV)."""
    model = _adapted(O.TINY, _params(), kind, B, cuda)
    got = _check_model(model, _adapted(O.TINY, _params(), kind, 1, cuda), B, cuda, kind)
    if kind == "lora16" and B == 3:  # the adapters are a visible part of the logits: the base model alone misses the bar
        from tests.util import build_model

        base = build_model(O.TINY, {k: v for k, v in _params().items() if not k.endswith(".m") and ".r32." not in k}, "cpu")
        base.build_cache(inference=True, batch_size=B)
        plain = _run_batched(base.to(cuda).eval(), B, cuda)
        assert (got - plain).abs().max().item() > 0.03 * plain.abs().max().item()


def test_mixed_rank_model_takes_the_weight_stream(cuda):
    """wq / wk / wv of ranks 16 / 32 / 16 (the other linears 16): per-segment ranks and t offsets in the q|k|v launch."""
    B = 3
    model = _adapted(O.TINY, _params(), "lora16", B, cuda, MIXED)
    att = model.layers[0].attention
    assert (att.wq.rank, att.wk.rank, att.wv.rank) == (16, 32, 16)
    _check_model(model, _adapted(O.TINY, _params(), "lora16", 1, cuda, MIXED), B, cuda, "ranks 16/32/16")


def test_generate_on_the_lora_model(cuda):
    """generate(prompts [3, P], 8, prompt_lens=...) greedy = a hand-written loop of model(...) calls and lowest-index argmax."""
    import llx.decode as D
    from llx.generate import prefill

    B, P, N = 3, 40, 8
    model = _adapted(O.TINY, _params(), "lora16", B, cuda)
    assert D.layer_ok(model.layers[0], *_probe(model, B, cuda))
    prompt = O.randint("generatel_prompts", (B, P), 0, O.TINY.vocab_size).to(cuda)
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
def _layer_cfg():
    return O.LLAMA31_8B._replace(num_layers=1, max_seq_len=4352, vocab_size=8)


@pytest.mark.parametrize("B", [2, 16])
@pytest.mark.parametrize("kind", KINDS)
def test_batched_adapted_layer_at_8b_dimensions(cuda, kind, B):
    """One decode step of B sequences at positions around 4100 of a filled cache, at the shapes where every product is split (the
    adapter term runs in the combine launch) and K = 14336: the layer and the head take the weight stream, the generic inference path
    on the same device state agrees within 3 %, and a second run of the fast path is bit-identical."""
    import llx.decode as D

    t0 = 4100
    cfg = _layer_cfg()
    model = _adapted(cfg, _params(cfg), kind, B, cuda)
    layer = model.layers[0]
    Smax = cfg.max_seq_len
    kc0 = O.randn("bll_kc", (1, cfg.num_kv_heads, Smax, 128), 1.0).to(BF).to(cuda)
    vc0 = O.randn("bll_vc", (1, cfg.num_kv_heads, Smax, 128), 1.0).to(BF).to(cuda)
    kc0[:, :, t0:], vc0[:, :, t0:] = 0, 0
    cache = layer.attention.kv_cache
    tok = O.randint("bll_tok", (16, 1), 0, 8)[:B].to(cuda)
    pos = (t0 + torch.arange(B) % 3)[:, None].to(cuda)  # [B, 1]: 4100 / 4101 / 4102 cycling

    def run():
        for b in range(B):  # every slot its own history: the shared rows rolled along the head dimension
            cache.k_cache[b].copy_(kc0[0].roll(b, 2))
            cache.v_cache[b].copy_(vc0[0].roll(b, 2))
        with torch.no_grad():
            return model(tok, input_pos=pos).float().cpu()

    x1 = model.tok_embeddings(tok)
    assert D.layer_ok(layer, x1, model.causal_mask[pos][:, None]) and D.head_ok(model, x1), "the adapted layer is not on the batched fast path"
    fast = run()
    assert torch.equal(fast, run()), "a second run of the fast path differs"
    D.BATCHED = False
    try:
        assert not D.layer_ok(layer, x1, model.causal_mask[pos][:, None])
        slow = run()
    finally:
        D.BATCHED = True
    assert fast.shape == (B, 1, 8)
    _close(fast, slow, 0.03, f"{kind} B={B}: weight-streaming path vs generic inference path")
