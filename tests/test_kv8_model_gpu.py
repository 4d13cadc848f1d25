"""GPU: the tiny model (G = 4 query heads per kv head) with an FP8 KV cache against its twin - the same weights with a bf16 cache whose
KVCache.update is wrapped so that k and v pass through clamp -> float8_e4m3fn -> bf16 before they are stored.  The contract (DESIGN
8.21): an fp8 cache behaves as a bf16 cache that holds dq(q(x)) wherever that one holds x.  The twin's rounding happens in Python and the
fast epilogues write the cache themselves, so the twin stays on the generic path (decode.layer_ok forced False for it).

  (a) the buffers, the default and the refusals of build_cache;
  (b) both models on the generic path: equal logits bit for bit, and dequantize() == the twin's cache bit for bit;
  (c) the fp8 model on the fast path (1-4 rows at batch 1, B = 3), on bf16, MXFP4 and dynamic-int8 layers: within the project's bar for
      fast against generic, 3 % of the max-norm of the twin's generic logits;
  (d) generate() on the fp8 model - greedy, B = 3 with prompt_lens, draft_tokens = 2, num_beams = 3 - token for token against the host
      loops of the matching existing tests, the fp8 model in both arms; a decode step captured in a graph replays the same logits."""
import pytest
import torch

from oracle import ref as O
from tests.util import _close, bf16_params, build_model

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
P = 40
KINDS = {"bf16": {}, "mxfp4": dict(quantize="mxfp4"), "int8d": dict(quantize="int8", quantize_kwargs=dict(dynamic_int8_act=True))}
_MODELS: dict = {}


def _through_e4m3(t):
    """dq(q(t)) in Python, on the host (the cast the CPU tests hold against the oracle on every bf16 pattern)."""
    return t.detach().cpu().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(BF).to(t.device)


def _model(cuda, kv="fp8", kind="bf16", batch=1, head_gain=None):
    """kv: "fp8" | "bf16" | "twin" (a bf16 cache that stores dq(q(.)))."""
    key = (kv, kind, batch, head_gain)
    if key not in _MODELS:
        pb, _ = bf16_params(O.init_params(O.TINY))
        model = build_model(O.TINY, pb, "cpu", **KINDS[kind])
        if head_gain:
            with torch.no_grad():
                model.output.weight.mul_(head_gain)
        model.build_cache(inference=True, batch_size=batch, **(dict(kv_dtype="fp8") if kv == "fp8" else {}))
        model = model.to(cuda).eval()
        if kv == "twin":
            for layer in model.layers:
                cache = layer.attention.kv_cache
                cache.update = (lambda orig: lambda pos, k, v: orig(pos, _through_e4m3(k), _through_e4m3(v)))(cache.update)
        _MODELS[key] = model
    return _MODELS[key]


def _generic(monkeypatch):
    import llx.decode as D

    monkeypatch.setattr(D, "layer_ok", lambda layer, x, mask: False)


def _prompt(cuda, B=1, n=P):
    return O.randint("kv8_model_prompt", (B, n), 0, O.TINY.vocab_size).to(cuda)


# --------------------------------------------------------------------------------------------------------------------------------- (a)
def test_buffers_default_and_refusals(cuda):
    from llx._lib import LlxError
    from modelling import Llama
    from tests.util import to_model_config

    f8, bf = _model(cuda, "fp8"), _model(cuda, "bf16")
    for lf, lb in zip(f8.layers, bf.layers):
        for name in ("k_cache", "v_cache"):
            cf, cb = getattr(lf.attention.kv_cache, name), getattr(lb.attention.kv_cache, name)
            assert cf.dtype is torch.uint8 and cb.dtype is BF and cf.shape == cb.shape == (1, 1, O.TINY.max_seq_len, 128)
            assert cf.numel() * cf.element_size() * 2 == cb.numel() * cb.element_size()
            assert name not in lf.attention.kv_cache.state_dict()
        assert lf.attention.kv_cache.kv_dtype == "fp8" and lb.attention.kv_cache.kv_dtype == "bf16"

    def fresh(**cfg):
        return Llama(to_model_config(O.TINY._replace(num_layers=1, **cfg))).bfloat16()

    # module.to(dtype) cannot cast the codes (a model of its own: the cast also rounds the shared models' RoPE table)
    m = fresh()
    m.build_cache(inference=True, kv_dtype="fp8")
    assert m.half().bfloat16().layers[0].attention.kv_cache.k_cache.dtype is torch.uint8

    for bad in ("fp16", "e5m2", None, torch.uint8):
        with pytest.raises(LlxError, match="kv_dtype"):
            fresh().build_cache(inference=True, kv_dtype=bad)
    m = fresh(max_seq_len=511)
    with pytest.raises(LlxError, match="even max_seq_len"):
        m.build_cache(inference=True, kv_dtype="fp8")
    assert m.layers[0].attention.kv_cache is None and not hasattr(m, "rope")  # refused before anything was built
    with pytest.raises(LlxError, match="head_dim 128"):
        fresh(head_dim=64, embed_dim=256).build_cache(inference=True, kv_dtype="fp8")
    m = fresh()
    m.build_cache(inference=True, kv_dtype="fp8")  # on the host: allocated, but no call runs there
    with pytest.raises(LlxError), torch.no_grad():
        m(torch.zeros(1, 4, dtype=torch.int64), input_pos=torch.arange(4))
    with pytest.raises(LlxError, match="bf16 cache"):
        bf.layers[0].attention.kv_cache.dequantize()


# --------------------------------------------------------------------------------------------------------------------------------- (b)
def test_generic_path_equals_the_twin_bit_for_bit(cuda, monkeypatch):
    _generic(monkeypatch)
    f8, twin = _model(cuda, "fp8"), _model(cuda, "twin")
    tokens = _prompt(cuda, n=32)
    with torch.no_grad():
        for lo, hi in ((0, 24), (24, 32)):  # a prefill, then a second chunk that reads the first one's keys from the cache
            pos = torch.arange(lo, hi, device=cuda)
            got, want = f8(tokens[:, lo:hi], input_pos=pos), twin(tokens[:, lo:hi], input_pos=pos)
            assert got.shape == (1, hi - lo, O.TINY.vocab_size) and torch.equal(got, want), f"logits of positions {lo}..{hi - 1}"
    for i, (lf, lt) in enumerate(zip(f8.layers, twin.layers)):
        k, v = lf.attention.kv_cache.dequantize()
        assert torch.equal(k.view(torch.int16), lt.attention.kv_cache.k_cache.view(torch.int16)), f"layer {i}: k"
        assert torch.equal(v.view(torch.int16), lt.attention.kv_cache.v_cache.view(torch.int16)), f"layer {i}: v"
        assert bool((k[:, :, :32] != 0).any()) and not bool(k[:, :, 32:].any())


# --------------------------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("kind", list(KINDS))
def test_fast_path_rows_at_batch_1(cuda, monkeypatch, kind):
    import llx.decode as D

    f8, twin = _model(cuda, "fp8", kind), _model(cuda, "twin", kind)
    prompt = _prompt(cuda)
    steps = O.randint("kv8_model_steps", (1, 12), 0, O.TINY.vocab_size).to(cuda)
    layer_ok = D.layer_ok
    with torch.no_grad():
        f8(prompt, input_pos=torch.arange(P, device=cuda))
        with monkeypatch.context() as mp:
            mp.setattr(D, "layer_ok", lambda *a: False)
            twin(prompt, input_pos=torch.arange(P, device=cuda))
        at = P
        for rows in (1, 2, 3, 4, 1):
            tok, pos = steps[:, at - P:at - P + rows], torch.arange(at, at + rows, device=cuda)
            x, mask = f8.tok_embeddings(tok), f8.causal_mask[None, None, pos]
            assert all(layer_ok(layer, x, mask) for layer in f8.layers), f"{kind}, {rows} rows: not on the fast path"
            got = f8(tok, input_pos=pos)
            with monkeypatch.context() as mp:
                mp.setattr(D, "layer_ok", lambda *a: False)
                want = twin(tok, input_pos=pos)
            err = (got.float() - want.float()).abs().max().item() / want.float().abs().max().item()
            print(f"[kv8 fast path, {kind}, {rows} rows at {at}] max err / max-norm {err:.4f}")
            _close(got.float().cpu(), want.float().cpu(), 0.03, f"{kind}: decode logits, {rows} rows at {at}")
            at += rows


@pytest.mark.parametrize("kind", ["bf16", "int8d"])
def test_fast_path_batch_of_3(cuda, monkeypatch, kind):
    import llx.decode as D
    from llx.generate import prefill

    B, lens = 3, [40, 17, 29]
    f8, twin = _model(cuda, "fp8", kind, B), _model(cuda, "twin", kind, B)
    prompt = _prompt(cuda, B)
    layer_ok = D.layer_ok
    tok = O.randint("kv8_model_bstep", (B, 2), 0, O.TINY.vocab_size).to(cuda)
    with torch.no_grad():
        prefill(f8, prompt, lens)
        with monkeypatch.context() as mp:
            mp.setattr(D, "layer_ok", lambda *a: False)
            prefill(twin, prompt, lens)
        for s in range(2):
            pos = (torch.tensor(lens, device=cuda) + s)[:, None]
            x, mask = f8.tok_embeddings(tok[:, s:s + 1]), f8._inference_mask(B, pos)
            assert all(layer_ok(layer, x, mask) for layer in f8.layers), f"{kind}: the batch is not on the fast path"
            got = f8(tok[:, s:s + 1], input_pos=pos)
            with monkeypatch.context() as mp:
                mp.setattr(D, "layer_ok", lambda *a: False)
                want = twin(tok[:, s:s + 1], input_pos=pos)
            err = (got.float() - want.float()).abs().max().item() / want.float().abs().max().item()
            print(f"[kv8 fast path, {kind}, B = 3, step {s}] max err / max-norm {err:.4f}")
            _close(got.float().cpu(), want.float().cpu(), 0.03, f"{kind}: batched decode logits, step {s}")


# --------------------------------------------------------------------------------------------------------------------------------- (d)
def test_generate_greedy(cuda):
    from tests import test_generate_gpu as T

    model, prompt = _model(cuda, "fp8"), _prompt(cuda, n=T.P)
    want = T._hand_loop(model, prompt, T.N, T._greedy)
    got = model.generate(prompt, T.N)
    assert got.shape == (1, T.N) and torch.equal(got, want) and len(set(got[0].tolist())) > 1
    assert torch.equal(model.generate(prompt, T.N, prefill_chunk=16), got)  # chunks past the first read the image of the codes
    assert torch.equal(model.generate(prompt, T.N), got)


def test_generate_batch_with_prompt_lens(cuda):
    from tests import test_generate_batch_gpu as T

    B = 3
    model = _model(cuda, "fp8", batch=B)
    prompt, lens = T._prompts(B, cuda)
    want = T._hand_loop(model, prompt, lens, T.N, dict(temperature=0.0))
    got = model.generate(prompt, T.N, prompt_lens=lens)
    assert got.shape == (B, T.N) and torch.equal(got, want) and got.unique().numel() > 1
    want_s = T._hand_loop(model, prompt, lens, T.N, T.SAMPLED)
    assert torch.equal(model.generate(prompt, T.N, prompt_lens=lens, **T.SAMPLED), want_s)


def test_generate_with_drafts(cuda):
    from tests import test_generate_draft_gpu as T

    model, prompt = _model(cuda, "fp8"), T._prompt(cuda)
    want, steps, _, _ = T._spec_hand_loop(model, prompt, T.N, 2)
    stats = {}
    got = model.generate(prompt, T.N, draft_tokens=2, draft_ngram=T.G, stats=stats)
    assert got[0].tolist() == want and stats["steps"] == steps and stats["accepted"] == T.N - steps
    assert model.generate(prompt, T.N)[0].tolist() == want  # drafting changes the number of steps, not the tokens


def test_generate_beams(cuda):
    from tests import test_generate_beam_gpu as T

    W = 3
    model = _model(cuda, "fp8", batch=W, head_gain=T.HEAD_GAIN)
    # a prompt whose every beam decision keeps the margin, by the host loop alone (the existing test's seeds were found the same way)
    for seed in range(12):
        prompt = T._prompt("fp8", W, cuda, seed=seed)
        margins: list = []
        want = T._host_beam(model, prompt, T.N, W, None, 1.0, margins)
        if min(margins) >= T.MARGIN:
            break
    else:
        pytest.fail("no prompt seed keeps the margin at every decision")
    print(f"fp8 W={W}: seed {seed}, min margin {min(margins):.4f} over {len(margins)} decisions")
    a = T._check_run(model, prompt, W, None, 1.0, want, 1)
    b = T._check_run(model, prompt, W, None, 1.0, want, 16)
    assert torch.equal(a, b)


def test_decode_step_in_a_graph(cuda):
    """The decode step of an fp8 cache allocates no image: captured after one warm-up step, the graph replays the step's logits and
    leaves the codes the eager step leaves."""
    import llx.decode as D

    model, prompt = _model(cuda, "fp8"), _prompt(cuda)
    tok = torch.tensor([[7]], device=cuda)
    pos = torch.tensor([P], device=cuda)
    with torch.no_grad():
        model(prompt, input_pos=torch.arange(P, device=cuda))
        D.prepare(model)
        want = model(tok, input_pos=pos).clone()  # (the warm-up: workspaces, the mask's extent)
        codes = [layer.attention.kv_cache.k_cache[:, :, P].clone() for layer in model.layers]
        for layer in model.layers:
            layer.attention.kv_cache.k_cache[:, :, P] = 0
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model(tok, input_pos=pos)
        image = model.layers[0].attention.kv_cache.k_cache.numel() * 2
        assert torch.cuda.memory_allocated() - before < image, "the captured step allocated a cache image"
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want)
    for layer, c in zip(model.layers, codes):
        assert torch.equal(layer.attention.kv_cache.k_cache[:, :, P], c)
