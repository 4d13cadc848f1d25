"""GPU: the tiny model with MXFP4 layer linears (quantize_linear_(model.layers, "mxfp4")) against its twin - the same model with bf16
weights set to dequantize().  An MXFP4 linear is a bf16 linear on the dequantised image: every path that builds the image (prefill,
training, batched decode) makes the twin's GEMM calls on the twin's operands and must equal it bit for bit; the decode fast path streams
the packed rows with the rounding points of the bf16 GEMV (bit-exact on exact operands, tests/test_mxfp4_gpu.py) and is held to the
project's bar for fast against generic, 3 % of the max-norm.  No bf16 image of a weight survives a call."""
import functools

import pytest
import torch

from oracle import ref as O
from tests import mx_cases as C
from tests.util import _close, bf16_params, build_model

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
P, N = 40, 12
_MODELS: dict = {}


@functools.lru_cache(maxsize=None)
def _params(lora: bool):
    """(bf16 parameters, the same with every layer linear replaced by its dequantised MXFP4 image - by the oracle of tests/mx_cases.py)."""
    p = O.init_params(O.TINY)
    if lora:
        p.update(O.init_lora(O.TINY, 8))
    pb, _ = bf16_params(p)
    twin = dict(pb)
    for i in range(O.TINY.num_layers):
        for suf in O.LINEAR_SUFFIXES:
            key = f"layers.{i}.{suf}.weight"
            twin[key] = C.dequantize(*C.quantize(pb[key]))
    return pb, twin


def _model(kind: str, cuda, lora: bool = False, batch: int = 1):
    """kind: "mx" (quantised on the host, then moved) | "twin"."""
    key = (kind, lora, batch)
    if key not in _MODELS:
        pb, twin = _params(lora)
        kw = dict(lora_rank=8 if lora else 0)
        model = build_model(O.TINY, pb, "cpu", quantize="mxfp4", **kw) if kind == "mx" else build_model(O.TINY, twin, "cpu", **kw)
        model.build_cache(inference=True, batch_size=batch)
        _MODELS[key] = model.to(cuda).eval()
    return _MODELS[key]


def _prompt(cuda, B=1):
    return O.randint("mx_model_prompt", (B, P), 0, O.TINY.vocab_size).to(cuda)


def test_quantised_model_holds_the_oracle_bytes(cuda):
    from subclasses import MXFP4LinearWeight

    model, (pb, twin) = _model("mx", cuda), _params(False)
    for i, layer in enumerate(model.layers):
        for suf in O.LINEAR_SUFFIXES:
            w = layer.get_submodule(suf).weight
            assert isinstance(w, MXFP4LinearWeight) and w.is_cuda and not w.requires_grad
            packed, scale = C.quantize(pb[f"layers.{i}.{suf}.weight"])
            assert torch.equal(w.packed.cpu(), packed) and torch.equal(w.scale.cpu(), scale)
            assert torch.equal(w.dequantize().cpu(), twin[f"layers.{i}.{suf}.weight"])
    assert not isinstance(model.output.weight, MXFP4LinearWeight)


def test_prefill_equals_the_twin(cuda):
    """(a) the same GEMMs on the same operands."""
    prompt, pos = _prompt(cuda), torch.arange(P, device=cuda)
    with torch.no_grad():
        got = _model("mx", cuda)(prompt, input_pos=pos)
        want = _model("twin", cuda)(prompt, input_pos=pos)
    assert got.shape == (1, P, O.TINY.vocab_size) and torch.equal(got, want)


def test_decode_streams_the_packed_rows(cuda):
    """(b) batch-1 decode steps and 2-4-row steps take the fast path; logits within 3 % of the twin's."""
    import llx.decode as D

    mx, twin = _model("mx", cuda), _model("twin", cuda)
    prompt = _prompt(cuda)
    steps = O.randint("mx_model_steps", (1, 12), 0, O.TINY.vocab_size).to(cuda)
    with torch.no_grad():
        for m in (mx, twin):
            m(prompt, input_pos=torch.arange(P, device=cuda))
        at = P
        for rows in (1, 1, 2, 3, 4, 1):
            tok, pos = steps[:, at - P:at - P + rows], torch.arange(at, at + rows, device=cuda)
            x = mx.tok_embeddings(tok)
            mask = mx.causal_mask[None, None, pos]
            assert all(D.layer_ok(layer, x, mask) for layer in mx.layers), f"{rows} rows: not on the fast path"
            assert D.head_ok(mx, x)
            got, want = mx(tok, input_pos=pos), twin(tok, input_pos=pos)
            err = (got.float() - want.float()).abs().max().item() / want.float().abs().max().item()
            print(f"[mxfp4 decode, {rows} rows at {at}] max err / max-norm {err:.4f}")
            _close(got.float().cpu(), want.float().cpu(), 0.03, f"decode logits, {rows} rows at {at}")
            at += rows


def test_decode_with_a_quantised_head(cuda):
    """head_ok / head_forward on an MXFP4 head: the model-level call against fp32 logits on the head's image, within the 3 % bar
    (the GEMV itself is held bit for bit in tests/test_mxfp4_gpu.py)."""
    import llx.decode as D
    from subclasses import quantize_linear_

    pb, _ = _params(False)
    model = build_model(O.TINY, pb, "cpu", quantize="mxfp4")
    quantize_linear_(model.output, "mxfp4")
    model.build_cache(inference=True)
    model = model.to(cuda).eval()
    x = O.randn("mx_head_x", (1, 3, O.TINY.embed_dim), 1.0).to(BF).to(cuda)
    assert D._plain(model.output) == D.KIND_MX4 and D.head_ok(model, x)
    with torch.no_grad():
        got = D.head_forward(model, x)
        xn = torch.nn.functional.rms_norm(x.float(), (O.TINY.embed_dim,), model.norm.weight.float(), model.norm.eps).to(BF)
        want = xn.float() @ model.output.weight.dequantize().float().T
    _close(got.float().cpu(), want.cpu(), 0.03, "logits of an MXFP4 head")


def test_generate_equals_the_hand_loop(cuda):
    """(c) generate() on the MXFP4 model, token for token against a loop of model(...) calls on the same model."""
    model, prompt = _model("mx", cuda), _prompt(cuda)

    def greedy(row):
        x = row.float()
        return (x[0] == x[0].max()).nonzero()[0]

    with torch.no_grad():
        last = model(prompt, input_pos=torch.arange(P, device=cuda))[0, -1:]
        toks = []
        for k in range(N):
            t = greedy(last)
            toks.append(t.view(1))
            if k < N - 1:
                last = model(t.view(1, 1), input_pos=torch.tensor([P + k], device=cuda))[0]
    want = torch.cat(toks)[None]
    got = model.generate(prompt, N)
    assert got.shape == (1, N) and torch.equal(got, want) and len(set(got[0].tolist())) > 1


@pytest.mark.parametrize("head", [False, True], ids=["bf16-head", "mxfp4-head"])
def test_training_step_equals_the_twin(cuda, head):
    """(d) MXFP4 base + LoRA r = 8: loss and adapter gradients of one step equal the twin's with a frozen base.  head: the LM head
    quantised too (the twin's head is its image): the frozen-head route of the loss on a transient image."""
    from subclasses import quantize_linear_

    tokens = O.randint("mx_model_train", (1, 256), 0, O.TINY.vocab_size)
    labels = torch.roll(tokens, -1, 1).clone()
    labels[:, :64] = -100
    res = {}
    for kind in ("mx", "twin"):
        pb, twin = _params(True)
        if head and kind == "twin":
            twin = dict(twin)
            twin["output.weight"] = C.dequantize(*C.quantize(pb["output.weight"]))
        model = build_model(O.TINY, pb if kind == "mx" else twin, "cpu", lora_rank=8, quantize="mxfp4" if kind == "mx" else None)
        if head and kind == "mx":
            quantize_linear_(model.output, "mxfp4")
        model = model.to(cuda)
        for n, q in model.named_parameters():
            if "lora_" not in n:
                q.requires_grad_(False)
        loss = model(tokens.to(cuda), labels=labels.to(cuda))
        loss.backward()
        grads = {n: q.grad.clone() for n, q in model.named_parameters() if q.requires_grad}
        assert len(grads) == 2 * 7 * O.TINY.num_layers and all(g.abs().sum() > 0 for n, g in grads.items() if n.endswith("lora_b"))
        res[kind] = (loss.detach().clone(), grads)
    assert torch.equal(res["mx"][0], res["twin"][0]), (res["mx"][0].item(), res["twin"][0].item())
    for n, g in res["twin"][1].items():
        assert torch.equal(res["mx"][1][n], g), n


def test_batched_decode_takes_the_generic_path(cuda, monkeypatch):
    """(e) B = 3: no batched stream for the kind - layer_ok is false and the logits equal the twin's generic path.  The twin's layers
    are sent down the generic path by hand (its bf16 linears would take the batched stream); the head is bf16 on both models and takes
    the same route on both, so the logits compare like with like."""
    import llx.decode as D

    B = 3
    mx, twin = _model("mx", cuda, batch=B), _model("twin", cuda, batch=B)
    prompt = _prompt(cuda, B)
    step = O.randint("mx_model_bstep", (B, 1), 0, O.TINY.vocab_size).to(cuda)
    pos = torch.full((B, 1), P, device=cuda, dtype=torch.int64)
    x = torch.zeros(B, 1, O.TINY.embed_dim, device=cuda, dtype=BF)
    mask = mx.causal_mask[torch.zeros(B, 1, dtype=torch.int64, device=cuda)][:, None]
    assert D.layer_ok(twin.layers[0], x, mask) and not D.layer_ok(mx.layers[0], x, mask)
    with torch.no_grad():
        assert D.head_ok(mx, x) and D.head_ok(twin, x)
        got = [mx(prompt, input_pos=torch.arange(P, device=cuda)), mx(step, input_pos=pos)]
        monkeypatch.setattr(D, "layer_ok", lambda layer, x_, mask_: False)
        want = [twin(prompt, input_pos=torch.arange(P, device=cuda)), twin(step, input_pos=pos)]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_no_image_is_retained(cuda):
    """(f) after a warm-up a prefill and a decode step leave less than one layer linear's bf16 image behind."""
    model, prompt = _model("mx", cuda), _prompt(cuda)

    def call():
        with torch.no_grad():
            a = model(prompt, input_pos=torch.arange(P, device=cuda))
            b = model(prompt[:, :1], input_pos=torch.tensor([P], device=cuda))
        del a, b

    call()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    call()
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    smallest = min(layer.get_submodule(suf).weight.numel() for layer in model.layers for suf in O.LINEAR_SUFFIXES) * 2
    print(f"[mxfp4 memory] {grown} bytes retained by a prefill and a decode step; smallest linear image {smallest} bytes")
    assert grown < smallest
    for layer in model.layers:
        for suf in O.LINEAR_SUFFIXES:
            w = layer.get_submodule(suf).weight
            assert not any(t.__dict__.get("_llx_cache") for t in (w, w.packed, w.scale)), f"{suf}: a cached image"
