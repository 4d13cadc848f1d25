"""GPU: training through block_mask=MaskSpec(dense=...) at the module level - one TransformerLayer under a scattered mask, the
two-layer LoRA model under a sliding window (loss and adapter gradients against the oracle's dense-mask path), the same model under
activation checkpointing, and MaskSpec.from_mask_mod on the causal mask_mod against block_mask=None.  Tiny config, parameters and
bars of tests/test_model_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref as O  # noqa: E402
from tests.util import _close, _rows_close, bf16_params, build_model  # noqa: E402

CFG = O.TINY
S = 384


def _data(B, S_, seed=0):
    tokens = O.randint("tokens", (B, S_), 0, CFG.vocab_size, seed)
    labels = torch.roll(tokens, -1, 1).clone()
    labels[:, : S_ // 4] = -100
    labels[:, -1] = -100
    return tokens, labels


def _window(S_, w):
    i = torch.arange(S_)
    return (i[:, None] >= i[None, :]) & (i[:, None] - i[None, :] < w)


def _lora_setup(rank=8):
    p = O.init_params(CFG)
    p.update(O.init_lora(CFG, rank))
    return bf16_params(p)


def _lora_model(pb, cuda, rank=8, ckpt=False):
    model = build_model(CFG._replace(activation_checkpointing=ckpt), pb, cuda, lora_rank=rank, lora_alpha=float(rank))
    for n, prm in model.named_parameters():
        if n.startswith(("tok_embeddings", "output", "norm")):
            prm.requires_grad_(False)
    return model


def _grads(model):
    return {n: q.grad.clone() for n, q in model.named_parameters() if q.grad is not None}


def test_layer_trains_through_a_scattered_mask(cuda):
    """The mask test_kv_cache_prefill_and_decode shows to raise through mask= (50 % random plus the diagonal), given as
    block_mask=MaskSpec(dense=...): output, dx and d attention_norm.weight against O.layer under autograd, at that test's bars."""
    from modelling.llama import MaskSpec

    pb, pf = bf16_params(O.init_params(CFG))
    model = build_model(CFG, pb, cuda)
    layer = model.layers[0]
    hid = O.randn("hidden1", (1, S, 512), 0.5).bfloat16()
    dy = O.randn("dense_dy", (1, S, 512), 0.1).bfloat16()
    g = torch.Generator().manual_seed(3)
    scattered = torch.rand(S, S, generator=g) < 0.5
    scattered |= torch.eye(S, dtype=torch.bool)
    assert bool(scattered.any(-1).all()) and int(scattered.triu(1).sum()) > 0
    xg = hid.to(cuda).requires_grad_()
    out = layer(xg, model.rope[:S], block_mask=MaskSpec(dense=scattered))
    out.backward(dy.to(cuda))
    xr = hid.float().requires_grad_()
    pr = {k: (v.clone().requires_grad_() if k.startswith("layers.0.") and k.endswith("_norm.weight") else v) for k, v in pf.items()}
    ref = O.layer(xr, pr, 0, CFG, O.rope_table(CFG)[:S], scattered[None, None])
    ref.backward(dy.float())
    _close(out.float().cpu(), ref.detach(), 0.03, "scattered dense mask: output")
    _close(xg.grad.float().cpu(), xr.grad, 0.05, "scattered dense mask: dx")
    _close(layer.attention_norm.weight.grad.float().cpu(), pr["layers.0.attention_norm.weight"].grad, 0.06, "d attention_norm.weight")


@pytest.fixture(scope="module")
def window_run(cuda):
    """The two-layer LoRA model (r 8) under a 100-wide sliding window: (parameters, tokens, labels, mask, loss, gradients)."""
    from modelling.llama import MaskSpec

    pb, pf = _lora_setup()
    tokens, labels = _data(2, S)
    mask = _window(S, 100)
    model = _lora_model(pb, cuda)
    loss = model(tokens.to(cuda), labels=labels.to(cuda), block_mask=MaskSpec(dense=mask))
    loss.backward()
    return pb, pf, tokens, labels, mask, loss.detach().clone(), _grads(model)


def test_lora_model_trains_through_a_sliding_window(cuda, window_run):
    pb, pf, tokens, labels, mask, loss, grads = window_run
    train = [k for k in pf if "lora_" in k or k.endswith("_norm.weight")]
    pr = {k: (v.clone().requires_grad_() if k in train else v) for k, v in pf.items()}
    ref = O.llama_forward(tokens, pr, CFG, mask=mask[None, None], labels=labels)
    ref.backward()
    print(f"[sliding window 100, S={S}] loss {loss.item():.5f} (oracle {ref.item():.5f})")
    assert abs(loss.item() - ref.item()) < 2e-3 * max(1.0, abs(ref.item())), (loss.item(), ref.item())
    seen = 0
    for name, g in grads.items():
        if "lora_a" in name or "lora_b" in name:
            seen += 1
            _close(g.float().cpu(), pr[name].grad, 0.04, name)
            _rows_close(g.float().cpu(), pr[name].grad, name, min_cos=0.995)
    assert seen == sum(1 for k in pf if "lora_" in k) > 0, seen


def test_checkpointing_is_bit_identical_under_a_dense_mask(cuda, window_run):
    from modelling.llama import MaskSpec

    pb, _, tokens, labels, mask, loss0, g0 = window_run
    model = _lora_model(pb, cuda, ckpt=True)
    assert model.config.activation_checkpointing
    loss = model(tokens.to(cuda), labels=labels.to(cuda), block_mask=MaskSpec(dense=mask))
    loss.backward()
    g1 = _grads(model)
    assert torch.equal(loss.detach(), loss0), (loss, loss0)
    assert g0.keys() == g1.keys() and len(g0) > 0
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_from_mask_mod_causal_equals_no_mask(cuda):
    """create_block_mask(causal_mask_mod) -> MaskSpec.from_mask_mod: the rule spec, hence the causal kernels - bit for bit."""
    from modelling.llama import MaskSpec

    pb, _ = _lora_setup()
    tokens, labels = _data(2, S)
    spec = MaskSpec.from_mask_mod(lambda b, h, q_idx, kv_idx: q_idx >= kv_idx, 2, S, cuda)
    assert spec.dense is None
    res = []
    for bm in (None, spec):
        model = _lora_model(pb, cuda)
        loss = model(tokens.to(cuda), labels=labels.to(cuda), block_mask=bm)
        loss.backward()
        res.append((loss.detach().clone(), _grads(model)))
    (l0, g0), (l1, g1) = res
    assert torch.equal(l0, l1)
    assert g0.keys() == g1.keys() and len(g0) > 0
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
