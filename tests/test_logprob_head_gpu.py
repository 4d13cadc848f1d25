"""GPU: ops.HeadLogprobFn (final norm + LM head + per-token log-probabilities) at T = 300, D = 512, with labels that hold a masked
prefix and a fully ignored stretch.

Vocabulary: V = 1000 wherever only a forward runs.  Every check that runs a backward uses V = 1024: the head's d-hidden GEMM contracts
over the vocabulary in 64-column steps, for HeadLossFn (which these checks compare with) and for the adapted / quantised plans alike,
so no head of this package has a backward at V = 1000 - HeadLogprobFn says so up front (test_gradients_need_a_vocabulary_of_64s)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ref as O  # noqa: E402

T, D, V_FWD, V_BWD = 300, 512, 1000, 1024
EPS = 1e-5


def _bf(x):
    return x.to(torch.bfloat16)


def _labels(V, prefix=64, hole=(150, 200)):
    lb = O.randint("lp_labels", (T,), 0, V)
    lb[prefix] = 0
    lb[prefix + 1] = V - 1
    lb[:prefix] = -100          # masked prompt
    lb[hole[0] : hole[1]] = -100  # a fully ignored stretch
    return lb


def _inputs(V):
    x = _bf(O.randn("lp_x", (T, D), 0.7))
    nw = _bf(1 + O.randn("lp_nw", (D,), 0.1))
    w = _bf(O.randn("lp_w", (V, D), 0.05))
    return x, nw, w


def _head(cuda, V, kind="plain"):
    """(norm, output) modules of the package on the GPU: a plain bf16 head, a LoRA r16 head or an int8 head."""
    from modelling import apply_linear_adapter_
    from modelling.llama import Linear, RMSNorm
    from subclasses import quantize_linear_

    _, nw, w = _inputs(V)
    norm, out = RMSNorm(D, eps=EPS).bfloat16(), Linear(D, V, bias=False).bfloat16()
    with torch.no_grad():
        norm.weight.copy_(nw)
        out.weight.copy_(w)
    if kind == "int8":
        quantize_linear_(out, "int8")
    if kind == "lora":
        apply_linear_adapter_(out, "lora", rank=16, alpha=16.0)
        with torch.no_grad():
            out.lora_a.copy_(_bf(O.randn("lp_a", (16, D), 0.04)))
            out.lora_b.copy_(_bf(O.randn("lp_b", (V, 16), 0.05)))
    return norm.to(cuda), out.to(cuda)


def _kernel_on_own_logits(norm, out, x, labels):
    """The forward kernel applied to the logits of output(norm(x)) on ALL rows."""
    from llx import kernels as K

    with torch.no_grad():
        logits = out(norm(x))
    logp, _, top1 = K.logprob_rows_fwd(logits, labels, want_top1=True)
    return logp, top1


@pytest.mark.parametrize("grad", [False, True])
def test_plain_frozen_head_equals_kernel_on_full_logits(cuda, grad):
    """The compacted route (gather -> row-limited GEMM -> kernel -> scatter) against the kernel on the logits of all rows: the two GEMMs
    share their per-row arithmetic, so the labelled positions agree bit for bit; 0.0 / -1 elsewhere.  With and without a graph."""
    from llx import ops

    V = V_BWD if grad else V_FWD
    norm, out = _head(cuda, V)
    out.weight.requires_grad_(False)
    norm.weight.requires_grad_(grad)
    x = _inputs(V)[0].to(cuda)
    lb = _labels(V).to(cuda)
    want, want_top1 = _kernel_on_own_logits(norm, out, x, lb)
    with torch.set_grad_enabled(grad):
        logp, top1 = ops.head_logprobs(x.clone().requires_grad_(grad), norm, out, lb, return_top1=True)
    assert logp.dtype is torch.float32 and logp.shape == (T,) and top1.dtype is torch.int32 and logp.requires_grad == grad
    assert not top1.requires_grad
    keep = lb != -100
    assert torch.equal(logp.detach()[keep], want[keep]) and torch.equal(top1[keep], want_top1[keep])
    assert (logp.detach()[~keep] == 0).all() and (top1[~keep] == -1).all()
    assert torch.equal(want[~keep], torch.zeros_like(want[~keep]))  # (the kernel itself: exact zeros on ignored rows)
    logp1 = ops.head_logprobs(x, norm, out, lb) if not grad else None  # without top1: the same values
    assert logp1 is None or torch.equal(logp1, logp)


def _loss_path(norm, out, x, lb):
    from llx import ops

    plan = ops.LinearPlan(out)
    xg = x.clone().requires_grad_()
    loss = ops.HeadLossFn.apply(xg, norm.weight, lb, norm.eps, plan, *plan.tensors())
    loss.backward()
    return loss.detach(), xg.grad


def _assert_grad_close(got, ref, name):
    eq = torch.equal(got, ref)
    err = (got.float() - ref.float()).abs().max().item()
    print(f"{name}: bit-identical {eq}, max |diff| {err:.3e} (max |ref| {ref.float().abs().max().item():.3e})")
    torch.testing.assert_close(got.float(), ref.float(), rtol=2 ** -7, atol=2 ** -7 * ref.float().abs().max().item(), msg=lambda m: f"{name}: {m}")


@pytest.mark.parametrize("trainable", [False, True])
def test_gradients_match_the_loss_path(cuda, trainable):
    """g = -1/count on the labelled rows makes sum(g * logp) the mean cross-entropy: dx, d norm_w (and dW of a trainable plain head) against
    HeadLossFn on the same inputs.  d logits is bf16(-1/count * (onehot - p)) here and bf16((p - onehot) * 1/count) there - the same
    number -, and d hidden / dW go through the same GEMM calls, so equality is the expectation (printed); the bar is rtol 2^-7,
    atol 2^-7 * max|ref|."""
    from llx import ops

    V = V_BWD
    norm, out = _head(cuda, V)
    out.weight.requires_grad_(trainable)
    x = _inputs(V)[0].to(cuda)
    lb = _labels(V).to(cuda)
    loss, dx_ref = _loss_path(norm, out, x, lb)
    dnw_ref, dw_ref = norm.weight.grad, out.weight.grad
    norm.weight.grad = out.weight.grad = None
    count = (lb != -100).sum()
    g = torch.where(lb != -100, -1.0 / count.float(), torch.zeros((), device=cuda))
    xg = x.clone().requires_grad_()
    logp = ops.head_logprobs(xg, norm, out, lb)
    torch.testing.assert_close(-logp.detach().sum() / count, loss, atol=1e-4, rtol=1e-5)
    logp.backward(g)
    _assert_grad_close(xg.grad, dx_ref, "dx")
    _assert_grad_close(norm.weight.grad, dnw_ref, "d norm_w")
    assert (xg.grad[lb == -100] == 0).all()
    if trainable:
        _assert_grad_close(out.weight.grad, dw_ref, "dW")
    else:
        assert out.weight.grad is None
    with pytest.raises(ops.LlxError):  # the saved logits became d logits: a second backward is refused, not computed from garbage
        xg2 = x.clone().requires_grad_()
        lp2 = ops.head_logprobs(xg2, norm, out, lb)
        lp2.backward(g, retain_graph=True)
        lp2.backward(g)


def test_per_row_gradient_matches_cpu_autograd(cuda):
    """Random per-row upstream gradients (some zero, some negative) against torch autograd on the CPU through the same rounding points:
    rmsnorm -> bf16 -> matmul -> bf16 logits -> fp32 log-softmax.  Bars of the rmsnorm / linear gradient tests of
    tests/test_kernels_gpu.py: atol 1e-2 * max|ref|, rtol 2e-2."""
    from llx import ops

    V = V_BWD
    norm, out = _head(cuda, V)
    out.weight.requires_grad_(False)
    x, nw, w = _inputs(V)
    lb = _labels(V)
    g = O.randn("lp_g", (T,), 1.0)
    g[::5] = 0.0
    assert (g < 0).any() and (g[lb != -100] == 0).any()
    xr, nwr = x.float().requires_grad_(), nw.float().requires_grad_()
    xn = (xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + EPS) * nwr).bfloat16().float()
    logits = (xn @ w.float().T).bfloat16().float()
    ref = -F.cross_entropy(logits, lb, reduction="none", ignore_index=-100)
    ref.backward(g)
    xg = x.to(cuda).requires_grad_()
    logp = ops.head_logprobs(xg, norm, out, lb.to(cuda))
    # forward against the CPU values: the two matmuls sum in different orders, so a logit may land on the neighbouring bf16 value - one ulp
    # of a logit below 8 is 2^-5 (|logits| stay below 8 here); the bar is two of them
    assert logits.abs().max() < 8
    torch.testing.assert_close(logp.detach().cpu(), ref.detach(), atol=2 ** -4, rtol=0)
    logp.backward(g.to(cuda))
    dx, dnw = xg.grad.float().cpu(), norm.weight.grad.float().cpu()
    torch.testing.assert_close(dx, xr.grad, atol=1e-2 * xr.grad.abs().max().item(), rtol=2e-2)
    torch.testing.assert_close(dnw, nwr.grad, atol=1e-2 * nwr.grad.abs().max().item(), rtol=2e-2)
    zero = (lb == -100) | (g == 0)
    assert (xg.grad.cpu()[zero] == 0).all() and (xr.grad[zero] == 0).all()


@pytest.mark.parametrize("kind", ["lora", "int8"])
def test_adapted_and_quantised_heads_take_the_generic_route(cuda, kind):
    """A LoRA r16 head and an int8 head: forward values equal the kernel on their own logits bit for bit (V = 1000), and the backward
    runs through the plan (V = 1024): finite, non-zero gradients, zero rows of dx at ignored positions."""
    from llx import ops

    norm, out = _head(cuda, V_FWD, kind)
    x = _inputs(V_FWD)[0].to(cuda)
    lb = _labels(V_FWD).to(cuda)
    want, want_top1 = _kernel_on_own_logits(norm, out, x, lb)
    with torch.no_grad():
        logp, top1 = ops.head_logprobs(x, norm, out, lb, return_top1=True)
    assert torch.equal(logp, want) and torch.equal(top1, want_top1)
    assert (logp[lb == -100] == 0).all() and (top1[lb == -100] == -1).all() and (logp[lb != -100] < 0).all()

    norm, out = _head(cuda, V_BWD, kind)
    x = _inputs(V_BWD)[0].to(cuda).requires_grad_()
    lb = _labels(V_BWD).to(cuda)
    want, _ = _kernel_on_own_logits(norm, out, x.detach(), lb)
    logp = ops.head_logprobs(x, norm, out, lb)
    assert torch.equal(logp.detach(), want)
    g = O.randn("lp_g", (T,), 1.0).to(cuda)
    logp.backward(g)
    grads = {"dx": x.grad, "d norm_w": norm.weight.grad}
    if kind == "lora":
        grads.update({"d lora_a": out.lora_a.grad, "d lora_b": out.lora_b.grad})
    for name, gr in grads.items():
        assert gr is not None and torch.isfinite(gr.float()).all() and gr.float().abs().max() > 0, name
    assert (x.grad[lb == -100] == 0).all() and (x.grad[lb != -100].float().abs().amax(1) > 0).all()


@pytest.mark.parametrize("kind", ["plain", "lora"])
def test_forced_chunks_are_bit_identical_under_no_grad(cuda, kind, monkeypatch):
    """The chunked walk of a row set beyond one logits buffer, forced at 256-row chunks (256 + 44 rows; 280 labelled rows, so the chunk
    boundary falls inside the compacted rows): one GEMM and one kernel launch per chunk, bit-identical to the single buffer.  With
    gradients a chunked row set is refused."""
    from llx import ops

    norm, out = _head(cuda, V_FWD, kind)
    x = _inputs(V_FWD)[0].to(cuda)
    lb = _labels(V_FWD, prefix=10, hole=(150, 160)).to(cuda)
    assert int((lb != -100).sum()) == 280
    res = {}
    for chunked in (False, True):
        monkeypatch.setattr(ops, "_HEAD_CHUNK_FORCED", chunked)
        monkeypatch.setattr(ops, "_HEAD_CHUNK_ROWS", 256)
        with torch.no_grad():
            res[chunked] = ops.head_logprobs(x, norm, out, lb, return_top1=True)
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    assert (res[True][0][lb != -100] < 0).all() and (res[True][0][lb == -100] == 0).all()
    norm_b, out_b = _head(cuda, V_BWD, kind)
    with pytest.raises(ops.LlxError, match="exceeds one logits buffer"):
        ops.head_logprobs(_inputs(V_BWD)[0].to(cuda).requires_grad_(), norm_b, out_b, _labels(V_BWD).to(cuda))


def test_gradients_need_a_vocabulary_of_64s(cuda):
    from llx import ops

    norm, out = _head(cuda, V_FWD)
    with pytest.raises(ops.LlxError, match="multiple of 64"):
        ops.head_logprobs(_inputs(V_FWD)[0].to(cuda).requires_grad_(), norm, out, _labels(V_FWD).to(cuda))
