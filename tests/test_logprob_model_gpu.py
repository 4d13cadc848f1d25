"""GPU: Llama.token_logprobs / LlamaAudio.token_logprobs on the tiny model (oracle.ref.TINY, LoRA r8 on the layers, frozen plain head,
B = 2, S = 256, labels with a masked prompt) against the forward kernel on the model's own logits, the loss path and the CPU oracle."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ref as O  # noqa: E402
from tests.util import _close, _rows_close, bf16_params, build_model  # noqa: E402

CFG = O.TINY
B, S = 2, 256


def _data(b=B, s=S):
    tokens = O.randint("tokens", (b, s), 0, CFG.vocab_size)
    labels = torch.roll(tokens, -1, 1).clone()
    labels[:, : s // 4] = -100  # masked prompt
    labels[:, -1] = -100
    return tokens, labels


@pytest.fixture(scope="module")
def setup(cuda):
    p = O.init_params(CFG)
    p.update(O.init_lora(CFG, 8))
    pb, pf = bf16_params(p)
    model = build_model(CFG, pb, cuda, lora_rank=8)
    for n, q in model.named_parameters():
        q.requires_grad_("lora_" in n)
    tokens, labels = _data()
    return model, pf, tokens, labels


def _lora_grads(model):
    out = {n: q.grad.clone() for n, q in model.named_parameters() if q.requires_grad}
    for q in model.parameters():
        q.grad = None
    return out


def test_no_grad_values(cuda, setup):
    """Bit for bit the forward kernel on model(tokens) at the labelled positions (the compacted and the full head GEMM share their per-row
    arithmetic), 0.0 / -1 elsewhere; against log_softmax of the oracle's logits within 0.03 of the oracle logits' scale - the bar the
    inference tests hold the logits themselves to."""
    from llx import kernels as K

    model, pf, tokens, labels = setup
    tk, lb = tokens.to(cuda), labels.to(cuda)
    for mode in (model.eval, model.train):
        mode()
        with torch.no_grad():
            logits = model(tk)
            logp, top1 = model.token_logprobs(tk, lb, return_top1=True)
            only = model.token_logprobs(tk, lb)
        assert logp.shape == (B, S) and logp.dtype is torch.float32 and top1.shape == (B, S) and top1.dtype is torch.int32
        assert torch.equal(only, logp)
        want, _, want_top1 = K.logprob_rows_fwd(logits.view(B * S, -1), lb.view(-1), want_top1=True)
        keep = lb != -100
        assert torch.equal(logp[keep], want.view(B, S)[keep]) and torch.equal(top1[keep], want_top1.view(B, S)[keep])
        assert (logp[~keep] == 0).all() and (top1[~keep] == -1).all()
        lf = logits.float()
        assert (lf.gather(-1, top1.long().clamp(min=0)[..., None])[..., 0][keep] == lf.max(-1).values[keep]).all()  # top1 holds the row maximum
    ref_logits = O.llama_forward(tokens, pf, CFG)
    ref = -F.cross_entropy(ref_logits.view(B * S, -1), labels.view(-1), reduction="none", ignore_index=-100).view(B, S)
    rel = 0.03 * ref_logits.abs().max().item() / ref.abs().max().item()  # _close scales by its reference: 0.03 of the LOGITS' scale
    _close(logp.cpu(), ref, rel, "token log-probabilities")


def test_mean_matches_loss_path(cuda, setup):
    """-sum(logp) / count is the loss of model(tokens, labels=labels) (atol 1e-4, rtol 1e-5), and the LoRA gradients of the two backward
    passes agree within rtol 2^-7, atol 2^-7 * max|ref|."""
    model, pf, tokens, labels = setup
    model.train()
    tk, lb = tokens.to(cuda), labels.to(cuda)
    loss = model(tk, labels=lb)
    loss.backward()
    ref = _lora_grads(model)
    logp = model.token_logprobs(tk, lb)
    assert logp.requires_grad
    mine = -logp.sum() / (lb != -100).sum()
    torch.testing.assert_close(mine.detach(), loss.detach(), atol=1e-4, rtol=1e-5)
    mine.backward()
    got = _lora_grads(model)
    assert got.keys() == ref.keys() and len(got) == 2 * 7 * CFG.num_layers
    for n in ref:
        torch.testing.assert_close(got[n].float(), ref[n].float(), rtol=2 ** -7, atol=2 ** -7 * ref[n].float().abs().max().item(), msg=lambda m: f"{n}: {m}")


def test_sequence_weights_match_oracle_autograd(cuda, setup):
    """Sequence weights (+1, -1) - a preference-pair shaped objective - against torch autograd through the oracle: LoRA gradients per
    row (tests/util._rows_close at its defaults)."""
    model, pf, tokens, labels = setup
    model.train()
    w = torch.tensor([1.0, -1.0])
    train = [k for k in pf if "lora_" in k]
    pr = {k: (v.clone().requires_grad_() if k in train else v) for k, v in pf.items()}
    ref_logits = O.llama_forward(tokens, pr, CFG)
    ref = -F.cross_entropy(ref_logits.view(B * S, -1), labels.view(-1), reduction="none", ignore_index=-100).view(B, S)
    (w[:, None] * ref).sum().backward()
    logp = model.token_logprobs(tokens.to(cuda), labels.to(cuda))
    (w.to(cuda)[:, None] * logp).sum().backward()
    got = _lora_grads(model)
    for n in train:
        g_, w_ = got[n].float().cpu(), pr[n].grad
        if g_.shape[1] < 16:  # a row of d lora_b has `rank` elements: compared along the other axis, as tests/util.layer_parity does
            g_, w_ = g_.T, w_.T
        _rows_close(g_, w_, n)


def test_audio_model_text_positions(cuda):
    """LlamaAudio.token_logprobs covers the text positions only (the audio prefix is dropped before the head, as in forward): [B, St],
    the kernel's values on the model's own logits; audio=None takes the plain embedding path."""
    from llx import kernels as K

    pb, _ = bf16_params(O.init_params(CFG, audio=True))
    model = build_model(CFG, pb, cuda, audio=True)
    audio = O.uniform("audio", (1, 32000), -0.1, 0.1).to(cuda)  # 2 s -> 100 audio tokens
    tokens, labels = _data(1, 128)
    tk, lb = tokens.to(cuda), labels.to(cuda)
    keep = lb != -100
    for au in (audio, None):
        with torch.no_grad():
            logits = model(au, tk)
            logp, top1 = model.token_logprobs(au, tk, lb, return_top1=True)
        assert logits.shape == (1, 128, CFG.vocab_size) and logp.shape == (1, 128) and top1.shape == (1, 128)
        want, _, want_top1 = K.logprob_rows_fwd(logits.reshape(128, -1), lb.view(-1), want_top1=True)
        assert torch.equal(logp[keep], want.view(1, 128)[keep]) and torch.equal(top1[keep], want_top1.view(1, 128)[keep])
        assert (logp[~keep] == 0).all() and (top1[~keep] == -1).all() and (logp[keep] < 0).all()


def test_bad_labels_are_refused(cuda, setup):
    from llx._lib import LlxError

    model, pf, tokens, labels = setup
    tk, lb = tokens.to(cuda), labels.to(cuda)
    with torch.no_grad():
        with pytest.raises(LlxError, match="shape"):
            model.token_logprobs(tk, lb[:, :-1])
        with pytest.raises(LlxError, match="shape"):
            model.token_logprobs(tk, lb.view(-1))
        with pytest.raises(LlxError, match="int64"):
            model.token_logprobs(tk, lb.to(torch.int32))
        with pytest.raises(LlxError):
            model.token_logprobs(tk, labels)  # CPU labels
        with pytest.raises(LlxError):
            model.token_logprobs(tokens, labels)  # CPU tokens and labels
