"""GPU: token_logprobs(top_k=k) and generate(return_logprobs=True, top_logprobs=k) on the tiny model (oracle.ref.TINY).

Scoring: logp and its gradients are bit for bit those of the call without top_k; top_ids[..., 0] is top1; an alternative that is the
label carries the label's logp bit for bit; ids and values agree with the host reference (tests/topk_cases.py) applied to the logits of
model(tokens) - ids exactly, on rows whose fifth and sixth largest logits differ (positions where they tie are taken out of the labels
up front, from those reference logits, and the test asserts that no labelled row ties: the tie rule hides nothing), values within the
project's bar between two paths, 0.03 * max |logit|.

Generation: tokens and logprobs are those of the call without top_logprobs; greedy tokens are top_ids[..., 0]; where the returned token
is among the alternatives its value is within 1e-5 of logprobs (the sampler sums the row in another order: log2(V) * 2^-24 ~ 1e-6
relative in the sum, ten times that); -1 / 0.0 after a row's eos; no host read inside a token."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref as O  # noqa: E402
from tests import topk_cases as C  # noqa: E402
from tests.util import bf16_params, build_model  # noqa: E402

CFG = O.TINY
V = CFG.vocab_size
B, S, KTOP = 2, 256, 5
P, N, KGEN = 40, 12, 3
LENS = (40, 17, 29)
SAMPLED = dict(temperature=0.8, top_p=0.9, seed=3)


def _tokens(b=B, s=S):
    tokens = O.randint("tokens", (b, s), 0, V)
    labels = torch.roll(tokens, -1, 1).clone()
    labels[:, : s // 4] = -100  # masked prompt
    labels[:, -1] = -100
    return tokens, labels


def _labels_without_boundary_ties(logits, labels, k=KTOP):
    """labels with the positions taken out whose k-th and k+1-th largest reference logits tie, plus one label per batch row moved onto
    the row's best token (so that a label among the alternatives occurs for sure)."""
    top = logits.float().topk(k + 1, dim=-1).values
    labels = labels.clone()
    labels[top[..., k - 1] == top[..., k]] = -100
    for b in range(labels.shape[0]):
        j = int((labels[b] != -100).nonzero()[3])
        labels[b, j] = int(logits[b, j].float().argmax())
    return labels


def _check_alternatives(logits, labels, logp, top1, top_ids, top_logp, k=KTOP):
    """The properties of the scoring results against the bf16 logits of model(tokens) (all on the host)."""
    lf = logits.float().reshape(-1, V)
    lb = labels.reshape(-1)
    keep = lb != -100
    top = lf.topk(k + 1, dim=-1).values
    assert keep.sum() > lb.numel() // 4 and (top[keep][:, k - 1] != top[keep][:, k]).all()  # no labelled row ties at the boundary
    ids, val = top_ids.reshape(-1, k), top_logp.reshape(-1, k)
    assert ids.dtype is torch.int32 and val.dtype is torch.float32 and not top_ids.requires_grad and not top_logp.requires_grad
    assert (ids[~keep] == -1).all() and (val[~keep] == 0).all()
    assert torch.equal(ids[:, 0], top1.reshape(-1))
    want_ids, want_val = C.top_logprobs_rows_ref(lf[keep], k)
    assert torch.equal(ids[keep], want_ids)
    bar = 0.03 * lf[keep].abs().max().item()
    worst = (val[keep].double() - want_val).abs().max().item()
    print(f"max |top_logp - fp64 on model(tokens)| = {worst:.3e} (bar {bar:.3e})")
    assert worst <= bar
    hit = (ids == lb[:, None].to(torch.int32)) & keep[:, None]
    assert hit.any(1).sum() >= labels.shape[0]
    assert torch.equal(val[hit], logp.reshape(-1)[:, None].expand(-1, k)[hit])  # the label's entry: bit for bit its logp


@pytest.fixture(scope="module")
def setup(cuda):
    p = O.init_params(CFG)
    p.update(O.init_lora(CFG, 8))
    pb, _ = bf16_params(p)
    model = build_model(CFG, pb, cuda, lora_rank=8)
    for n, q in model.named_parameters():
        q.requires_grad_("lora_" in n)
    tokens, labels = _tokens()
    tk = tokens.to(cuda)
    with torch.no_grad():
        logits = model.eval()(tk).cpu()
    labels = _labels_without_boundary_ties(logits, labels)
    return model, tk, labels.to(cuda), logits, labels


def test_scoring_no_grad(cuda, setup):
    model, tk, lb, logits, labels = setup
    with torch.no_grad():
        plain = model.token_logprobs(tk, lb, return_top1=True)
        logp, top1, top_ids, top_logp = model.token_logprobs(tk, lb, return_top1=True, top_k=KTOP)
        only = model.token_logprobs(tk, lb, top_k=KTOP)
        again = model.token_logprobs(tk, lb, top_k=KTOP)
    assert top_ids.shape == top_logp.shape == (B, S, KTOP)
    assert torch.equal(logp, plain[0]) and torch.equal(top1, plain[1])
    assert len(only) == 3 and torch.equal(only[0], logp) and torch.equal(only[1], top_ids) and torch.equal(only[2], top_logp)
    assert torch.equal(again[1], top_ids) and torch.equal(again[2], top_logp)
    _check_alternatives(logits, labels, logp.cpu(), top1.cpu(), top_ids.cpu(), top_logp.cpu())
    with torch.no_grad():
        one = model.token_logprobs(tk, lb, top_k=1)
        eight = model.token_logprobs(tk, lb, top_k=8)
    assert torch.equal(one[1][..., 0], top1) and torch.equal(eight[1][..., :KTOP], top_ids) and torch.equal(eight[2][..., :KTOP], top_logp)


def test_scoring_gradients_are_untouched(cuda, setup, monkeypatch):
    """With autograd the kernel runs in the forward, before the backward turns the logits into d logits in place: logp, the gradient of
    a LoRA factor and the gradient of the head's input are bit for bit those of the call without top_k."""
    model, tk, lb, logits, labels = setup
    hidden = []
    orig = model._hidden

    def keep_hidden(*a, **k):
        h = orig(*a, **k)
        h.retain_grad()
        hidden.append(h)
        return h

    monkeypatch.setattr(model, "_hidden", keep_hidden)
    g = O.randn("topk_g", (B, S), 1.0).to(cuda)
    res = {}
    for k in (0, KTOP):
        out = model.token_logprobs(tk, lb, return_top1=True, top_k=k)
        assert out[0].requires_grad and all(not t.requires_grad for t in out[1:])
        (out[0] * g).sum().backward()
        lora = model.layers[1].feed_forward.w2.lora_a
        res[k] = (out, lora.grad.clone(), hidden[-1].grad.clone())
        for q in model.parameters():
            q.grad = None
    assert torch.equal(res[KTOP][0][0], res[0][0][0]) and torch.equal(res[KTOP][0][1], res[0][0][1])
    assert res[0][1].float().abs().max() > 0 and res[0][2].float().abs().max() > 0
    assert torch.equal(res[KTOP][1], res[0][1]) and torch.equal(res[KTOP][2], res[0][2])
    logp, top1, top_ids, top_logp = (t.detach().cpu() for t in res[KTOP][0])
    _check_alternatives(logits, labels, logp, top1, top_ids, top_logp)


@pytest.mark.parametrize("kind", ["plain", "lora"])
def test_scoring_chunked_walk_and_lora_head(cuda, setup, monkeypatch, kind):
    """The chunked no_grad walk (forced at 256-row chunks: the boundary falls inside the labelled rows) gives the single buffer's results
    bit for bit; the same with a LoRA adapter on the head (the generic route: all rows, no compaction)."""
    from llx import ops
    from modelling import apply_linear_adapter_

    if kind == "plain":
        model, tk, lb, logits, labels = setup
    else:
        _, tk, _, _, _ = setup
        p = O.init_params(CFG)
        pb, _ = bf16_params(p)
        model = build_model(CFG, pb, "cpu")
        apply_linear_adapter_(model.output, "lora", rank=16, alpha=16.0)
        with torch.no_grad():
            model.output.lora_a.copy_(O.randn("topk_head_a", tuple(model.output.lora_a.shape), 0.04).to(torch.bfloat16))
            model.output.lora_b.copy_(O.randn("topk_head_b", tuple(model.output.lora_b.shape), 0.05).to(torch.bfloat16))
        model = model.to(cuda).eval()
        with torch.no_grad():
            logits = model(tk).cpu()
        labels = _labels_without_boundary_ties(logits, _tokens()[1])
        lb = labels.to(cuda)
    assert int((labels != -100).sum()) > 256
    res = {}
    for chunked in (False, True):
        monkeypatch.setattr(ops, "_HEAD_CHUNK_FORCED", chunked)
        monkeypatch.setattr(ops, "_HEAD_CHUNK_ROWS", 256)
        with torch.no_grad():
            res[chunked] = model.token_logprobs(tk, lb, return_top1=True, top_k=KTOP)
            plain = model.token_logprobs(tk, lb, return_top1=True)
        assert torch.equal(res[chunked][0], plain[0]) and torch.equal(res[chunked][1], plain[1])
    assert all(torch.equal(a, b) for a, b in zip(res[True], res[False]))
    _check_alternatives(logits, labels, *(t.cpu() for t in res[True]))


def test_scoring_audio_model(cuda):
    pb, _ = bf16_params(O.init_params(CFG, audio=True))
    model = build_model(CFG, pb, cuda, audio=True).eval()
    audio = O.uniform("audio", (1, 32000), -0.1, 0.1).to(cuda)
    tokens, labels0 = _tokens(1, 128)
    tk = tokens.to(cuda)
    for au in (audio, None):
        with torch.no_grad():
            logits = model(au, tk).cpu()
            labels = _labels_without_boundary_ties(logits, labels0)
            plain = model.token_logprobs(au, tk, labels.to(cuda), return_top1=True)
            out = model.token_logprobs(au, tk, labels.to(cuda), return_top1=True, top_k=KTOP)
        assert out[2].shape == (1, 128, KTOP) and torch.equal(out[0], plain[0]) and torch.equal(out[1], plain[1])
        _check_alternatives(logits, labels, *(t.cpu() for t in out))


def test_scoring_refuses_bad_top_k(cuda, setup):
    from llx._lib import LlxError

    model, tk, lb, _, _ = setup
    for bad in (-1, 9, 2.0, True, "3"):
        with torch.no_grad(), pytest.raises(LlxError, match="top_k must be an int in 0..8"):
            model.token_logprobs(tk, lb, top_k=bad)


# ---- generation ---------------------------------------------------------------------------------------------------------------------
_MODELS: dict = {}


def _gen_model(Bc, cuda, audio=False):
    if (Bc, audio) not in _MODELS:
        pb, _ = bf16_params(O.init_params(CFG, audio=True) if audio else O.init_params(CFG))
        model = build_model(CFG, pb, "cpu", audio=True) if audio else build_model(CFG, pb, "cpu")
        model.build_cache(inference=True, batch_size=Bc)
        _MODELS[(Bc, audio)] = model.to(cuda).eval()
    return _MODELS[(Bc, audio)]


def _prompts(Bc, cuda):
    if Bc == 1:
        return O.randint("generate_prompt", (1, P), 0, V).to(cuda), None
    return O.randint("generate_batch_prompts", (16, P), 0, V)[:Bc].to(cuda), [LENS[b % 3] for b in range(Bc)]


def _check_generated(plain, out, eos, greedy, k=KGEN):
    tokens, logprobs, top_ids, top_logp = (t.cpu() for t in out)
    assert torch.equal(tokens, plain[0].cpu()) and torch.equal(logprobs, plain[1].cpu())
    Bc, T = tokens.shape
    assert top_ids.shape == top_logp.shape == (Bc, T, k) and top_ids.dtype is torch.int32 and top_logp.dtype is torch.float32
    live = torch.ones(Bc, T, dtype=torch.bool)
    if eos is not None:
        for b in range(Bc):
            at = (tokens[b] == eos).nonzero()
            if at.numel():
                live[b, int(at[0]) + 1:] = False
    assert (top_ids[~live] == -1).all() and (top_logp[~live] == 0).all()
    assert (top_ids[live] >= 0).all() and (top_ids[live] < V).all()
    assert (top_logp[live][:, :-1] >= top_logp[live][:, 1:]).all() and (top_logp[live] < 0).all()  # descending log-probabilities
    if greedy:
        assert torch.equal(top_ids[..., 0][live].long(), tokens[live])
    hit = (top_ids.long() == tokens[..., None]) & live[..., None]
    assert not greedy or hit[..., 0][live].all()
    if hit.any():  # (a sampled token need not be among the three likeliest)
        worst = (top_logp[hit] - logprobs[..., None].expand(-1, -1, k)[hit]).abs().max().item()
        print(f"max |top_logp - logprobs| on {int(hit.sum())} returned tokens = {worst:.3e}")
        assert worst <= 1e-5
    return live


@pytest.mark.parametrize("Bc", [1, 3])
@pytest.mark.parametrize("sampling", [None, SAMPLED], ids=["greedy", "sampled"])
def test_generate_top_logprobs(cuda, Bc, sampling):
    model = _gen_model(Bc, cuda)
    prompt, lens = _prompts(Bc, cuda)
    kw = dict(prompt_lens=lens, return_logprobs=True, **(sampling or {}))
    free = model.generate(prompt, N, **kw)
    out = model.generate(prompt, N, top_logprobs=KGEN, **kw)
    assert isinstance(out, tuple) and len(out) == 4 and out[0].shape == (Bc, N)
    _check_generated(free, out, None, sampling is None)
    eos = int(free[0][0, 5])  # row 0 ends at its sixth token at the latest
    for every in (1, 16):
        plain = model.generate(prompt, N, eos_id=eos, check_every=every, **kw)
        stats_a, stats_b = {}, {}
        model.generate(prompt, N, eos_id=eos, check_every=every, stats=stats_a, **kw)
        out = model.generate(prompt, N, eos_id=eos, check_every=every, top_logprobs=KGEN, stats=stats_b, **kw)
        live = _check_generated(plain, out, eos, sampling is None)
        assert live[0].sum() <= 6
        if Bc > 1:
            assert live.sum(1).max() > live[0].sum()  # row 0 ends early, another row goes on
        assert {k: v for k, v in stats_a.items() if k != "counts"} == {k: v for k, v in stats_b.items() if k != "counts"}


def test_generate_top_logprobs_audio(cuda):
    Pa, Na, samples = 20, 8, 3200
    model = _gen_model(1, cuda, audio=True)
    audio = O.uniform("generate_audio_clips", (3, samples), -0.1, 0.1)[:1].to(cuda)
    prompt = O.randint("generate_audio_prompts", (3, Pa), 0, V, seed=1234)[:1].to(cuda)
    for au in (audio, None):
        plain = model.generate(au, prompt, Na, return_logprobs=True)
        out = model.generate(au, prompt, Na, return_logprobs=True, top_logprobs=KGEN)
        _check_generated(plain, out, None, True)


def test_generate_refusals_before_any_launch(cuda, monkeypatch):
    from llx import kernels as K
    from llx._lib import LlxError

    model = _gen_model(1, cuda)
    prompt, _ = _prompts(1, cuda)
    launched = []
    monkeypatch.setattr(K, "sample", lambda *a, **k: launched.append("sample"))
    monkeypatch.setattr(K, "topk_logprobs_rows", lambda *a, **k: launched.append("topk"))
    for kw, names in ((dict(top_logprobs=2), ("top_logprobs", "return_logprobs")),
                      (dict(top_logprobs=2, return_logprobs=True, num_beams=2), ("num_beams", "return_logprobs")),
                      (dict(top_logprobs=2, return_logprobs=True, draft_tokens=1), ("draft_tokens", "return_logprobs")),
                      (dict(top_logprobs=9, return_logprobs=True), ("top_logprobs", "0..8")),
                      (dict(top_logprobs=-1, return_logprobs=True), ("top_logprobs", "0..8")),
                      (dict(top_logprobs=2.0, return_logprobs=True), ("top_logprobs", "0..8"))):
        with pytest.raises(LlxError) as e:
            model.generate(prompt, N, **kw)
        assert all(n in str(e.value) for n in names), (kw, str(e.value))
    assert launched == []


@pytest.mark.parametrize("Bc", [1, 3])
def test_generate_no_host_read_inside_a_token(cuda, monkeypatch, Bc):
    """No item / tolist / synchronize beyond those of the call without top_logprobs."""
    model = _gen_model(Bc, cuda)
    prompt, lens = _prompts(Bc, cuda)
    kw = dict(prompt_lens=lens, return_logprobs=True, **SAMPLED)
    want = model.generate(prompt, N, top_logprobs=KGEN, **kw)
    unused = next(t for t in range(V) if t not in set(want[0].flatten().tolist()))
    calls = []
    item, tolist, sync = torch.Tensor.item, torch.Tensor.tolist, torch.cuda.synchronize
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (calls.append("item"), item(self))[1])
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (calls.append("tolist"), tolist(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (calls.append("sync"), sync(*a, **k))[1])
    counts = {}
    for k in (0, KGEN):
        calls.clear()
        out = model.generate(prompt, N, top_logprobs=k, **kw)
        counts[k, None] = list(calls)
        calls.clear()
        model.generate(prompt, N, eos_id=unused, check_every=4, top_logprobs=k, **kw)
        counts[k, 4] = list(calls)
    monkeypatch.undo()
    assert counts[KGEN, None] == counts[0, None] and counts[KGEN, 4] == counts[0, 4] and len(counts[0, 4]) <= math.ceil(N / 4)
    assert "item" not in counts[KGEN, None] and "sync" not in counts[KGEN, None]
    assert all(torch.equal(a, b) for a, b in zip(out, want))
