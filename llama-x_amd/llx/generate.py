"""Text generation on the KV-cache inference path: prefill, then one `model(...)` call and one sampler launch per token.

The reference names its `input_pos` branch "used for inference i.e. generate" (modelling/llama.py:204) and ships no generate();
this is that loop.  Nothing in it reads the device inside a token: the sampler (csrc/sample.hip) writes the next input token, appends
it to the history buffer and advances the position counter on the device, so the launch-bound decode path is never
stalled by an `.item()`.  With `eos_id` the host looks at the finished flag once every `check_every` tokens.

generate(draft_tokens=k) is the greedy loop with prompt-lookup drafts: a step feeds the last token and k draft tokens found in the sequence
itself as one k + 1-row call of the batch-1 decode path (llx/decode.py: up to four rows for one pass over the weights) and keeps the
prefix of the draft that the model confirms; accepting, appending and drafting are one launch of csrc/lookup.hip.

generate(num_beams=W) is beam search: the W beams of one prompt are the W rows of a batched decode step, and choosing the next beams, the
hypothesis bookkeeping and moving each surviving beam's keys and values to its cache slot are three launches of csrc/beam.hip (DESIGN
8.17).  generate(audio=clips) drives a LlamaAudio: clip and prompt are prefilled as one sequence, the decode steps feed text tokens.
"""
from __future__ import annotations

from contextlib import contextmanager
from typing import Optional, Sequence

import torch
from torch import Tensor

from . import decode as D
from . import kernels as K
from ._lib import LlxError
from .sampling import check_params, check_penalties, penalties_on

MAX_NGRAM = 8  # the longest n-gram a lookup draft matches (csrc/lookup.hip)


def _check(model, prompt: Tensor, max_new_tokens: int, eos_id, prefill_chunk, check_every, prompt_lens=None, draft=None, beams=None,
           audio=None) -> Optional[list]:
    """Raises LlxError on anything generate() cannot run, before any launch; returns the prompt lengths as a list (None: every row is P).
    draft: (draft_tokens, draft_ngram, temperature) of a call with draft_tokens != 0; beams: (num_beams, length_penalty, temperature,
    top_k, top_p, draft_tokens) of a call with num_beams != 1; audio: the clips of a call with audio."""
    from modelling.llama import Llama

    if not isinstance(model, Llama):
        raise LlxError(f"generate() drives a Llama or a LlamaAudio (got {type(model).__name__})")
    if model.training:
        raise LlxError("generate() needs the model in eval mode: call model.eval()")
    if any(layer.attention.kv_cache is None for layer in model.layers) or not hasattr(model, "causal_mask"):
        raise LlxError("generate() needs the KV cache: call model.build_cache(inference=True) first")
    if not (isinstance(prompt, Tensor) and prompt.dtype is torch.int64 and prompt.dim() == 2 and prompt.shape[0] >= 1 and prompt.shape[1] >= 1):
        raise LlxError("generate(): prompt must be an int64 tensor [B, P] with B, P >= 1")
    cache_b = model.layers[0].attention.kv_cache.k_cache.shape[0]
    if beams is not None:
        _check_beams(prompt, prompt_lens, cache_b, *beams)
    elif prompt.shape[0] != cache_b:
        raise LlxError(f"generate(): a batch of {prompt.shape[0]} prompts against a KV cache of batch {cache_b}: "
                       f"call model.build_cache(inference=True, batch_size={prompt.shape[0]})")
    lens = None
    if prompt_lens is not None:
        lens = prompt_lens.tolist() if isinstance(prompt_lens, Tensor) else list(prompt_lens)  # the one host read of the lengths
        if len(lens) != prompt.shape[0] or not all(isinstance(v, int) and not isinstance(v, bool) for v in lens):
            raise LlxError(f"prompt_lens must hold {prompt.shape[0]} integer lengths, one per row of prompt")
        if not all(1 <= v <= prompt.shape[1] for v in lens):
            raise LlxError(f"prompt_lens {lens} must lie in [1, {prompt.shape[1]}] (prompt is right-padded to P = {prompt.shape[1]})")
    if draft is not None:
        _check_draft(model, prompt, max_new_tokens, lens, *draft)
    n_audio = _check_audio(model, prompt, audio, prefill_chunk, draft) if audio is not None else 0
    if not prompt.is_cuda or model.tok_embeddings.weight.device != prompt.device:
        raise LlxError("generate() runs on the HIP device: model and prompt must be on the same GPU")
    if not (isinstance(max_new_tokens, int) and max_new_tokens >= 1):
        raise LlxError(f"max_new_tokens={max_new_tokens!r} must be an integer >= 1")
    longest = max(lens) if lens is not None else prompt.shape[1]
    if n_audio + longest + max_new_tokens > model.config.max_seq_len:
        raise LlxError(f"{f'audio ({n_audio} positions) + ' if audio is not None else ''}prompt ({longest}) + max_new_tokens ({max_new_tokens}) "
                       f"exceeds max_seq_len ({model.config.max_seq_len})")
    if eos_id is not None and not (isinstance(eos_id, int) and 0 <= eos_id < model.config.vocab_size):
        raise LlxError(f"eos_id={eos_id!r} must be a token id in [0, {model.config.vocab_size})")
    if prefill_chunk is not None and not (isinstance(prefill_chunk, int) and prefill_chunk >= 1):
        raise LlxError(f"prefill_chunk={prefill_chunk!r} must be None or an integer >= 1")
    if not (isinstance(check_every, int) and check_every >= 1):
        raise LlxError(f"check_every={check_every!r} must be an integer >= 1")
    return lens


def _check_beams(prompt: Tensor, prompt_lens, cache_b: int, W, length_penalty, temperature, top_k, top_p, draft_tokens) -> None:
    """The conditions of generate(num_beams=W), W != 1: one prompt, a cache slot per beam, and none of the arguments that choose tokens
    another way."""
    if not (isinstance(W, int) and not isinstance(W, bool) and 2 <= W <= D.MAX_BATCH):
        raise LlxError(f"num_beams={W!r} must be an integer in 1..{D.MAX_BATCH} (the beams of a step are the rows of one batched decode step)")
    if prompt.shape[0] != 1 or prompt_lens is not None:
        raise LlxError(f"num_beams={W} searches the continuations of one prompt: prompt [1, P] and no prompt_lens "
                       f"(got {prompt.shape[0]} rows, prompt_lens {prompt_lens!r})")
    if cache_b != W:
        raise LlxError(f"num_beams={W} against a KV cache of batch {cache_b}: every beam has a cache slot, "
                       f"call model.build_cache(inference=True, batch_size={W})")
    if temperature != 0 or top_k != 0 or top_p != 1:
        raise LlxError(f"num_beams={W} ranks hypotheses by their log-probability: temperature={temperature!r}, top_k={top_k!r} and "
                       f"top_p={top_p!r} must stay 0, 0 and 1")
    if draft_tokens != 0:
        raise LlxError(f"num_beams={W} cannot be combined with draft_tokens={draft_tokens!r}: a draft step holds the rows of one sequence")
    if not (isinstance(length_penalty, (int, float)) and not isinstance(length_penalty, bool) and length_penalty - length_penalty == 0):
        raise LlxError(f"length_penalty={length_penalty!r} must be a finite number (final score = log-probability / length ** length_penalty)")


def _check_audio(model, prompt: Tensor, audio, prefill_chunk, draft) -> int:
    """The conditions of generate(audio=...); returns the number of positions the clips take in front of the prompt."""
    from modelling.audio import LlamaAudio

    if not isinstance(model, LlamaAudio):
        raise LlxError(f"audio= needs a LlamaAudio (got {type(model).__name__})")
    if not (isinstance(audio, Tensor) and audio.dtype is torch.float32 and audio.dim() == 2 and audio.shape[0] == prompt.shape[0]
            and audio.shape[1] >= model.audio_config.hop_length):
        raise LlxError(f"audio must be an fp32 tensor [B, samples] with B = {prompt.shape[0]} rows, one clip of at least "
                       f"{model.audio_config.hop_length} samples per prompt")
    if prefill_chunk is not None:
        raise LlxError(f"prefill_chunk={prefill_chunk!r} with audio: the clip and the prompt are prefilled as one call")
    if draft is not None:
        raise LlxError(f"draft_tokens={draft[0]!r} with audio: drafting drives a text sequence")
    if audio.device != prompt.device:
        raise LlxError("generate(): audio and prompt must be on the same device")
    return model.audio_positions(audio.shape[1])


def _caller(model):
    """call(tokens, input_pos): one call of the model on the inference path.  A LlamaAudio takes the clip first; decode steps have none."""
    from modelling.audio import LlamaAudio

    if isinstance(model, LlamaAudio):
        return lambda tok, pos: model(None, tok, input_pos=pos)
    return lambda tok, pos: model(tok, input_pos=pos)


def _check_draft(model, prompt: Tensor, max_new_tokens, lens, k, g, temperature) -> None:
    """The conditions of generate(draft_tokens=k): greedy, one sequence, and room in the cache for the rows a draft step writes."""
    if not (isinstance(k, int) and not isinstance(k, bool) and 0 <= k <= D.MAX_TOKENS - 1):
        raise LlxError(f"draft_tokens={k!r} must be an integer in 0..{D.MAX_TOKENS - 1} (a decode step takes {D.MAX_TOKENS} rows)")
    if not (isinstance(g, int) and not isinstance(g, bool) and 1 <= g <= MAX_NGRAM):
        raise LlxError(f"draft_ngram={g!r} must be an integer in 1..{MAX_NGRAM}")
    if temperature != 0:
        raise LlxError(f"draft_tokens={k} needs temperature == 0 (got {temperature!r}): drafting confirms greedy picks; a sampled draft would "
                       "change the random stream")
    P = prompt.shape[1]
    if prompt.shape[0] != 1 or (lens is not None and lens != [P]):
        raise LlxError(f"draft_tokens={k} drives one sequence: a cache of batch 1 and prompt_lens None or [{P}] "
                       f"(got a batch of {prompt.shape[0]}, prompt_lens {lens})")
    if isinstance(max_new_tokens, int) and P + max_new_tokens + k > model.config.max_seq_len:
        # a step writes keys and values at positions up to len - 1 + k <= P + max_new_tokens - 1 + k, and the decode path does not check
        # positions against the cache: this bound is what keeps those writes inside it
        raise LlxError(f"prompt ({P}) + max_new_tokens ({max_new_tokens}) + draft_tokens ({k}) exceeds max_seq_len ({model.config.max_seq_len}): "
                       "a draft step writes cache rows up to k positions past the last token")


# ---- history bookkeeping of a batch with prompts of different lengths (pure: no device, no model)
def history_plan(lens: Sequence[int], n: int) -> tuple[int, int, list]:
    """(columns, hist_base, shifts) of the sampler's history buffer for prompt lengths `lens` and `n` new tokens.  The sampler writes the
    token drawn at counter pos to column pos - hist_base with ONE base for all rows; row b's first draw is at pos = lens[b] - 1, so with
    hist_base = min(lens) - 1 its k-th token lands in column shifts[b] + k, shifts[b] = lens[b] - min(lens), and max - min + n columns
    hold every row."""
    lo = min(lens)
    return max(lens) - lo + n, lo - 1, [v - lo for v in lens]


def history_column(lens: Sequence[int], b: int, k: int) -> int:
    """Column of the k-th generated token (k = 0 ..) of row b in the history buffer of history_plan."""
    return lens[b] - min(lens) + k


def history_rows(history: Tensor, shifts, counts: Tensor, T: int, pad: int) -> Tensor:
    """[B, T]: row b of `history` shifted left by shifts[b], its first counts[b] tokens kept and the rest filled with `pad`."""
    B = history.shape[0]
    j = torch.arange(T, device=history.device)
    sh = torch.as_tensor(shifts, device=history.device, dtype=torch.int64).view(B, 1)
    got = history.gather(1, (sh + j).clamp_(max=history.shape[1] - 1))
    return torch.where(j < counts.view(B, 1), got, torch.full_like(got, pad))


def history_rows_k(history: Tensor, shifts, counts: Tensor, T: int, pad) -> Tensor:
    """history_rows for a [B, cols, k] buffer (the top-k alternatives): [B, T, k], the shift and the cut along the columns."""
    B, _, k = history.shape
    j = torch.arange(T, device=history.device)
    sh = torch.as_tensor(shifts, device=history.device, dtype=torch.int64).view(B, 1)
    got = history.gather(1, (sh + j).clamp_(max=history.shape[1] - 1)[:, :, None].expand(B, T, k))
    return torch.where((j < counts.view(B, 1))[:, :, None], got, torch.full_like(got, pad))


class _TopLogprobs:
    """The buffers of generate(top_logprobs=k): ids int32 / logp fp32 [B, cols, k] in the geometry of the sampler's history, prefilled
    with -1 / 0.0, and the one extra launch of a step - BEFORE the step's sampler launch, so that it reads the position counter and
    the finished flags the sampler is about to use and writes the column the sampler then fills."""

    def __init__(self, k: int, B: int, cols: int, dev):
        self.k = k
        self.ids = torch.full((B, cols, k), -1, device=dev, dtype=torch.int32)
        self.logp = torch.zeros(B, cols, k, device=dev, dtype=torch.float32)

    def step(self, logits: Tensor, kw: dict) -> None:
        if logits.dtype is not torch.bfloat16:
            raise LlxError(f"generate: top_logprobs ranks bf16 logits (the model returned {logits.dtype})")
        K.topk_logprobs_rows(logits, self.k, pos=kw["pos"], hist_base=kw["hist_base"], finished=kw["finished"], ids=self.ids, logp=self.logp)


def seed_counts(prompt: Tensor, lens: Optional[Sequence[int]], vocab_size: int, penalize_prompt: bool) -> Tensor:
    """The sampler's count table (int32 [B, V], rule 0 of llx/sampling.py) before the first draw: zero, or with penalize_prompt the number
    of times each token occurs in row b's own prompt - its first lens[b] columns (None: all); pads are not counted.  No host read."""
    B, P = prompt.shape
    table = torch.zeros(B, vocab_size, device=prompt.device, dtype=torch.int32)
    if penalize_prompt:
        if lens is None:
            real = torch.ones(B, P, device=prompt.device, dtype=torch.int32)
        else:
            real = (torch.arange(P, device=prompt.device)[None] < torch.tensor(lens, device=prompt.device, dtype=torch.int64)[:, None]).to(torch.int32)
        table.scatter_add_(1, prompt.clamp(0, vocab_size - 1), real)
    return table


@torch.no_grad()
def prefill(model, prompt: Tensor, prompt_lens: Optional[Sequence[int]] = None, prefill_chunk: Optional[int] = None) -> Tensor:
    """Fill the KV cache from `prompt` (int64 [B, P], right-padded; B = the cache's batch) and return the logits [B, 1, V] of each
    sequence's last prompt token (row prompt_lens[b] - 1).  Positions 0 .. P-1 are shared by the batch: under the causal mask no
    prompt token attends to a pad, which comes later, and the keys and values a pad leaves at positions >= prompt_lens[b] are
    overwritten by sequence b's own decode step at that position before anything attends to them.  The [B, P, V] logits are never
    built: the layers run, one hidden row per sequence is gathered, the head runs on [B, 1, D]."""
    if prompt_lens is not None:
        prompt_lens = prompt_lens.tolist() if isinstance(prompt_lens, Tensor) else list(prompt_lens)
        prompt = prompt[:, : max(prompt_lens)]  # columns that are padding in every row are not run (P may exceed max_seq_len, the prompts may not)
    dev, (B, P) = prompt.device, prompt.shape
    chunk = P if prefill_chunk is None else prefill_chunk
    positions = torch.arange(P, device=dev)
    last = (torch.tensor(prompt_lens, device=dev, dtype=torch.int64) if prompt_lens is not None else torch.full((B,), P, device=dev)) - 1
    hidden = None
    table = model.rope  # a chunk runs with the table shifted to its first position (see generate below)
    try:
        for s in range(0, P, chunk):
            model.rope = table[s:]
            h = model._hidden(prompt[:, s : s + chunk], positions[s : s + chunk])  # [B, c, D]
            c = h.shape[1]
            idx = (last - s).clamp(0, c - 1).view(B, 1, 1).expand(B, 1, h.shape[2])
            rows = h.gather(1, idx)
            inside = ((last >= s) & (last < s + c)).view(B, 1, 1)
            hidden = rows if hidden is None else torch.where(inside, rows, hidden)
    finally:
        model.rope = table
    return model._head(hidden.contiguous(), None)


def prefill_audio(model, audio: Tensor, prompt: Tensor, prompt_lens: Optional[Sequence[int]] = None) -> Tensor:
    """prefill() for a LlamaAudio with clips: one model(audio, prompt, input_pos=arange(A + P)) call under the causal mask, A = the
    positions of the clips; the text tokens sit at A .. A + P - 1.  Returns the logits [B, 1, V] of each sequence's last prompt token."""
    if prompt_lens is not None:
        prompt = prompt[:, : max(prompt_lens)]
    B, P = prompt.shape
    A = model.audio_positions(audio.shape[1])
    logits = model(audio, prompt, input_pos=torch.arange(A + P, device=prompt.device))  # [B, P, V]: the audio positions are dropped
    if prompt_lens is None:
        return logits[:, -1:]
    last = torch.tensor(prompt_lens, device=prompt.device, dtype=torch.int64) - 1
    return logits.gather(1, last.view(B, 1, 1).expand(B, 1, logits.shape[2]))


def _generate_batch(model, prompt: Tensor, n: int, lens: list, sampling: dict, eos_id, prefill_chunk, check_every: int, call,
                    audio: Optional[Tensor] = None, table: Optional[Tensor] = None, return_logprobs: bool = False, top_logprobs: int = 0):
    """The loop of a batch.  sampling: the sampler's keyword arguments, penalties included; table: its count table (None: no penalties),
    seeded by the caller from each row's own text prompt; return_logprobs: also the fp32 log-probabilities, laid out like the tokens;
    top_logprobs = k > 0: also the k likeliest tokens and their log-probabilities [B, T, k]."""
    dev, B = prompt.device, prompt.shape[0]
    if audio is not None:
        logits = prefill_audio(model, audio, prompt, lens)
        A = model.audio_positions(audio.shape[1])
        lens = [A + v for v in lens]  # from here on a length is the sequence's: clip and prompt
    else:
        logits = prefill(model, prompt, lens, prefill_chunk)
    cols, base, shifts = history_plan(lens, n)
    start = torch.tensor(lens, device=dev, dtype=torch.int64) - 1
    pos = start.clone()  # per row: the position of the logits row being sampled from = the draw counter; the sampler advances it
    tok = torch.empty(B, 1, device=dev, dtype=torch.int64)
    history = torch.zeros(B, cols, device=dev, dtype=torch.int64)
    finished = torch.zeros(B, device=dev, dtype=torch.int32) if eos_id is not None else None
    kw = dict(**sampling, pos=pos, out=tok.view(B), history=history, hist_base=base, advance=True, eos_id=eos_id, finished=finished)
    if table is not None:
        kw["counts"] = table
    if return_logprobs:
        kw["logprob_history"] = torch.zeros(B, cols, device=dev, dtype=torch.float32)
    top = _TopLogprobs(top_logprobs, B, cols, dev) if top_logprobs else None
    if top is not None:
        top.step(logits[:, 0], kw)
    K.sample(logits[:, 0], **kw)
    T = n
    for k in range(1, n + 1):
        if finished is not None and (k % check_every == 0 or k == n):
            # one host read: a finished row stops advancing, so pos - start is every row's length (eos included); all rows finished
            # or the budget used up ends the loop, and the longest row is the width of the result
            state = int(((pos - start).max() * 2 + finished.min()).item())
            if state & 1 or k == n:
                T = state >> 1
                break
        if k == n:
            break
        # a finished row feeds eos_id at its frozen position: it re-writes its own cache row there, nothing else
        logits = call(tok, pos[:, None])[:, 0]
        if top is not None:
            top.step(logits, kw)
        K.sample(logits, **kw)
    counts = pos - start if finished is not None else torch.full((B,), n, device=dev, dtype=torch.int64)
    tokens = history_rows(history, shifts, counts, T, eos_id if eos_id is not None else 0)
    if top is not None:
        return (tokens, history_rows(kw["logprob_history"], shifts, counts, T, 0.0), history_rows_k(top.ids, shifts, counts, T, -1),
                history_rows_k(top.logp, shifts, counts, T, 0.0))
    return (tokens, history_rows(kw["logprob_history"], shifts, counts, T, 0.0)) if return_logprobs else tokens


# ---- greedy decoding with prompt-lookup drafts (generate(draft_tokens=k)): several rows of one sequence per step
@contextmanager
def decode_rope(model):
    """While active, `model.rope` is a contiguous fp32 [4, head_dim / 2, 2] buffer that holds the table's row 0 four times; the table is
    back afterwards, also on an exception.  forward rotates a call's rows by rope[:L], the index in the call (the reference's
    modelling/llama.py:207), so the one-row decode steps of a plain loop rotate every generated token by row 0.  A step that feeds
    several rows of the same sequence must rotate each of them by that row too, or drafting would change the result."""
    table = model.rope
    model.rope = table[:1].float().expand(D.MAX_TOKENS, -1, -1).contiguous()
    try:
        yield
    finally:
        model.rope = table


def _draft_rows(model, k: int, dev) -> int:
    """k, lowered to the largest k' for which the decode fast path takes a k' + 1-row step, if it takes a one-row step of this model
    at all (a model on the generic path runs any number of rows there).  Probes only: nothing is launched."""
    def fast(rows: int) -> bool:
        x = torch.empty(1, rows, model.config.embed_dim, device=dev, dtype=model.tok_embeddings.weight.dtype)
        mask = model.causal_mask[None, None, :rows]
        return all(D.layer_ok(layer, x, mask) for layer in model.layers) and D.head_ok(model, x)

    if not fast(1):
        return k
    while k > 0 and not fast(k + 1):
        k -= 1
    return k


def _generate_draft(model, prompt: Tensor, logits: Tensor, n: int, k: int, g: int, eos_id, check_every: int, stats, call) -> Tensor:
    """The decode loop of generate(draft_tokens=k) after the prefill (`logits`: the prefill's last call).  Per step: one model call on the
    k + 1 rows of step_tok at step_pos, one sampler launch (the greedy pick of every row), one llx_lookup_step launch (accept, append,
    draft, the next step's rows) - nothing reads the host."""
    dev, P = prompt.device, prompt.shape[1]
    seq = torch.empty(P + n, device=dev, dtype=torch.int64)  # the prompt, then the generated tokens
    seq[:P] = prompt[0]
    st = torch.zeros(3, device=dev, dtype=torch.int64)  # len | steps, accepted
    length, counters = st[:1], st[1:]
    length.fill_(P)
    finished = torch.zeros(1, device=dev, dtype=torch.int32)
    step_tok = torch.zeros(k + 1, device=dev, dtype=torch.int64)
    step_pos = torch.zeros(k + 1, device=dev, dtype=torch.int64)
    picks = torch.empty(k + 1, device=dev, dtype=torch.int64)
    draw = torch.zeros(k + 1, device=dev, dtype=torch.int64)  # the sampler's draw counter: not used at temperature 0
    kw = dict(P=P, n=n, k=k, g=g, eos_id=eos_id)
    K.sample(logits[0, -1:], temperature=0.0, pos=draw[:1], out=picks[:1])
    K.lookup_step(picks, seq, length, step_tok, step_pos, finished, counters, init=True, **kw)
    with decode_rope(model):
        for s in range(1, n + 1):
            if s % check_every == 0 or s == n:
                # one host read.  Every step that is not frozen emits a token, so after n - 1 steps the sequence is done at the latest.
                total, steps, accepted, fin = torch.cat((st, finished.to(torch.int64))).tolist()
                if fin or total == P + n or s == n:
                    break
            K.sample(call(step_tok[None], step_pos)[0], temperature=0.0, pos=draw, out=picks)
            K.lookup_step(picks, seq, length, step_tok, step_pos, finished, counters, **kw)
    if stats is not None:
        stats.update(steps=steps, tokens=total - P, accepted=accepted, draft_tokens=k, launched=s - 1,
                     state=dict(seq=seq, len=length, step_tok=step_tok, step_pos=step_pos, finished=finished, counters=counters))
    return seq[None, P:total]


# ---- beam search (generate(num_beams=W)): the W beams of one prompt are the W rows of a batched decode step
def _generate_beam(model, call, prompt: Tensor, audio, n: int, W: int, length_penalty: float, eos_id, prefill_chunk, check_every: int,
                   stats) -> Tensor:
    """The loop of generate(num_beams=W).  The prompt (and the clip) is prefilled in all W cache slots; per step: one model call on tok
    [W, 1] at the shared position, then beam_rows (the shortlists), beam_merge (the walk and all bookkeeping) and kv_reorder_rows (slot b
    takes over the keys and values of its parent) - nothing reads the host.  The beams' token k sits at position base + k - 1."""
    dev = prompt.device
    if audio is not None:
        logits = prefill_audio(model, audio.expand(W, -1).contiguous(), prompt.expand(W, -1).contiguous())[:, 0]
        base = model.audio_positions(audio.shape[1]) + prompt.shape[1]
    else:
        logits = prefill(model, prompt.expand(W, -1).contiguous(), None, prefill_chunk)[:, 0]
        base = prompt.shape[1]
    cand_score = torch.empty(W, W + 1, device=dev, dtype=torch.float32)
    cand_token = torch.empty(W, W + 1, device=dev, dtype=torch.int32)
    s = torch.zeros(W, device=dev, dtype=torch.float32)
    parent = torch.zeros(W, device=dev, dtype=torch.int32)
    tok = torch.zeros(W, 1, device=dev, dtype=torch.int64)
    hist = torch.zeros(W, n, device=dev, dtype=torch.int64)
    bank_tok = torch.zeros(W, n, device=dev, dtype=torch.int64)
    bank_len = torch.zeros(W, device=dev, dtype=torch.int32)
    bank_score = torch.zeros(W, device=dev, dtype=torch.float32)
    meta = torch.zeros(3, device=dev, dtype=torch.int32)  # hypotheses in the bank, done, tokens generated
    table = K.kv_cache_table(c for layer in model.layers for c in (layer.attention.kv_cache.k_cache, layer.attention.kv_cache.v_cache))
    positions = torch.arange(base, base + n, device=dev)
    state = (cand_score, cand_token, s, parent, tok, hist, bank_tok, bank_len, bank_score, meta)
    kw = dict(n=n, eos_id=eos_id, length_penalty=length_penalty)
    K.beam_rows(logits, cand_score, cand_token)
    K.beam_merge(*state, init=True, **kw)  # all slots hold the same keys and values: nothing to move
    for k in range(1, n + 1):
        # without an eos_id nothing finishes early: the n-th merge sets done.  With one, one host read every check_every steps; a done
        # state is frozen, the steps launched since then moved nothing
        if k == n or (eos_id is not None and k % check_every == 0 and int(meta[1].item())):
            break
        K.beam_rows(call(tok, positions[k - 1 : k])[:, 0], cand_score, cand_token)
        K.beam_merge(*state, **kw)
        K.kv_reorder_rows(table, parent, base + k)
    # the one read that ends the loop (token ids and lengths are exact in fp64)
    count, _, steps, *rest = torch.cat((meta.double(), bank_len.double(), bank_score.double(), bank_tok.flatten().double())).tolist()
    count = int(count)
    lens, scores, toks = rest[:W], rest[W : 2 * W], rest[2 * W :]
    order = sorted(range(count), key=lambda i: (-scores[i], i))
    beams = [([int(t) for t in toks[i * n : i * n + int(lens[i])]], scores[i]) for i in order]
    if stats is not None:
        stats.update(steps=int(steps), tokens=len(beams[0][0]), accepted=0, draft_tokens=0, launched=k - 1, num_beams=W, beams=beams)
    return torch.tensor(beams[0][0], dtype=torch.int64)[None].to(dev)


@torch.no_grad()
def generate(model, prompt: Tensor, max_new_tokens: int, *, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0,
             eos_id: Optional[int] = None, prefill_chunk: Optional[int] = None, check_every: int = 16, prompt_lens=None,
             draft_tokens: int = 0, draft_ngram: int = 3, stats: Optional[dict] = None, num_beams: int = 1, length_penalty: float = 1.0,
             audio: Optional[Tensor] = None, repetition_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
             penalize_prompt: bool = True, return_logprobs: bool = False, top_logprobs: int = 0):
    """Continue `prompt` (int64 [B, P], B = the batch the KV cache was built for) by up to `max_new_tokens` tokens -> int64 [B, n_new] on
    the prompt's device.  `prompt_lens` (B lengths in [1, P], a sequence or an int64 tensor, read once on the host before the first
    launch): the rows of `prompt` are right-padded prompts of these lengths; default: every row is P long.  For a batch the result is as
    wide as the longest row; with `eos_id` a row that ended earlier is padded with `eos_id`, and the loop stops when every row has
    ended.  The draw also takes the row index, and row r does not depend on what the other rows hold.  The decode steps of 2..16 sequences
    with bf16 or dynamic-int8 un-adapted linears stream every weight once for the whole batch (llx/decode.py); a single sequence streams
    bf16 and int8 linears with or without LoRA, and bf16 DoRA linears through their cached row factors (decode.prepare builds them here,
    before the prefill); anything else runs the generic path.

    The draw for the token at absolute position q uses the counter q - 1 (the position of the logits row it is sampled from), so the
    same arguments give the same tokens whatever `prefill_chunk` and `check_every` are.  With `eos_id` the result ends at the first
    `eos_id`, inclusive.

    The host learns of an `eos_id` only at the next `check_every` boundary: until then the loop keeps launching decode steps (up to
    `check_every - 1` of them), each feeding `eos_id` at the position counter, which no longer advances.  The returned tokens are not
    affected, but after an early stop the cache row at the position that follows the `eos_id` holds that token's keys and values rather
    than nothing.  While a prefill chunk runs, `model.rope` is a shifted view of the table (restored before the first decode step, also
    on an exception): do not drive the same model from another thread meanwhile.

    `draft_tokens` = k in 1..3 (greedy only, one sequence, P + max_new_tokens + k <= max_seq_len; 0, the default, is the loop above):
    prompt-lookup drafting.  Each decode step feeds the last token and k draft tokens as one k + 1-row call - the weights stream once for
    all rows - and keeps the longest prefix of the draft that the model's own greedy picks confirm, so a step yields 1 .. k + 1 tokens.
    The draft is what followed the most recent earlier occurrence of the last `draft_ngram` .. 1 tokens in the sequence itself (the longest
    n-gram that occurs wins; sampling.lookup_draft).  The result is the greedy continuation: only the number of weight passes changes (a
    row's logits may differ in the last bits between a one-row and a k + 1-row step, so a near-tie may fall the other way).  `eos_id`,
    `check_every` and `prefill_chunk` keep their meaning; the host looks at the device once every `check_every` steps, also without an
    `eos_id`, because the number of steps is not known in advance.  Between looks the device state is frozen once the sequence is done:
    the extra steps feed the same tokens at the same positions and rewrite the same cache rows with the same values.  If the decode fast
    path (llx/decode.py) takes a one-row step of this model but not a k + 1-row one, k is lowered to the largest row count it takes (0:
    the plain loop).  Afterwards the cache rows 0 .. P + len(result) - 2 hold the keys and values of the sequence; later rows, up to
    P + len(result) - 1 + k, may hold those of rejected drafts.  While the decode steps run, `model.rope` is decode_rope's table.

    `stats` (a dict) receives, from the one host read that ends the loop: "steps" (model calls that yielded tokens, the prefill's last row
    counted as one), "tokens" (= len(result)), "accepted" (draft tokens in the result: tokens - steps), "draft_tokens" (the k that ran)
    and "launched" (decode steps launched, the frozen ones included); with drafting also "state", the device tensors of the loop (seq,
    len, step_tok, step_pos, finished, counters), not read.  Without drafting the numbers come from the loop itself, without a read.

    `num_beams` = W in 2..16 (one prompt [1, P], a cache built with batch_size=W, greedy arguments only; 1, the default, is everything
    above): beam search by the rule of sampling.beam_step.  The W beams are the W rows of one batched decode step at a
    shared position, so a step streams the weights once; choosing the next beams, the bookkeeping and moving every surviving beam's keys
    and values to its cache slot are three launches (csrc/beam.hip), nothing is read by the host inside a step, and the done flag is
    read once every `check_every` steps.  A hypothesis that ends in `eos_id` is ranked by log-probability / length ** `length_penalty`
    (the eos counted); the search ends when W hypotheses have finished or after `max_new_tokens` tokens, when the live beams are ranked
    the same way.  The result is the best hypothesis, int64 [1, T], ending at its eos inclusive; `stats` also receives "beams": every
    hypothesis kept as (tokens, final score), best first.  The prompt is prefilled in all W slots.

    `audio` (fp32 [B, samples], with a LlamaAudio; LlamaAudio.generate(audio, prompt, n) is the method form): the clips are prefilled
    in front of the prompts as one call under the causal mask and take A = model.audio_positions(samples) positions, so the text sits at
    A .. A + P - 1, A + P + max_new_tokens <= max_seq_len, and the draw counter of a sampled token is its position, A included.  The
    decode steps feed text tokens only.  `prefill_chunk` and `draft_tokens` are refused with audio; without it a LlamaAudio generates
    as a text model.

    `repetition_penalty` (finite, > 0, 1 = off), `presence_penalty` and `frequency_penalty` (finite, 0 = off) shape the distribution a
    token is chosen from - greedy included - by rule 0 of llx/sampling.py: with c the number of times a token has occurred in the row's
    sequence so far, a logit x with c > 0 becomes x / repetition_penalty if x > 0 else x * repetition_penalty, then
    x - (presence_penalty + frequency_penalty * c), in fp32, in front of temperature, top-k and top-p.  The counts live in an int32
    [B, vocab] table on the device: with `penalize_prompt` (the default) it starts from each row's own prompt tokens (`prompt_lens`
    honoured, pads and audio positions not counted), otherwise from zero; the sampler launch that picks a token adds one to its count, a
    finished row's counts stay as they are, and nothing is read by the host.  `stats` also receives "counts": that table (not read), or
    None when no penalty is on.

    `return_logprobs=True` returns (tokens, logprobs), logprobs fp32 [B, n_new] aligned with the tokens: the log-probability of each
    returned token under the model's RAW logits - log_softmax at temperature 1, no penalty, nothing filtered, the formula of
    Llama.token_logprobs - computed by the sampler launch itself; positions after a row's `eos_id` hold 0.0.  That is the model's
    probability of the token, comparable across sampling settings; it is the probability the token was drawn with only when
    temperature == 1 and no filter and no penalty is on.  Penalties and `return_logprobs` are refused with `num_beams` != 1 (beams rank
    by their own log-probabilities) and with `draft_tokens` != 0 (the rows of a draft step would each need the counts of another prefix).

    `top_logprobs` = k in 1..8 (with `return_logprobs=True`; refused where that is) returns (tokens, logprobs, top_ids, top_logp): int32 /
    fp32 [B, n_new, k], the k likeliest tokens at every returned position and their log-probabilities under the same RAW logits,
    descending, equal logits by ascending index (csrc/topk.hip) - whatever the sampling settings, so a greedy token is top_ids[..., 0]
    and a sampled or penalised one need not be among them.  One extra launch per step, in front of the sampler's, nothing read by the
    host; positions after a row's `eos_id` hold -1 / 0.0.  The row's lse is formed in another order than the sampler's, so the entry of
    the returned token agrees with `logprobs` to about 1e-6, not bit for bit."""
    check_params(temperature, top_k, top_p, seed)
    check_penalties(repetition_penalty, presence_penalty, frequency_penalty)
    if isinstance(top_logprobs, bool) or not isinstance(top_logprobs, int) or not 0 <= top_logprobs <= K.TOPK_MAX:
        raise LlxError(f"top_logprobs={top_logprobs!r} must be an integer in 0..{K.TOPK_MAX}")
    if top_logprobs and not return_logprobs:
        raise LlxError(f"top_logprobs={top_logprobs!r} needs return_logprobs=True: the alternatives come with the tokens' log-probabilities")
    penalised = penalties_on(repetition_penalty, presence_penalty, frequency_penalty)
    for name, value, off in (("num_beams", num_beams, 1), ("draft_tokens", draft_tokens, 0)):
        if value != off and penalised:
            raise LlxError(f"{name}={value!r} cannot be combined with repetition_penalty={repetition_penalty!r}, presence_penalty="
                           f"{presence_penalty!r}, frequency_penalty={frequency_penalty!r}: the penalties shape the draw of the plain loops only")
        if value != off and return_logprobs:
            raise LlxError(f"{name}={value!r} cannot be combined with return_logprobs=True: the sampler of the plain loops reports them")
    lens = _check(model, prompt, max_new_tokens, eos_id, prefill_chunk, check_every, prompt_lens,
                  (draft_tokens, draft_ngram, temperature) if draft_tokens != 0 else None,
                  (num_beams, length_penalty, temperature, top_k, top_p, draft_tokens) if num_beams != 1 else None, audio)
    D.prepare(model)
    dev, P, n = prompt.device, prompt.shape[1], max_new_tokens
    call = _caller(model)
    if num_beams != 1:
        return _generate_beam(model, call, prompt, audio, n, num_beams, float(length_penalty), eos_id, prefill_chunk, check_every, stats)
    sampling = dict(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed)
    seen = None
    if penalised:
        sampling.update(repetition_penalty=repetition_penalty, presence_penalty=presence_penalty, frequency_penalty=frequency_penalty)
        seen = seed_counts(prompt, lens, model.config.vocab_size, penalize_prompt)
    if stats is not None:
        stats["counts"] = seen
    if prompt.shape[0] > 1 or (lens is not None and lens != [P]):
        return _generate_batch(model, prompt, n, lens if lens is not None else [P] * prompt.shape[0], sampling, eos_id, prefill_chunk,
                               check_every, call, audio, seen, return_logprobs, top_logprobs)
    if audio is not None:
        logits = prefill_audio(model, audio, prompt)
        P += model.audio_positions(audio.shape[1])  # from here on P is the length of the sequence: clip and prompt
    else:
        chunk = P if prefill_chunk is None else prefill_chunk
        positions = torch.arange(P, device=dev)
        # forward rotates a call's tokens by rope[:L] whatever input_pos says (the reference's modelling/llama.py:207).  For one
        # whole-prompt call that is each token's own position; a later chunk must see the same rows, or chunking - a memory measure -
        # would change the result: the chunk runs with the table shifted to its first position.  Decode steps below keep rope[:1], as a
        # hand loop does.
        table = model.rope
        try:
            for s in range(0, P, chunk):
                model.rope = table[s:]
                logits = call(prompt[:, s : s + chunk], positions[s : s + chunk])
        finally:
            model.rope = table
    if draft_tokens != 0:
        draft_tokens = _draft_rows(model, draft_tokens, dev)
    if draft_tokens != 0:
        return _generate_draft(model, prompt, logits, n, draft_tokens, draft_ngram, eos_id, check_every, stats, call)
    pos = torch.full((1,), P - 1, device=dev, dtype=torch.int64)  # position of the row being sampled from; the sampler advances it
    tok = torch.empty(1, 1, device=dev, dtype=torch.int64)
    history = torch.empty(1, n, device=dev, dtype=torch.int64)
    finished = torch.zeros(1, device=dev, dtype=torch.int32) if eos_id is not None else None
    kw = dict(**sampling, pos=pos, out=tok.view(1), history=history, hist_base=P - 1, advance=True, eos_id=eos_id, finished=finished)
    if seen is not None:
        kw["counts"] = seen
    if return_logprobs:
        kw["logprob_history"] = torch.zeros(1, n, device=dev, dtype=torch.float32)
    top = _TopLogprobs(top_logprobs, 1, n, dev) if top_logprobs else None
    if top is not None:
        top.step(logits[0, -1:], kw)
    K.sample(logits[0, -1:], **kw)
    count = n
    for k in range(1, n + 1):
        if finished is not None and (k % check_every == 0 or k == n):
            # one host read: a finished row stops advancing, so its counter gives the length (eos included)
            state = int((pos * 2 + finished).item())
            if state & 1:
                count = (state >> 1) - (P - 1)
                break
        if k == n:
            break
        logits = call(tok, pos)[0]
        if top is not None:
            top.step(logits, kw)
        K.sample(logits, **kw)
    if stats is not None:
        stats.update(steps=count, tokens=count, accepted=0, draft_tokens=0, launched=k - 1)
    if top is not None:
        return history[:, :count], kw["logprob_history"][:, :count], top.ids[:, :count], top.logp[:, :count]
    return (history[:, :count], kw["logprob_history"][:, :count]) if return_logprobs else history[:, :count]
