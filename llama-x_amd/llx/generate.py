"""Text generation on the KV-cache inference path: prefill, then one `model(...)` call and one sampler launch per token.

The reference names its `input_pos` branch "used for inference i.e. generate" (modelling/llama.py:204) and ships no generate();
this is that loop.  Nothing in it reads the device inside a token: the sampler (csrc/sample.hip) writes the next input token, appends
it to the history buffer and advances the position counter on the device, so the launch-bound decode path is never
stalled by an `.item()`.  With `eos_id` the host looks at the finished flag once every `check_every` tokens.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import kernels as K
from ._lib import LlxError
from .sampling import check_params


def _check(model, prompt: Tensor, max_new_tokens: int, eos_id, prefill_chunk, check_every) -> None:
    from modelling.llama import Llama

    if not isinstance(model, Llama) or type(model)._embed is not Llama._embed:
        raise LlxError(f"generate() drives a text Llama (got {type(model).__name__})")
    if model.training:
        raise LlxError("generate() needs the model in eval mode: call model.eval()")
    if any(layer.attention.kv_cache is None for layer in model.layers) or not hasattr(model, "causal_mask"):
        raise LlxError("generate() needs the KV cache: call model.build_cache(inference=True) first")
    if not (isinstance(prompt, Tensor) and prompt.dtype is torch.int64 and prompt.dim() == 2 and prompt.shape[0] == 1 and prompt.shape[1] >= 1):
        raise LlxError("generate(): prompt must be an int64 tensor [1, P] with P >= 1 (the KV cache is batch 1)")
    if not prompt.is_cuda or model.tok_embeddings.weight.device != prompt.device:
        raise LlxError("generate() runs on the HIP device: model and prompt must be on the same GPU")
    if not (isinstance(max_new_tokens, int) and max_new_tokens >= 1):
        raise LlxError(f"max_new_tokens={max_new_tokens!r} must be an integer >= 1")
    if prompt.shape[1] + max_new_tokens > model.config.max_seq_len:
        raise LlxError(f"prompt ({prompt.shape[1]}) + max_new_tokens ({max_new_tokens}) exceeds max_seq_len ({model.config.max_seq_len})")
    if eos_id is not None and not (isinstance(eos_id, int) and 0 <= eos_id < model.config.vocab_size):
        raise LlxError(f"eos_id={eos_id!r} must be a token id in [0, {model.config.vocab_size})")
    if prefill_chunk is not None and not (isinstance(prefill_chunk, int) and prefill_chunk >= 1):
        raise LlxError(f"prefill_chunk={prefill_chunk!r} must be None or an integer >= 1")
    if not (isinstance(check_every, int) and check_every >= 1):
        raise LlxError(f"check_every={check_every!r} must be an integer >= 1")


@torch.no_grad()
def generate(model, prompt: Tensor, max_new_tokens: int, *, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0,
             eos_id: Optional[int] = None, prefill_chunk: Optional[int] = None, check_every: int = 16) -> Tensor:
    """Continue `prompt` (int64 [1, P]) by up to `max_new_tokens` tokens -> int64 [1, n_new] on the prompt's device.

    The draw for the token at absolute position q uses the counter q - 1 (the position of the logits row it is sampled from), so the
    same arguments give the same tokens whatever `prefill_chunk` and `check_every` are.  With `eos_id` the result ends at the first
    `eos_id`, inclusive.

    The host learns of an `eos_id` only at the next `check_every` boundary: until then the loop keeps launching decode steps (up to
    `check_every - 1` of them), each feeding `eos_id` at the position counter, which no longer advances.  The returned tokens are not
    affected, but after an early stop the cache row at the position that follows the `eos_id` holds that token's keys and values rather
    than nothing.  While a prefill chunk runs, `model.rope` is a shifted view of the table (restored before the first decode step, also
    on an exception): do not drive the same model from another thread meanwhile."""
    check_params(temperature, top_k, top_p, seed)
    _check(model, prompt, max_new_tokens, eos_id, prefill_chunk, check_every)
    dev, P, n = prompt.device, prompt.shape[1], max_new_tokens
    chunk = P if prefill_chunk is None else prefill_chunk
    positions = torch.arange(P, device=dev)
    # forward rotates a call's tokens by rope[:L] whatever input_pos says (the reference's modelling/llama.py:207).  For one whole-prompt
    # call that is each token's own position; a later chunk must see the same rows, or chunking - a memory measure - would change the
    # result: the chunk runs with the table shifted to its first position.  Decode steps below keep rope[:1], as a hand loop does.
    table = model.rope
    try:
        for s in range(0, P, chunk):
            model.rope = table[s:]
            logits = model(prompt[:, s : s + chunk], input_pos=positions[s : s + chunk])
    finally:
        model.rope = table
    pos = torch.full((1,), P - 1, device=dev, dtype=torch.int64)  # position of the row being sampled from; the sampler advances it
    tok = torch.empty(1, 1, device=dev, dtype=torch.int64)
    history = torch.empty(1, n, device=dev, dtype=torch.int64)
    finished = torch.zeros(1, device=dev, dtype=torch.int32) if eos_id is not None else None
    kw = dict(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, pos=pos, out=tok.view(1), history=history, hist_base=P - 1,
              advance=True, eos_id=eos_id, finished=finished)
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
        K.sample(model(tok, input_pos=pos)[0], **kw)
    return history[:, :count]
