"""Decode fast path: a transformer layer / LM head for a handful of query tokens against the KV cache, as weight-streaming kernels.

Reference semantics: the cached branch of Attention.forward (modelling/llama.py:126-127,135-137) inside TransformerLayer.forward
(:163-174) and the head of Llama.forward (:216) - same values as the generic inference path of modelling/llama.py::_run_dense, which
stays for every call this path does not take (more than 4 tokens, more than 16 query rows per kv head, biases, DoRA linears).
Int8LinearWeight linears (weight-only or dynamic, subclasses/int8.py:106-121) stream their int8 rows (llx_gemv_i8): no bf16 image of
the matrix is built or read.

A batch of 2 <= B <= 16 sequences with one token each (x [B, 1, D], a cache of batch B, bf16 linears without adapters) takes the same
steps per layer with the MFMA weight stream (llx_gemm_rows16_bf16) in place of the GEMV: the weights are read once for all B rows (a
product whose K is split adds a small combine launch).  int8 and LoRA / DoRA linears and B > 16 stay on the generic path at B > 1.

Per layer (M <= 4 tokens at batch 1):
    q            = gemv([wq; wk; wv], rmsnorm(x))  + RoPE on q, k + k, v scattered into the caches        1 launch
    o            = SDPA(q, k_cache, v_cache, mask)  split over the cache, 4 heads per K/V read             2 launches
    x            = x + gemv(wo, o)                                                                         1 launch
    h            = silu(gemv(w1, rmsnorm(x))) * gemv(w3, rmsnorm(x))                                       1 launch
    x            = x + gemv(w2, h)                                                                         1 launch
LoRA-dressed linears (modelling/lora.py:43) add one small launch per group for t = x @ A^T; the B factors ride in the main launch.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from . import kernels as K
from . import ops

BF16 = torch.bfloat16
MAX_TOKENS = 4
MAX_BATCH = 16  # sequences per batched decode step on the MFMA weight stream (one MFMA operand)
BATCHED = True  # False: x [B, 1, D] with B > 1 takes the generic inference path (the tests' reference arm)


KIND_BF16, KIND_I8W, KIND_I8D = "bf16", "int8-weight-only", "int8-dynamic"


def _plain(m: nn.Linear) -> Optional[str]:
    """The kind of a linear this path streams, or None: bf16 weight or Int8LinearWeight (bf16 scale; weight-only or dynamic), no bias,
    optionally a LoRA adapter (rank a multiple of 8)."""
    from subclasses.int8 import Int8LinearWeight

    if m.bias is not None or m.weight.dtype is not BF16 or getattr(m, "m", None) is not None:
        return None
    rank = int(getattr(m, "rank", 0) or 0)
    if not (rank == 0 or (rank % 8 == 0 and m.lora_a.dtype is BF16)):
        return None
    if isinstance(m.weight, Int8LinearWeight):
        if m.weight.scale.dtype is not BF16 or m.in_features % 16 != 0:
            return None
        return KIND_I8D if m.weight.dynamic_int8_act else KIND_I8W
    return KIND_BF16


def _w(mods) -> dict:
    """The weight operands of one gemv call: (ws, wscale, dynamic) of a group of linears of one kind."""
    if _plain(mods[0]) == KIND_BF16:
        return dict(ws=[m.weight.detach() for m in mods])
    return dict(ws=[m.weight.int_data for m in mods], wscale=[m.weight.scale for m in mods], dynamic=bool(mods[0].weight.dynamic_int8_act))


def _batched(x: Tensor) -> bool:
    return x.dim() == 3 and 2 <= x.shape[0] <= MAX_BATCH and x.shape[1] == 1 and BATCHED


def _bf16_plain(mods) -> bool:
    return all(_plain(m) == KIND_BF16 and int(getattr(m, "rank", 0) or 0) == 0 for m in mods)


def _layer_ok_batched(layer, x: Tensor, mask: Optional[Tensor]) -> bool:
    """x [B, 1, D], 2 <= B <= 16: a cache of batch B, a bool mask [B | 1, 1, 1, Skv], bf16 linears without adapters, head_dim 128."""
    att, ff = layer.attention, layer.feed_forward
    if att.kv_cache is None or mask is None or x.dtype is not BF16 or not x.is_cuda or att.kv_cache.k_cache.shape[0] != x.shape[0]:
        return False
    Skv = att.kv_cache.k_cache.shape[2]
    if mask.dtype is not torch.bool or mask.dim() != 4 or mask.shape[0] not in (1, x.shape[0]) or tuple(mask.shape[1:]) != (1, 1, Skv):
        return False
    if att.head_dim != 128 or att.num_heads // att.num_kv_heads > 16 or x.shape[2] % 8 != 0 or ff.w2.in_features % 8 != 0:
        return False
    if not _bf16_plain((att.wq, att.wk, att.wv, att.wo, ff.w1, ff.w3, ff.w2)):
        return False
    return ff.w1.out_features == ff.w3.out_features


def layer_ok(layer, x: Tensor, mask: Optional[Tensor]) -> bool:
    if _batched(x):
        return _layer_ok_batched(layer, x, mask)
    att = layer.attention
    if att.kv_cache is None or mask is None or x.dim() != 3 or x.shape[0] != 1 or x.dtype is not BF16 or not x.is_cuda:
        return False
    M = x.shape[1]
    if M > MAX_TOKENS or M * (att.num_heads // att.num_kv_heads) > 16 or att.head_dim != 128 or mask.dtype is not torch.bool:
        return False
    if x.shape[2] % 8 != 0 or layer.feed_forward.w2.in_features % 8 != 0:
        return False
    ff = layer.feed_forward
    lins = (att.wq, att.wk, att.wv, att.wo, ff.w1, ff.w3, ff.w2)
    if not all(_plain(m) is not None for m in lins):
        return False
    for grp in ((att.wq, att.wk, att.wv), (ff.w1, ff.w3)):  # one t vector, one scale and one weight kind per fused group
        ranks = {int(getattr(m, "rank", 0) or 0) > 0 for m in grp}
        if len(ranks) != 1 or len({float(getattr(m, "scale", 1.0)) for m in grp}) != 1 or len({_plain(m) for m in grp}) != 1:
            return False
    return att.wq.out_features % 4 == 0 and att.wk.out_features % 4 == 0 and ff.w1.out_features == ff.w3.out_features


def _lora(mods, x: Tensor, norm):
    """(b factors, t = [rmsnorm(x) | x] @ [A_0; A_1; ..]^T, scale) or None."""
    if int(getattr(mods[0], "rank", 0) or 0) == 0:
        return None
    t = K.gemv([m.lora_a.detach() for m in mods], x, norm=norm)
    return [m.lora_b.detach() for m in mods], t, float(mods[0].scale)


def mask_extent(mask: Tensor) -> Tensor:
    """Extent of the call's mask, computed once and shared by all layers (cached on the mask tensor)."""
    return ops._cached(mask, "extent", lambda: K.mask_extent(mask))


def _layer_forward_batched(layer, x: Tensor, rope: Tensor, mask: Tensor, input_pos: Tensor) -> Tensor:
    """B sequences, one token each: the launches of the batch-1 layer, every weight read once for all rows."""
    att, ff = layer.attention, layer.feed_forward
    B, D = x.shape[0], x.shape[2]
    H, KVH, hd = att.num_heads, att.num_kv_heads, att.head_dim
    x2 = x.reshape(B, D)
    cache = att.kv_cache
    pos = input_pos.to(torch.int64)
    pos = (pos.reshape(B) if pos.dim() == 2 else pos.expand(B)).contiguous()  # [B, 1]: a position per sequence; [1]: shared
    q = K.gemm_rows16([att.wq.weight.detach(), att.wk.weight.detach(), att.wv.weight.detach()], x2,
                      norm=(layer.attention_norm.weight.detach(), layer.attention_norm.eps), epilogue=K.GV_QKV,
                      qkv=(rope, H * hd, KVH * hd, cache.k_cache, cache.v_cache, pos))
    o = K.attn_decode(q.view(B, 1, H, hd).transpose(1, 2), cache.k_cache, cache.v_cache, mask, mask_extent(mask))  # [B, 1, H*hd]
    x1 = K.gemm_rows16([att.wo.weight.detach()], o.view(B, H * hd), epilogue=K.GV_RESIDUAL, res=x2)
    h = K.gemm_rows16([ff.w1.weight.detach(), ff.w3.weight.detach()], x1, norm=(layer.ffn_norm.weight.detach(), layer.ffn_norm.eps),
                      epilogue=K.GV_SWIGLU)
    x3 = K.gemm_rows16([ff.w2.weight.detach()], h, epilogue=K.GV_RESIDUAL, res=x1)
    return x3.view(B, 1, D)


def layer_forward(layer, x: Tensor, rope: Tensor, mask: Tensor, input_pos: Tensor) -> Tensor:
    if x.shape[0] > 1:
        return _layer_forward_batched(layer, x, rope, mask, input_pos)
    att, ff = layer.attention, layer.feed_forward
    M, D = x.shape[1], x.shape[2]
    H, KVH, hd = att.num_heads, att.num_kv_heads, att.head_dim
    x2 = x.view(M, D)
    n1 = (layer.attention_norm.weight.detach(), layer.attention_norm.eps)
    qkv_mods = (att.wq, att.wk, att.wv)
    cache = att.kv_cache
    pos = input_pos.to(torch.int64).reshape(-1).contiguous()  # [M], or [1, M]: batch 1 with a position row of its own
    q = K.gemv(x=x2, norm=n1, epilogue=K.GV_QKV, **_w(qkv_mods),
               qkv=(rope, H * hd, KVH * hd, cache.k_cache, cache.v_cache, pos), lora=_lora(qkv_mods, x2, n1))
    o = K.attn_decode(q.view(1, M, H, hd).transpose(1, 2), cache.k_cache, cache.v_cache, mask, mask_extent(mask))  # [1, M, H*hd]
    o2 = o.view(M, H * hd)
    x1 = K.gemv(x=o2, epilogue=K.GV_RESIDUAL, res=x2, lora=_lora((att.wo,), o2, None), **_w((att.wo,)))
    n2 = (layer.ffn_norm.weight.detach(), layer.ffn_norm.eps)
    h = K.gemv(x=x1, norm=n2, epilogue=K.GV_SWIGLU, lora=_lora((ff.w1, ff.w3), x1, n2), **_w((ff.w1, ff.w3)))
    x3 = K.gemv(x=h, epilogue=K.GV_RESIDUAL, res=x1, lora=_lora((ff.w2,), h, None), **_w((ff.w2,)))
    return x3.view(1, M, D)


def head_ok(model, x: Tensor) -> bool:
    if _batched(x):
        return x.is_cuda and x.dtype is BF16 and x.shape[2] % 8 == 0 and _bf16_plain((model.output,))
    return (x.dim() == 3 and x.shape[0] == 1 and x.shape[1] <= MAX_TOKENS and x.is_cuda and x.dtype is BF16 and _plain(model.output) is not None
            and x.shape[2] % 8 == 0)


def head_forward(model, x: Tensor) -> Tensor:
    """logits = output(norm(x)) (modelling/llama.py:216) for M <= 4 rows: the 1 GB head weight streamed once."""
    M, D = x.shape[1], x.shape[2]
    nw = (model.norm.weight.detach(), model.norm.eps)
    if x.shape[0] > 1:  # [B, 1, D]: the same product on the MFMA weight stream
        return K.gemm_rows16([model.output.weight.detach()], x.reshape(x.shape[0], D), norm=nw).view(x.shape[0], 1, -1)
    x2 = x.reshape(M, D)
    logits = K.gemv(x=x2, norm=nw, lora=_lora((model.output,), x2, nw), **_w((model.output,)))
    return logits.view(1, M, -1)
