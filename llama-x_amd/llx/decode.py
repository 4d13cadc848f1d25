"""Decode fast path: a transformer layer / LM head for a handful of query tokens against the KV cache, as weight-streaming kernels.

Reference semantics: the cached branch of Attention.forward (modelling/llama.py:126-127,135-137) inside TransformerLayer.forward
(:163-174) and the head of Llama.forward (:216) - same values as the generic inference path of modelling/llama.py::_run_dense, which
stays for every call this path does not take (more than 4 tokens, more than 16 query rows per kv head, biases, adapters of rank
above 64 or not a multiple of 8, a fused group that mixes DoRA and other members, DoRA on an int8 weight).
Int8LinearWeight linears (weight-only or dynamic, subclasses/int8.py:106-121) stream their int8 rows (llx_gemv_i8): no bf16 image of
the matrix is built or read.  MXFP4LinearWeight linears (subclasses/mxfp4.py) stream their packed rows and scale bytes
(llx_gemv_mxfp4) with the rounding points of the bf16 GEMV on the dequantised image; they have no batched stream yet, so a batch of
B > 1 sequences stays on the generic path.

A batch of 2 <= B <= 16 sequences with one token each (x [B, 1, D], a cache of batch B) takes the same steps per layer with the MFMA
weight stream in place of the GEMV: the weights are read once for all B rows (a product whose K is split adds a small combine
launch).  Every fused group is bf16 (llx_gemm_rows16_bf16) or dynamic int8 (llx_gemm_rows16_i8: the rows quantised in the prologue,
int8 MFMA); groups of different kinds may sit next to each other in a layer, as at batch 1.  LoRA linears on either kind and DoRA
linears on bf16 ride the same stream when every rank of the group is 16, 32, 48 or 64 (llx_gemm_rows16_bf16_lora /
llx_gemm_rows16_i8_lora): t = x @ A^T is the stream itself run on the A factors - its segments are 16-row tiles, hence the ranks -
and the B factors (and DoRA's cached row factors) enter where a tile's epilogue runs, as a short MFMA chain.  Weight-only int8,
other ranks, a group that mixes adapted and plain members and B > 16 stay on the generic path at B > 1.

Per layer (M <= 4 tokens at batch 1):
    q            = gemv([wq; wk; wv], rmsnorm(x))  + RoPE on q, k + k, v scattered into the caches        1 launch
    o            = SDPA(q, k_cache, v_cache, mask)  split over the cache, 4 heads per K/V read             2 launches
    x            = x + gemv(wo, o)                                                                         1 launch
    h            = silu(gemv(w1, rmsnorm(x))) * gemv(w3, rmsnorm(x))                                       1 launch
    x            = x + gemv(w2, h)                                                                         1 launch
LoRA-dressed linears (modelling/lora.py:43) add one small launch per group for t = x @ A^T; the B factors ride in the main launch.
DoRA linears (modelling/lora.py:51-59, bf16 weights) are LoRA linears whose bf16 output is multiplied by c = m / ||W + s B A||_row
in the same launch (llx_gemv_bf16_dora).  c depends on parameters only: ops.dora_scale_cached keeps it per linear (2 bytes per
output row, rebuilt when weight, lora_a, lora_b or m change), so a token costs a DoRA model the launches and the one weight pass
of a LoRA model.  The factor is built at a linear's first use: prepare(model) builds them all up front, which a caller that
captures a decode step into a graph must do (or run one warm-up step) before the capture - a tensor first allocated while
capturing lives in the capture's private pool.  generate() calls prepare().
An FP8 KV cache (build_cache(..., kv_dtype="fp8")) needs no route of its own here: the uint8 caches ride in the qkv
tuple, K.gemv / K.gemm_rows16 pick the q|k|v epilogue that stores E4M3 codes and K.attn_decode reads them.  A decode step builds no
bf16 image of such a cache (only prefill calls do), so nothing of it is allocated inside a captured step.
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


KIND_BF16, KIND_I8W, KIND_I8D, KIND_MX4 = "bf16", "int8-weight-only", "int8-dynamic", "mxfp4"


def _plain(m: nn.Linear) -> Optional[str]:
    """The kind of a linear this path streams, or None: bf16 weight, Int8LinearWeight (bf16 scale; weight-only or dynamic) or
    MXFP4LinearWeight, no bias, optionally a LoRA adapter (rank a multiple of 8), or - bf16 weights only - a DoRA adapter (rank a
    multiple of 8 up to 64, the ranks dora_scale_cached builds; bf16 factors and magnitude vector)."""
    from subclasses.int8 import Int8LinearWeight
    from subclasses.mxfp4 import MXFP4LinearWeight

    if m.bias is not None or m.weight.dtype is not BF16:
        return None
    rank = int(getattr(m, "rank", 0) or 0)
    if not (rank == 0 or (rank % 8 == 0 and m.lora_a.dtype is BF16)):
        return None
    if _dora(m) and not (rank <= 64 and m.lora_b.dtype is BF16 and m.m.dtype is BF16 and tuple(m.m.shape) == (m.out_features,)
                         and not isinstance(m.weight, (Int8LinearWeight, MXFP4LinearWeight))):
        return None
    if isinstance(m.weight, MXFP4LinearWeight):  # (reports bf16: recognised before the bf16 fall-through)
        return KIND_MX4
    if isinstance(m.weight, Int8LinearWeight):
        if m.weight.scale.dtype is not BF16 or m.in_features % 16 != 0:
            return None
        return KIND_I8D if m.weight.dynamic_int8_act else KIND_I8W
    return KIND_BF16


def _dora(m: nn.Linear) -> bool:
    """A DoRALinear with an adapter (modelling/lora.py:51: rank 0 attaches no magnitude vector)."""
    return int(getattr(m, "rank", 0) or 0) > 0 and getattr(m, "m", None) is not None


def _w(mods) -> dict:
    """The weight operands of one gemv call: (ws, wscale, dynamic) of a group of linears of one kind; bf16 DoRA members add their cached
    row factors (colscale), MXFP4 members hand over their packed rows and scale bytes (mxscale)."""
    if _plain(mods[0]) == KIND_BF16:
        if _dora(mods[0]):  # (layer_ok: all members or none)
            return dict(ws=[m.weight.detach() for m in mods], colscale=[ops.dora_scale_cached(m) for m in mods])
        return dict(ws=[m.weight.detach() for m in mods])
    if _plain(mods[0]) == KIND_MX4:
        return dict(ws=[m.weight.packed for m in mods], mxscale=[m.weight.scale for m in mods])
    return dict(ws=[m.weight.int_data for m in mods], wscale=[m.weight.scale for m in mods], dynamic=bool(mods[0].weight.dynamic_int8_act))


def _batched(x: Tensor) -> bool:
    return x.dim() == 3 and 2 <= x.shape[0] <= MAX_BATCH and x.shape[1] == 1 and BATCHED


BATCH_RANKS = (16, 32, 48, 64)  # adapter ranks of the batched stream: the t product's segments are its 16-row tiles


def _batch_group(mods) -> bool:
    """A fused group the batched stream takes: all members bf16, or all dynamic int8; none with an adapter, or all with LoRA adapters
    of ranks in BATCH_RANKS (bf16 factors) and one scale, or - bf16 only - all with such DoRA adapters."""
    if {_plain(m) for m in mods} not in ({KIND_BF16}, {KIND_I8D}):
        return False
    ranks = [int(getattr(m, "rank", 0) or 0) for m in mods]
    if not any(ranks):
        return True
    if not all(r in BATCH_RANKS and m.lora_b.dtype is BF16 for r, m in zip(ranks, mods)):
        return False
    return len({float(m.scale) for m in mods}) == 1 and len({_dora(m) for m in mods}) == 1


def layer_ok(layer, x: Tensor, mask: Optional[Tensor]) -> bool:
    """x [1, M <= 4, D], or x [B, 1, D] with 2 <= B <= 16: a cache of batch B, a bool mask [B | 1, 1, 1, Skv], every fused group
    one that _batch_group takes."""
    att, ff = layer.attention, layer.feed_forward
    if att.kv_cache is None or mask is None or x.dim() != 3 or x.dtype is not BF16 or not x.is_cuda or mask.dtype is not torch.bool:
        return False
    if att.head_dim != 128 or x.shape[2] % 8 != 0 or ff.w2.in_features % 8 != 0 or ff.w1.out_features != ff.w3.out_features:
        return False
    lins = (att.wq, att.wk, att.wv, att.wo, ff.w1, ff.w3, ff.w2)
    G = att.num_heads // att.num_kv_heads
    if _batched(x):
        B, Skv = x.shape[0], att.kv_cache.k_cache.shape[2]
        return (att.kv_cache.k_cache.shape[0] == B and mask.dim() == 4 and mask.shape[0] in (1, B) and tuple(mask.shape[1:]) == (1, 1, Skv)
                and G <= 16 and all(_batch_group(g) for g in ((att.wq, att.wk, att.wv), (att.wo,), (ff.w1, ff.w3), (ff.w2,))))
    if x.shape[0] != 1 or x.shape[1] > MAX_TOKENS or x.shape[1] * G > 16 or not all(_plain(m) is not None for m in lins):
        return False
    for grp in ((att.wq, att.wk, att.wv), (ff.w1, ff.w3)):  # one t vector, one scale and one weight kind per fused group, all DoRA or none
        ranks = {int(getattr(m, "rank", 0) or 0) > 0 for m in grp}
        if len(ranks) != 1 or len({float(getattr(m, "scale", 1.0)) for m in grp}) != 1 or len({_plain(m) for m in grp}) != 1:
            return False
        if len({_dora(m) for m in grp}) != 1:
            return False
    return att.wq.out_features % 4 == 0 and att.wk.out_features % 4 == 0


def _lora(mods, x: Tensor, norm, stream=K.gemv):
    """(b factors, t = [rmsnorm(x) | x] @ [A_0; A_1; ..]^T, scale) or None; stream: the product that computes t (K.gemv | K.gemm_rows16)."""
    if int(getattr(mods[0], "rank", 0) or 0) == 0:
        return None
    t = stream([m.lora_a.detach() for m in mods], x, norm=norm)
    return [m.lora_b.detach() for m in mods], t, float(mods[0].scale)


def mask_extent(mask: Tensor) -> Tensor:
    """Extent of the call's mask, computed once and shared by all layers (cached on the mask tensor)."""
    return ops._cached(mask, "extent", lambda: K.mask_extent(mask))


def _lin(batched: bool):
    """lin(mods, x, **kw): the fused product of a group of linears on the rows of x - the GEMV (any streamed kind, adapters) at batch 1,
    the MFMA weight stream for a batch (per group: bf16 or dynamic int8, adapters of the ranks in BATCH_RANKS)."""
    if batched:
        def lin(mods, x, norm=None, **kw):
            w = _w(mods)
            w.pop("dynamic", None)  # int8 groups of a batch are of the dynamic kind (layer_ok)
            return K.gemm_rows16(x=x, norm=norm, lora=_lora(mods, x, norm, K.gemm_rows16), **w, **kw)
        return lin
    return lambda mods, x, norm=None, **kw: K.gemv(x=x, norm=norm, lora=_lora(mods, x, norm), **_w(mods), **kw)


def layer_forward(layer, x: Tensor, rope: Tensor, mask: Tensor, input_pos: Tensor) -> Tensor:
    """x [1, M, D]: M tokens of one sequence; x [B, 1, D]: B sequences, one token each - the same launches, every weight read once."""
    att, ff = layer.attention, layer.feed_forward
    batched = x.shape[0] > 1
    lin = _lin(batched)
    R, D = x.shape[0] * x.shape[1], x.shape[2]  # activation rows
    H, KVH, hd = att.num_heads, att.num_kv_heads, att.head_dim
    x2 = x.reshape(R, D)
    cache = att.kv_cache
    pos = input_pos.to(torch.int64)
    if batched and pos.dim() != 2:
        pos = pos.expand(R)  # [1]: one position shared by the batch ([B, 1]: a position per sequence)
    pos = pos.reshape(R).contiguous()  # batch 1: [M], or [1, M] (a position row of its own)
    q = lin((att.wq, att.wk, att.wv), x2, norm=(layer.attention_norm.weight.detach(), layer.attention_norm.eps), epilogue=K.GV_QKV,
            qkv=(rope, H * hd, KVH * hd, cache.k_cache, cache.v_cache, pos))
    o = K.attn_decode(q.view(*x.shape[:2], H, hd).transpose(1, 2), cache.k_cache, cache.v_cache, mask, mask_extent(mask))  # [.., .., H*hd]
    x1 = lin((att.wo,), o.view(R, H * hd), epilogue=K.GV_RESIDUAL, res=x2)
    h = lin((ff.w1, ff.w3), x1, norm=(layer.ffn_norm.weight.detach(), layer.ffn_norm.eps), epilogue=K.GV_SWIGLU)
    x3 = lin((ff.w2,), h, epilogue=K.GV_RESIDUAL, res=x1)
    return x3.view(x.shape)


def prepare(model):
    """Build the cached row factor of every DoRA linear of `model` that the decode path streams (a no-op for other models) and return
    the model.  Call it - or run one warm-up step - before capturing a decode step into a graph: built lazily, the first factors would
    be allocated inside the capture and live in its private pool."""
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.Linear) and _dora(m) and m.weight.is_cuda and _plain(m) is not None:
                ops.dora_scale_cached(m)
    return model


def head_ok(model, x: Tensor) -> bool:
    if x.dim() != 3 or not x.is_cuda or x.dtype is not BF16 or x.shape[2] % 8 != 0:
        return False
    if _batched(x):
        return _batch_group((model.output,))
    return x.shape[0] == 1 and x.shape[1] <= MAX_TOKENS and _plain(model.output) is not None


def head_forward(model, x: Tensor) -> Tensor:
    """logits = output(norm(x)) (modelling/llama.py:216) for M <= 4 rows, or a batch of one-token rows: the 1 GB head weight streamed once."""
    logits = _lin(x.shape[0] > 1)((model.output,), x.reshape(-1, x.shape[2]), norm=(model.norm.weight.detach(), model.norm.eps))
    return logits.view(*x.shape[:2], -1)
