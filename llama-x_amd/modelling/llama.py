"""Llama decoder with the reference's module API (/root/reference/modelling/llama.py:17-292), executing on
hand-written gfx950 kernels.

Class names, constructor signatures, parameter / state-dict names and forward signatures match the reference so
training scripts can switch packages unchanged.  What differs is below the module boundary: every residual branch of
a layer is ONE autograd node (llx/ops.py) that calls the HIP kernels of llama-x_amd/csrc through the C-ABI; there
is no SDPA / FlexAttention / aten matmul on the hot path and no CPU fallback (CPU tensors raise).

``block_mask`` takes a :class:`llx.kernels.MaskSpec` in place of FlexAttention's BlockMask: per-token ``doc_ids`` /
per-sample ``prefix_len`` (the mask rule is the reference's ``mask_mod``, train_metamathqa.py:67-68, plus the prefix-LM
term of README.md:16), or ``dense=`` any bool mask; ``MaskSpec.from_mask_mod(mask_mod, B, S, device)`` stands where the
reference calls ``create_block_mask(mask_mod, ...)`` (train_metamathqa.py:70).
"""
import json
import os
from typing import NamedTuple

import torch
from torch import Tensor, nn
from torch.utils.checkpoint import checkpoint

from llx import decode as D
from llx import kernels as K
from llx import ops
from llx._lib import LlxError
from llx.kernels import MaskSpec  # noqa: F401  (re-exported: the block_mask type of this package)


class LlamaConfig(NamedTuple):
    embed_dim: int
    num_layers: int
    head_dim: int
    num_heads: int
    num_kv_heads: int
    intermediate_dim: int
    max_seq_len: int = 2048
    vocab_size: int = 128_256  # Llama3
    attn_dropout: float = 0.0
    rope_base: int = 50_000
    is_llama3_1: bool = False
    activation_checkpointing: bool = False


# ------------------------------------------------------------------------------------------------- RoPE
def scale_llama3_1_rope(freqs: Tensor) -> Tensor:
    """Llama-3.1 frequency rescale (factor 8, low 1, high 4, original context 8192), host side, fp32."""
    factor, low, high, ctx_len = 8, 1, 4, 8192
    wavelen = 2 * torch.pi / freqs
    ratio = (ctx_len / wavelen - low) / (high - low)
    blended = (1 - ratio) * freqs / factor + ratio * freqs
    long_wave = torch.where(wavelen > ctx_len / low, freqs / factor, blended)
    return torch.where(wavelen < ctx_len / high, freqs, long_wave).to(freqs.dtype)


def build_rope(config: LlamaConfig) -> Tensor:
    """fp32 [max_seq_len, head_dim/2, 2] table of (cos, sin); built on the host for bit parity of the table."""
    half = torch.arange(0, config.head_dim, 2, dtype=torch.float32) / config.head_dim
    theta = 1.0 / (config.rope_base**half)
    if config.is_llama3_1:
        theta = scale_llama3_1_rope(theta)
    angle = torch.outer(torch.arange(config.max_seq_len, dtype=torch.float32), theta)
    return torch.stack([angle.cos(), angle.sin()], dim=-1)


class _RopeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, table: Tensor):
        B, S, H, hd = x.shape
        ctx.table, ctx.shape = table, x.shape
        y = x.contiguous().clone().view(B, S, H * hd)
        return K.rope_(y, table, H).view(B, S, H, hd)

    @staticmethod
    def backward(ctx, g: Tensor):
        B, S, H, hd = ctx.shape
        y = g.contiguous().clone().view(B, S, H * hd)
        return K.rope_(y, ctx.table, H, backward=True).view(B, S, H, hd), None


def _rope_f32(rope: Tensor) -> Tensor:
    # model.bfloat16() also casts the buffer (train_metamathqa.py:176): keep those rounded values, widen for the kernel
    return rope if rope.dtype is torch.float32 else ops._cached(rope, "f32", lambda: rope.float())


def apply_rope(x: Tensor, rope: Tensor) -> Tensor:
    """Interleaved-pair rotation of x [B, S, H, 128] by the first S rows of ``rope`` (fp32 math, one rounding)."""
    return _RopeFn.apply(x, _rope_f32(rope).contiguous())


# ------------------------------------------------------------------------------------------------- leaf modules
class Linear(nn.Linear):
    """nn.Linear whose stand-alone forward runs the llx GEMM (still an nn.Linear for quantize_/adapter surgery)."""

    def forward(self, x: Tensor) -> Tensor:
        return ops.linear(x, self)


class RMSNorm(nn.RMSNorm):
    def forward(self, x: Tensor) -> Tensor:
        return ops.rmsnorm(x, self.weight, self.eps)


class _EmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids: Tensor, table: Tensor):
        ctx.save_for_backward(ids)
        ctx.vocab = table.shape[0]
        return K.embedding_fwd(ids, table.detach())

    @staticmethod
    def backward(ctx, g: Tensor):
        (ids,) = ctx.saved_tensors
        return None, K.embedding_bwd(ids, g.contiguous(), ctx.vocab).to(g.dtype)


class Embedding(nn.Embedding):
    def forward(self, ids: Tensor) -> Tensor:
        return _EmbeddingFn.apply(ids, self.weight)


def check_kv_dtype(kv_dtype, config: LlamaConfig) -> None:
    """What build_cache refuses before it allocates: an unknown kv_dtype; for "fp8" a head_dim other than 128 or an odd max_seq_len."""
    if kv_dtype not in K.KV_DTYPES:
        raise LlxError(f"build_cache: kv_dtype={kv_dtype!r} must be one of {K.KV_DTYPES}")
    if kv_dtype == "fp8" and config.head_dim != 128:
        raise LlxError(f"build_cache: kv_dtype='fp8' needs head_dim 128 (got {config.head_dim})")
    if kv_dtype == "fp8" and config.max_seq_len % 2 != 0:
        raise LlxError(f"build_cache: kv_dtype='fp8' needs an even max_seq_len (got {config.max_seq_len}): beams move two positions per 256-byte row")


class KVCache(nn.Module):
    """kv_dtype "bf16": the reference's cache in `dtype`.  "fp8": uint8 buffers of OCP E4M3 codes without a scale - uint8,
    not torch.float8_e4m3fn, so that module.to(dtype) cannot cast them; the cache behaves as a bf16 cache that holds dq(q(x)) wherever
    that one holds x.  Device only: there is no CPU path."""

    def __init__(self, batch_size: int, config: LlamaConfig, dtype: torch.dtype, kv_dtype: str = "bf16"):
        super().__init__()
        check_kv_dtype(kv_dtype, config)
        self.kv_dtype = kv_dtype
        shape = (batch_size, config.num_kv_heads, config.max_seq_len, config.head_dim)
        if kv_dtype == "fp8":
            dtype = torch.uint8  # code 0x00 = +0
        self.register_buffer("k_cache", torch.zeros(shape, dtype=dtype), persistent=False)
        self.register_buffer("v_cache", torch.zeros(shape, dtype=dtype), persistent=False)

    def dequantize(self) -> tuple[Tensor, Tensor]:
        """The bf16 images (dq(k_cache), dq(v_cache)) of an fp8 cache: built for the call, never kept (tests and the prefill branch)."""
        if self.kv_dtype != "fp8":
            raise LlxError("KVCache.dequantize: a bf16 cache has no codes to dequantise")
        return K.kv_dequantize(self.k_cache), K.kv_dequantize(self.v_cache)

    def update(self, input_pos: Tensor, k: Tensor, v: Tensor):
        # input_pos: [S], or [B, S] (sequence b at its own positions); k/v: [B, KVH, S, hd]
        assert input_pos.shape[-1] == k.shape[2], (input_pos.shape, k.shape)
        if self.kv_dtype == "fp8":  # q(k), q(v) into the codes; returns the code tensors
            if not (k.is_cuda and self.k_cache.is_cuda):
                raise LlxError("an fp8 KV cache runs on the HIP device only; there is no CPU path")
            if not (k.dtype is torch.bfloat16 and k.shape[0] == self.k_cache.shape[0] and k.stride(3) == 1 and v.stride(3) == 1):
                raise LlxError(f"an fp8 KV cache takes bf16 k / v [B = {self.k_cache.shape[0]}, KVH, S, 128] with a dense last dim "
                               f"(got {k.dtype} {tuple(k.shape)})")
            if k.stride() != v.stride():
                k, v = k.contiguous(), v.contiguous()
            K.kv_scatter(k, v, self.k_cache, self.v_cache, input_pos)
            return self.k_cache, self.v_cache
        if k.is_cuda and k.dtype is torch.bfloat16 and k.shape[0] == self.k_cache.shape[0] and k.stride() == v.stride() and k.stride(3) == 1:
            K.kv_scatter(k, v, self.k_cache, self.v_cache, input_pos)  # both caches from one HIP launch, straight from the q|k|v buffer's views
        elif input_pos.dim() == 2:
            for b in range(k.shape[0]):
                self.k_cache[b, :, input_pos[b]] = k[b]
                self.v_cache[b, :, input_pos[b]] = v[b]
        else:
            self.k_cache[:, :, input_pos] = k
            self.v_cache[:, :, input_pos] = v
        return self.k_cache, self.v_cache


def _as_maskspec(block_mask):
    if block_mask is None or isinstance(block_mask, MaskSpec):
        return block_mask
    raise LlxError(
        "block_mask must be an llx MaskSpec(doc_ids=..., prefix_len=...) or MaskSpec(dense=bool_mask) - FlexAttention BlockMask "
        "objects are not dispatched on this platform: build the mask with MaskSpec.from_mask_mod(mask_mod, B, S, device)"
    )


def _refuse_block_mask_with_dropout(p: float, block_mask) -> None:
    """Train mode with attn_dropout set and an explicit block_mask=: refused, before any launch."""
    if isinstance(block_mask, MaskSpec) and block_mask.dense is not None:
        raise LlxError(f"attn_dropout={p} in train mode with block_mask=MaskSpec(dense=...): the mask-driven kernels have no dropout - "
                       "set attn_dropout=0 or call model.eval()")
    if block_mask is not None:
        raise LlxError(f"attn_dropout={p} in train mode with an explicit block_mask=: the reference's flex_attention branch applies no "
                       "dropout, so the field would be ignored - set attn_dropout=0, or pass the mask as mask=")


# ------------------------------------------------------------------------------------------------- blocks
class Attention(nn.Module):
    def __init__(self, config: LlamaConfig) -> None:
        super().__init__()
        self.num_heads = config.num_heads
        self.num_kv_heads = config.num_kv_heads
        self.embed_dim = config.embed_dim
        self.attn_dropout = config.attn_dropout
        self.head_dim = config.head_dim

        self.wq = Linear(self.embed_dim, self.num_heads * self.head_dim, bias=False)
        self.wk = Linear(self.embed_dim, self.num_kv_heads * self.head_dim, bias=False)
        self.wv = Linear(self.embed_dim, self.num_kv_heads * self.head_dim, bias=False)
        self.wo = Linear(self.num_heads * self.head_dim, self.embed_dim, bias=False)
        self.kv_cache = None
        self.dropout_stream_id = 0  # which mask stream of a step this module draws from: Llama.__init__ assigns the layer index

    def plans(self):
        return ops.GroupPlan((self.wq, self.wk, self.wv)), ops.GroupPlan((self.wo,))

    def _dropout(self) -> bool:
        """Attention dropout is active: train mode and 0 < attn_dropout < 1 (the reference: ``self.attn_dropout if self.training else 0.0``)."""
        if not self.training or self.attn_dropout == 0.0:
            return False
        if not (isinstance(self.attn_dropout, (int, float)) and 0.0 < self.attn_dropout < 1.0):
            raise LlxError(f"attn_dropout={self.attn_dropout!r} must lie in [0, 1)")
        return True

    def _run(self, x: Tensor, rope: Tensor, norm: nn.Module | None, residual: bool, mask, input_pos, block_mask, plans=None,
             attn_ticket: Tensor | None = None) -> Tensor:
        drop = self._dropout()
        mask_arg_none = mask is None  # (a recognised dense mask= becomes a block_mask below)
        if mask is not None and self.kv_cache is None and torch.is_grad_enabled() and (
                x.requires_grad or any(p.requires_grad for p in self.parameters()) or (norm is not None and norm.weight.requires_grad)):
            # training through the reference's dense-mask route (llama.py:135-137): a mask that the MaskSpec rule reproduces exactly
            # (causal / prefix-LM / contiguous documents) runs on the fused kernels with their backward; anything else trains through
            # block_mask=MaskSpec(dense=mask) (this route keeps the reference's mask= semantics and does not guess)
            spec = ops._cached(mask, "maskspec", lambda: (K.maskspec_from_dense(mask, x.shape[0], x.shape[1]),))[0]
            if spec is None and drop:
                raise LlxError(f"attn_dropout={self.attn_dropout} with a dense mask= that is not of the form (k <= q or k < prefix[b]) and "
                               "same-document: the mask-driven kernels have no dropout - use a mask of that form or set attn_dropout=0")
            if spec is None:
                raise LlxError("training with a dense mask= needs a mask of the form (k <= q or k < prefix[b]) and same-document "
                               "(contiguous documents): pass block_mask=MaskSpec(dense=mask) to train through any other bool mask")
            mask, block_mask = None, (spec if (spec.doc_ids is not None or spec.prefix_len is not None) else None)
        if self.kv_cache is not None or mask is not None:
            return self._run_dense(x, rope, norm, residual, mask, input_pos)
        dropout = None
        if drop:
            # Dropout applies where the reference's SDPA branch runs: no mask (causal) and a dense mask= recognised as a rule (above).
            # Its flex_attention branch (block_mask=) applies none, so an explicit block_mask with attn_dropout set is refused, not ignored.
            if mask_arg_none:
                _refuse_block_mask_with_dropout(self.attn_dropout, block_mask)
            dropout = (K.attn_dropout_threshold(self.attn_dropout), int(self.dropout_stream_id))
            if attn_ticket is None:  # a stand-alone Attention / TransformerLayer draws its own
                attn_ticket = ops.attn_dropout_ticket(x.device)
        qkv, wo = plans or self.plans()
        meta = ops.AttnBlockMeta(qkv, wo, self.num_heads, self.num_kv_heads, self.head_dim, _as_maskspec(block_mask),
                                 norm.eps if norm is not None else 0.0, norm is not None, residual, dropout)
        tensors = qkv.tensors() + wo.tensors()
        return ops.AttnBlockFn.apply(x, _rope_f32(rope), norm.weight if norm is not None else None, meta, attn_ticket if drop else None, *tensors)

    def _run_dense(self, x: Tensor, rope: Tensor, norm, residual: bool, mask, input_pos) -> Tensor:
        """Inference path: KV cache and/or an explicit bool mask (SDPA branch with is_causal=False, llama.py:126-127,135-137).
        Forward only: training uses block_mask=MaskSpec(...) - the rule or dense=mask - which has a fused backward."""
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise LlxError("dense-mask / KV-cache attention is forward-only here: run it under torch.no_grad() "
                           "(for training use block_mask=MaskSpec(doc_ids=..., prefix_len=...) or MaskSpec(dense=mask))")
        B, L_, _ = x.shape
        H, KVH, hd = self.num_heads, self.num_kv_heads, self.head_dim
        xn = norm(x) if norm is not None else x
        x2 = K._rows2d(xn.contiguous())
        qkv = torch.empty(B * L_, (H + 2 * KVH) * hd, device=x.device, dtype=x.dtype)
        ops.GroupPlan((self.wq, self.wk, self.wv)).forward(x2, qkv, cached_scale=True)  # forward-only: DoRA's row factors come from their cache
        qkv3 = qkv.view(B, L_, -1)
        K.rope_(qkv3, _rope_f32(rope).contiguous(), H + KVH)
        q = qkv3[..., : H * hd].unflatten(-1, (H, hd)).transpose(1, 2)
        k = qkv3[..., H * hd : (H + KVH) * hd].unflatten(-1, (KVH, hd)).transpose(1, 2)
        v = qkv3[..., (H + KVH) * hd :].unflatten(-1, (KVH, hd)).transpose(1, 2)
        if self.kv_cache is not None:
            k, v = self.kv_cache.update(input_pos, k, v)
        if mask is None:  # no cache, no mask cannot reach here; a cache without mask attends to everything cached
            mask = torch.ones(L_, k.shape[2], dtype=torch.bool, device=x.device)
        decode = L_ * (H // KVH) <= 16 and k.stride() == v.stride()
        if k.dtype is torch.uint8 and not decode:
            # an fp8 cache past the decode branch (which reads the codes): the existing kernels on a transient bf16 image of the cache,
            # dequantised for this call and dropped after it (two launches per layer; tools/decode_kv8_bench.py times them)
            k, v = self.kv_cache.dequantize()
        if decode:  # a few query tokens over a long cache: split-cache decode kernel
            o2 = K.attn_decode(q, k, v, mask, D.mask_extent(mask)).view(B * L_, H * hd)
        elif K.attn_mask_routable(mask, B, L_, k.shape[2]):
            # prefill / explicit mask broadcast over heads: the MFMA tile loop driven by the mask bytes, o written as rows.  No range of small
            # L stays on the per-row kernel: at the smallest shape past the decode branch (8 tokens at position 4096 of an 8192 cache,
            # 8B heads) the attention call takes 0.12 ms here against 1.37 ms there, 0.18 against 25.2 ms at 4096 tokens
            # (tools/prefill_bench.py, profiles/prefill_bench.json): no crossover was found.
            o2 = K.attn_mask_fwd(q, k, v, mask).view(B * L_, H * hd)
        else:  # per-head masks
            o2 = K.attn_dense_fwd(q, k, v, mask).transpose(1, 2).reshape(B * L_, H * hd)  # [B,H,L,hd] -> rows
        y, _ = ops.GroupPlan((self.wo,)).forward(o2, None, K._rows2d(x.contiguous()) if residual else None, cached_scale=True)
        return y.view(B, L_, -1)

    def forward(self, x: Tensor, rope: Tensor, *, mask: Tensor | None = None, input_pos: Tensor | None = None,
                block_mask=None, attn_ticket: Tensor | None = None) -> Tensor:
        return self._run(x, rope, None, False, mask, input_pos, block_mask, attn_ticket=attn_ticket)


class FeedForward(nn.Module):
    def __init__(self, config: LlamaConfig):
        super().__init__()
        self.w1 = Linear(config.embed_dim, config.intermediate_dim, bias=False)
        self.w3 = Linear(config.embed_dim, config.intermediate_dim, bias=False)
        self.w2 = Linear(config.intermediate_dim, config.embed_dim, bias=False)
        self.act = nn.SiLU()

    def plans(self):
        return ops.GroupPlan((self.w1, self.w3)), ops.GroupPlan((self.w2,))

    def _run(self, x: Tensor, norm: nn.Module | None, residual: bool, plans=None) -> Tensor:
        w13, w2 = plans or self.plans()
        meta = ops.MLPBlockMeta(w13, w2, norm.eps if norm is not None else 0.0, norm is not None, residual)
        tensors = w13.tensors() + w2.tensors()
        return ops.MLPBlockFn.apply(x, norm.weight if norm is not None else None, meta, *tensors)

    def forward(self, x: Tensor) -> Tensor:
        return self._run(x, None, False)


class TransformerLayer(nn.Module):
    def __init__(self, config: LlamaConfig) -> None:
        super().__init__()
        self.attention_norm = RMSNorm(config.embed_dim, eps=1e-5)
        self.attention = Attention(config)
        self.ffn_norm = RMSNorm(config.embed_dim, eps=1e-5)
        self.feed_forward = FeedForward(config)

    def forward(self, x: Tensor, rope: Tensor, *, mask: Tensor | None = None, input_pos: Tensor | None = None,
                block_mask=None, attn_ticket: Tensor | None = None) -> Tensor:
        # x + attention(attention_norm(x)) and x + feed_forward(ffn_norm(x)), each as one fused autograd node
        if D.layer_ok(self, x, mask) and not (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))):
            return D.layer_forward(self, x, _rope_f32(rope).contiguous(), mask, input_pos)  # decode: every linear a weight stream
        if mask is None and self.attention.kv_cache is None and self.attention._dropout():
            _refuse_block_mask_with_dropout(self.attention.attn_dropout, block_mask)
        pa = pf = None
        if x.is_cuda and self.attention.kv_cache is None and mask is None:
            pa, pf = self.attention.plans(), self.feed_forward.plans()
            ops.prepack((*pa, *pf))  # the LoRA operand images of the layer's four linear groups from one launch
        x = self.attention._run(x, rope, self.attention_norm, True, mask, input_pos, block_mask, pa, attn_ticket)
        return self.feed_forward._run(x, self.ffn_norm, True, pf)


class Llama(nn.Module):
    def __init__(self, config: LlamaConfig) -> None:
        super().__init__()
        self.tok_embeddings = Embedding(config.vocab_size, config.embed_dim)
        self.layers = nn.ModuleList([TransformerLayer(config) for _ in range(config.num_layers)])
        for i, layer in enumerate(self.layers):
            layer.attention.dropout_stream_id = i  # attention dropout: every layer draws its own mask from the step's ticket
        self.norm = RMSNorm(config.embed_dim, eps=1e-5)
        self.output = Linear(config.embed_dim, config.vocab_size, bias=False)
        self.config = config

    def build_cache(self, inference: bool = False, batch_size: int = 1, kv_dtype: str = "bf16"):
        """The RoPE table and, for inference, a KV cache of `batch_size` sequences per layer (the reference's KVCache, update() and
        Attention.forward are written for a batch; only its build_cache fixes the batch at 1).  kv_dtype="fp8": caches of E4M3 codes,
        half the bytes (KVCache); refused, before anything is allocated, for head_dim != 128 or an odd max_seq_len."""
        check_kv_dtype(kv_dtype, self.config)
        self.register_buffer("rope", build_rope(self.config), persistent=False)
        if inference:
            if not (isinstance(batch_size, int) and batch_size >= 1):
                raise LlxError(f"build_cache: batch_size={batch_size!r} must be an integer >= 1")
            for layer in self.layers:
                layer.attention.kv_cache = KVCache(batch_size, self.config, self.tok_embeddings.weight.dtype, kv_dtype)
            L = self.config.max_seq_len
            self.register_buffer("causal_mask", torch.tril(torch.ones(L, L, dtype=torch.bool)), persistent=False)

    def _run_layers(self, x: Tensor, rope: Tensor, lo: int = 0, hi: int | None = None, **kw) -> Tensor:
        if self.training and self.config.attn_dropout != 0.0 and kw.get("input_pos") is None and x.is_cuda:
            K.attn_dropout_threshold(self.config.attn_dropout)  # (the range check, before any launch)
            _refuse_block_mask_with_dropout(self.config.attn_dropout, kw.get("block_mask"))
            # one ticket per step (two launches on the device, no host read); the layers differ by their stream ids, and a layer that is
            # recomputed under activation checkpointing gets the same ticket again
            kw["attn_ticket"] = ops.attn_dropout_ticket(x.device)
        for layer in self.layers[lo:hi]:
            if self.config.activation_checkpointing:
                x = checkpoint(layer, x, rope, use_reentrant=False, **kw)
            else:
                x = layer(x, rope, **kw)
        return x

    def _head(self, x: Tensor, labels: Tensor | None) -> Tensor:
        if labels is None:
            if D.head_ok(self, x) and not (torch.is_grad_enabled() and (x.requires_grad or self.output.weight.requires_grad or self.norm.weight.requires_grad)):
                return D.head_forward(self, x)
            return self.output(self.norm(x))
        plan = ops.LinearPlan(self.output)
        return ops.HeadLossFn.apply(x, self.norm.weight, labels, self.norm.eps, plan, *plan.tensors())

    def _embed(self, x: Tensor) -> tuple[Tensor, int]:
        """(hidden states [B, S, D], number of leading positions that are dropped before the head)."""
        return self.tok_embeddings(x), 0

    def _inference_mask(self, batch: int, input_pos: Tensor | None) -> Tensor | None:
        """The attention mask of a call of `batch` sequences at input_pos (None: not the inference path)."""
        if input_pos is None:
            return None
        cache = self.layers[0].attention.kv_cache if len(self.layers) else None
        if cache is not None and batch != cache.k_cache.shape[0]:
            raise LlxError(f"batch of {batch} against a KV cache of batch {cache.k_cache.shape[0]}: "
                           f"call build_cache(inference=True, batch_size={batch})")
        if input_pos.dim() == 2:
            # [B, L]: sequence b writes its keys and values at input_pos[b] and attends through causal_mask[input_pos[b]]
            if input_pos.shape[0] != batch:
                raise LlxError(f"input_pos {tuple(input_pos.shape)} must be [L] or [B, L] with B = {batch}")
            return self.causal_mask[input_pos][:, None]  # [B, 1, L, Skv]
        return self.causal_mask[None, None, input_pos]

    def _hidden(self, x: Tensor, input_pos: Tensor | None = None, block_mask=None) -> Tensor:
        """forward() up to the head: the hidden states [B, S, D] after the last layer."""
        mask = self._inference_mask(x.shape[0], input_pos)
        x, _ = self._embed(x)
        rope = self.rope[: x.shape[1]]
        return self._run_layers(x, rope, mask=mask, input_pos=input_pos, block_mask=block_mask)

    def forward(self, x: Tensor, *, input_pos: Tensor | None = None, block_mask=None, labels: Tensor | None = None) -> Tensor:
        return self._head(self._hidden(x, input_pos, block_mask), labels)

    def token_logprobs(self, tokens: Tensor, labels: Tensor, *, block_mask=None, return_top1: bool = False, top_k: int = 0):
        """fp32 [B, S] log-probabilities of ``labels`` under the model, ``-F.cross_entropy(logits.float(), labels, reduction="none",
        ignore_index=-100)`` - the per-token terms of the mean that ``forward(labels=...)`` returns - without materialising the logits
        in fp32, 0.0 where labels == -100, differentiable.  return_top1: also the int32 [B, S] argmax of every labelled position
        (-1 at the others): token accuracy from the same pass.  top_k = k in 1..8: also, last, ``top_ids`` (int32) and ``top_logp``
        (fp32) [B, S, k], the k likeliest tokens of every labelled position and their log-probabilities, descending, equal logits by
        ascending index (``top_ids[..., 0]`` is top1), -1 / 0.0 at the others, detached; an alternative that is the label carries
        the label's logp bit for bit.  Train and eval mode; not the KV-cache path (no input_pos)."""
        ops._check_labels(labels, tokens.shape, tokens.device, "token_logprobs")
        ops._check_top_k(top_k, "token_logprobs: top_k")
        return ops.head_logprobs(self._hidden(tokens, None, block_mask), self.norm, self.output, labels, return_top1, top_k)

    def generate(self, prompt: Tensor, max_new_tokens: int, **kwargs) -> Tensor:
        """llx.generate.generate(self, ...): prefill + one forward and one on-device sampler launch per token (the reference has no
        generate(); its input_pos branch above is what this drives).  prompt [B, P] with B the cache's batch; prompt_lens=... for
        right-padded prompts of different lengths; draft_tokens=k (greedy, one sequence) feeds k prompt-lookup draft tokens with every
        step and keeps the ones the model confirms: the same tokens in fewer weight passes; num_beams=W (one prompt, a cache of batch
        W) is beam search with the beams as the rows of one batched step; repetition_penalty / presence_penalty / frequency_penalty
        penalise the tokens a row has seen and return_logprobs=True also returns each token's log-probability, both inside the
        sampler launch."""
        from llx.generate import generate

        return generate(self, prompt, max_new_tokens, **kwargs)

    @staticmethod
    def from_hf(model_id: str, **kwargs):
        config = _get_hf_config(model_id)._replace(**kwargs)
        with torch.device("meta"):
            model = Llama(config).eval()
        # the cache cannot be built under the meta device: load (assign) first, then build
        model.load_state_dict(_get_hf_state_dict(model_id), assign=True)
        model.build_cache()
        return model


# ------------------------------------------------------------------------------------------------- HF loading
def _hf_file(model_id: str, filename: str) -> str:
    """A local checkpoint directory is used as is; otherwise the hub is asked (needs network, as in the reference)."""
    if os.path.isdir(model_id):
        return os.path.join(model_id, filename)
    from huggingface_hub import hf_hub_download

    return hf_hub_download(model_id, filename)


def _hf_list(model_id: str) -> list[str]:
    if os.path.isdir(model_id):
        return sorted(os.listdir(model_id))
    from huggingface_hub import list_repo_files

    return list_repo_files(model_id)


def _get_hf_config(model_id: str) -> LlamaConfig:
    with open(_hf_file(model_id, "config.json")) as f:
        hf = json.load(f)
    assert hf["architectures"][0] == "LlamaForCausalLM"
    config = LlamaConfig(
        embed_dim=hf["hidden_size"],
        num_layers=hf["num_hidden_layers"],
        head_dim=hf.get("head_dim", hf["hidden_size"] // hf["num_attention_heads"]),
        num_heads=hf["num_attention_heads"],
        num_kv_heads=hf["num_key_value_heads"],
        intermediate_dim=hf["intermediate_size"],
        vocab_size=hf["vocab_size"],
    )
    if "rope_theta" in hf:
        config = config._replace(rope_base=hf["rope_theta"])
    if hf.get("rope_scaling", None) is not None:
        config = config._replace(is_llama3_1=hf["rope_scaling"]["rope_type"] == "llama3")
    return config


_HF_RENAMES = (
    ("embed_tokens", "tok_embeddings"),
    ("self_attn.q_proj", "attention.wq"),
    ("self_attn.k_proj", "attention.wk"),
    ("self_attn.v_proj", "attention.wv"),
    ("self_attn.o_proj", "attention.wo"),
    ("mlp.gate_proj", "feed_forward.w1"),
    ("mlp.up_proj", "feed_forward.w3"),
    ("mlp.down_proj", "feed_forward.w2"),
    ("input_layernorm", "attention_norm"),
    ("post_attention_layernorm", "ffn_norm"),
    ("lm_head", "output"),
)


def _rename_hf_key(key: str) -> str:
    key = key.removeprefix("model.")
    for old, new in _HF_RENAMES:
        key = key.replace(old, new)
    return key


def _get_hf_state_dict(model_id: str) -> dict:
    names = _hf_list(model_id)
    filenames = [n for n in names if n.endswith(".safetensors")] or [n for n in names if n.endswith(".bin")]
    if not filenames:
        raise RuntimeError(f"No weights found for {model_id=}")
    state = {}
    for name in filenames:
        path = _hf_file(model_id, name)
        if path.endswith(".safetensors"):
            import safetensors

            with safetensors.safe_open(path, framework="pt") as f:
                for k in f.keys():
                    state[k] = f.get_tensor(k)
        else:
            state.update(torch.load(path, map_location="cpu", weights_only=True, mmap=True))
    return {_rename_hf_key(k): v for k, v in state.items()}
