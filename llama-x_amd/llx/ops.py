"""Autograd layer over the HIP kernels: per-linear plans (dense / LoRA / int8) and fused block functions.

One ``torch.autograd.Function`` per residual branch keeps the host-side graph small (2 nodes per transformer
layer) and lets the forward write q|k|v and gate|up into fused buffers that the attention / SwiGLU kernels
read through strides.  Frozen base weights get a cached transposed copy (HBM is 288 GB; a second 16 GB image
of Llama-3.1-8B is cheap) so that every data-gradient is the same tuned NT GEMM as the forward.

Reference semantics reproduced here: modelling/llama.py:108-174,196-219 ; modelling/lora.py:40-44 ;
subclasses/int8.py:106-130.
"""
from __future__ import annotations

import os

from typing import NamedTuple, Optional, Sequence

import torch
from torch import Tensor, nn
from torch.autograd import Function

from . import kernels as K
from ._lib import LlxError

BF16 = torch.bfloat16


# =================================================================================================
# cached derived images of (mostly frozen) weights
# =================================================================================================
def _cached_multi(tensors: Sequence[Tensor], tag: str, build):
    """Cache ``build()`` (any value) on the first tensor, keyed by the version counters and devices of all of them: an in-place update
    or a move of any source invalidates."""
    store = tensors[0].__dict__.setdefault("_llx_cache", {})
    key = tuple((t._version, str(t.device)) for t in tensors)
    hit = store.get(tag)
    if hit is not None and hit[0] == key:
        return hit[1]
    val = build()
    store[tag] = (key, val)
    return val


def _cached(t: Tensor, tag: str, build):
    return _cached_multi([t], tag, build)


def weight_t(w: Tensor) -> Tensor:
    """[N,K] -> cached [K,N] bf16 image (B operand of the dgrad GEMM)."""
    return _cached(w, "wt", lambda: K.transpose(w.detach()))


# =================================================================================================
# LinearPlan: how one nn.Linear (possibly LoRA-dressed, possibly int8) runs forward / backward
# =================================================================================================
class LinearPlan:
    """Execution plan of one ``nn.Linear`` child as the reference would run it:

    * plain:      F.linear(x, W, b)                                              (modelling/llama.py:118-120 ...)
    * LoRA:       F.linear(x, W, b) + x @ A^T @ B^T * (alpha/r)                  (modelling/lora.py:40-44)
    * int8 W:     _Int8Linear (weight-only or dynamic-activation)                (subclasses/int8.py:106-130)
    * MXFP4 W:    the plain / LoRA plan on a transient bf16 image of the weight  (subclasses/mxfp4.py)

    ``tensors()`` lists the tensors autograd must see; ``backward`` returns their gradients in that order.
    """

    def __init__(self, m: nn.Linear):
        from subclasses.int8 import Int8LinearWeight  # local import: subclasses imports llx too
        from subclasses.mxfp4 import MXFP4LinearWeight

        self.N, self.K = m.out_features, m.in_features
        self.weight = m.weight
        self.bias = m.bias
        self.rank = int(getattr(m, "rank", 0) or 0)
        self.lora_a = getattr(m, "lora_a", None) if self.rank > 0 else None
        self.lora_b = getattr(m, "lora_b", None) if self.rank > 0 else None
        self.scale = float(getattr(m, "scale", 1.0))
        self.dora_m = getattr(m, "m", None) if self.rank > 0 else None  # DoRALinear's magnitude vector (modelling/lora.py:51)
        self.int8 = isinstance(self.weight, Int8LinearWeight)
        self.dynamic = bool(self.int8 and self.weight.dynamic_int8_act)
        # MXFP4 weight-only: the bf16 plan on a transient image of the weight (w_image / wt_image), which is never cached - the memory
        # is the point of the format; frozen like int8 (no weight gradient)
        self.mx4 = isinstance(self.weight, MXFP4LinearWeight)
        self.no_grad = False  # set by linear(): the call runs with grad disabled
        if self.dora_m is not None and self.int8:
            # the reference cannot run this combination either: (weight + delta).norm() has no Int8LinearWeight dispatch (subclasses/int8.py:102)
            raise LlxError("DoRA on an Int8LinearWeight is not supported (nor by the reference: no dispatch for weight + delta)")
        if self.dora_m is not None and self.mx4:
            raise LlxError("DoRA on an MXFP4LinearWeight is not supported (as on int8: no dispatch for weight + delta)")
        if self.rank > 64:
            raise LlxError(f"LoRA rank {self.rank} > 64 is not supported by the skinny kernels")
        if self.rank > 0 and self.lora_a.dtype is not BF16:
            raise LlxError("LoRA factors must be bf16")

    # ---- autograd-visible tensors
    def tensors(self) -> list[Tensor]:
        ts = []
        if not self.int8 and not self.mx4:
            ts.append(self.weight)
        if self.bias is not None:
            ts.append(self.bias)
        if self.rank > 0:
            ts += [self.lora_a, self.lora_b]
        if self.dora_m is not None:
            ts.append(self.dora_m)
        return ts

    # ---- the bf16 operand images of the base weight: the weight itself and its cached transpose, or - MXFP4 - transient images
    def w_image(self) -> Tensor:
        return K.dequantize_mxfp4(self.weight.packed, self.weight.scale) if self.mx4 else self.weight.detach()

    def wt_image(self) -> Tensor:
        return K.dequantize_mxfp4(self.weight.packed, self.weight.scale, transpose=True) if self.mx4 else weight_t(self.weight)

    # ---- forward: y = linear(x) [+ residual]; returns (y, saved) where saved is the LoRA intermediate t = x @ A^T
    # (DoRA: the tuple (t, z, c, inv_norm) - un-scaled output, column scale m / ||W + sBA||, 1 / norm)
    # cached_scale: no backward will follow (the caller's inputs need no gradient): DoRA's c comes from dora_scale_cached, inv_norm is not made
    def forward(self, x: Tensor, out: Optional[Tensor] = None, residual: Optional[Tensor] = None, gelu: bool = False, cached_scale: bool = False):
        t = b2 = None
        if self.rank > 0:
            t = K.skinny_nt(x, self.lora_a.detach())
            b2 = K.pad64(self.lora_b.detach(), self.scale)
        if self.dora_m is not None:
            if gelu:
                raise LlxError("DoRA + GELU epilogue is not supported")
            w = self.weight.detach()
            c, inv = (dora_scale_cached(self), None) if cached_scale else dora_colscale([self], w, self.lora_a.detach(), b2)
            z = K.gemm_nt(x, w, a2=t, b2=b2, k2_eff=self.rank)
            direct = residual is None
            y = K.colscale_bias(z, c, self.bias.detach() if self.bias is not None else None, out=out if direct else None)
            if residual is not None:
                y = K.add(y, residual, out=out)
            return y, (t, z, c, inv)
        if self.int8:
            from subclasses.int8 import int8_linear_forward

            if self.bias is not None or gelu:
                raise LlxError("int8 linear with bias is not on the fused path")
            # (x @ W8^T) * scale is rounded to bf16 first (subclasses/int8.py:118); adapter and residual are added after
            direct = self.rank == 0 and residual is None
            y = int8_linear_forward(x, self.weight, out=out if direct else None)
            if self.rank > 0:
                y = K.gemm_nt(t, b2, out=out if residual is None else None, epilogue=K.EPI_RESIDUAL, e=y, k2_eff=0)
            if residual is not None:
                y = K.add(y, residual, out=out)
            return y, t
        w = self.w_image()
        if self.bias is not None:
            if residual is not None:
                raise LlxError("bias + residual epilogue is not supported")
            y = K.gemm_nt(x, w, out=out, a2=t, b2=b2, epilogue=K.EPI_BIAS_GELU if gelu else K.EPI_BIAS, e=self.bias.detach(), k2_eff=self.rank)
        elif residual is not None:
            y = K.gemm_nt(x, w, out=out, a2=t, b2=b2, epilogue=K.EPI_RESIDUAL, e=residual, k2_eff=self.rank)
        else:
            y = K.gemm_nt(x, w, out=out, a2=t, b2=b2, k2_eff=self.rank)
        return y, t

    # ---- backward: grads of tensors() and (optionally) dx (accumulated into dx_out when dx_accum)
    def backward(self, dy: Tensor, x: Tensor, t: Optional[Tensor], needs: Sequence[bool], need_dx: bool = True,
                 dx_out: Optional[Tensor] = None, dx_accum: bool = False):
        grads: list[Optional[Tensor]] = []
        ni = iter(needs)
        u = None
        dy_out, gm = dy, None
        if self.dora_m is not None:  # out = z * c (+ bias): d m = colsum(dy * z) / norm, and everything upstream sees dz = dy * c
            t, z, c, inv = t
            if needs[-1]:
                gm = K.colsum_mul(dy, z, inv)
            dy = K.scale(dy, colscale=c)
        if self.rank > 0:
            u = K.skinny_nt(dy, K.transpose(self.lora_b.detach()))  # dy @ B  -> [M,64]
        # --- parameter gradients, in tensors() order
        if not self.int8 and not self.mx4:
            grads.append(K.gemm_tn(dy, x) if next(ni) else None)
        if self.bias is not None:
            grads.append(K.colsum(dy_out) if next(ni) else None)  # the bias is added after the DoRA rescale
        if self.rank > 0:
            need_a, need_b = next(ni), next(ni)
            ga = gb = None
            if need_a:
                ga = _grad_dst([self.lora_a], (self.rank, self.K))
                if ga is None:
                    ga = torch.empty(self.rank, self.K, device=dy.device, dtype=BF16)
                K.skinny_tn(u, x, self.rank, self.scale, ga, transpose_out=False)
            if need_b:
                gb = _grad_dst([self.lora_b], (self.N, self.rank))
                if gb is None:
                    gb = torch.empty(self.N, self.rank, device=dy.device, dtype=BF16)
                K.skinny_tn(t, dy, self.rank, self.scale, gb, transpose_out=True)
            grads += [ga, gb]
        if self.dora_m is not None:
            grads.append(gm)
        # --- data gradient
        dx = None
        if need_dx:
            b2 = K.pad64(self.lora_a.detach(), self.scale, transposed=True) if self.rank > 0 else None
            if self.int8:
                from subclasses.int8 import int8_weight_t

                g = K.scale(dy, colscale=self.weight.scale)  # (g * scale) rounded to bf16 (subclasses/int8.py:127)
                wt = int8_weight_t(self.weight)
            else:
                g = dy
                wt = self.wt_image()
            if dx_accum:
                dx = K.gemm_nt(g, wt, out=dx_out, a2=u, b2=b2, epilogue=K.EPI_RESIDUAL, e=dx_out, k2_eff=self.rank)
            else:
                dx = K.gemm_nt(g, wt, out=dx_out, a2=u, b2=b2, k2_eff=self.rank)
        return dx, grads


def dora_colscale(members: Sequence[LinearPlan], w_cat: Tensor, a_cat: Tensor, b2: Tensor, wn2_tag: str = "wn2") -> tuple[Tensor, Tensor]:
    """DoRA's per-output-row factor for one linear or a fused group (modelling/lora.py:55-59, norm detached from A and B):
    c [N] bf16 = m / ||W + s B A||_row and inv_norm [N] fp32, from ||W_n||^2 (cached with the frozen weight), G = W A^T and A A^T -
    W is read once by the skinny MFMA kernel, no [out, in] temporary is formed.  b2 = the [N, 64] image of s * B (block diagonal)."""
    N, R = w_cat.shape[0], a_cat.shape[0]
    wn2 = _cached_multi([m.weight for m in members], wn2_tag, lambda: K.rownorm2(w_cat))
    G = K.skinny_nt(w_cat, a_cat)
    AAt = K.skinny_nt(a_cat, a_cat)
    c = torch.empty(N, device=w_cat.device, dtype=BF16)
    inv = torch.empty(N, device=w_cat.device, dtype=torch.float32)
    off = 0
    for m in members:
        sl = slice(off, off + m.N)
        K.dora_colscale(wn2[sl], G[sl], b2[sl], AAt, m.dora_m.detach(), c[sl], inv[sl], R)
        off += m.N
    return c, inv


def dora_scale_cached(m) -> Tensor:
    """c [out_features] bf16 = m / ||W + s B A||_row of ONE DoRA linear (an nn.Linear dressed by modelling/lora.py, or its LinearPlan),
    built once by dora_colscale and kept on the weight: the factor depends on parameters only, so a forward that no backward follows
    (decode, prefill, eval loss) need not read W a second time per call.  Per member, never from a concatenated image: the decode path
    keeps no second copy of a weight.  Next to it stays ||W_n||^2 (fp32, tag "wn2m"): 6 bytes per output row in all.

    The cache key is the version counter and device of weight, lora_a, lora_b and m: an optimizer step, load_state_dict, any in-place
    update under no_grad or a move of one of them rebuilds it.  What the key cannot see - as for the "wn2" and "wt" images: a write
    through .data (or any other write that bypasses the version counter) leaves a stale factor; bump the version (p.add_(0) under
    no_grad) or drop p._llx_cache after such a write."""
    plan = m if isinstance(m, LinearPlan) else None
    mag = plan.dora_m if plan is not None else m.m

    def build():
        p = plan if plan is not None else LinearPlan(m)
        c, _ = dora_colscale([p], p.weight.detach(), p.lora_a.detach(), K.pad64(p.lora_b.detach(), p.scale), wn2_tag="wn2m")
        return c

    return _cached_multi([m.weight, m.lora_a, m.lora_b, mag], "dora_c", build)


class GroupPlan:
    """Linears that read the SAME input (wq|wk|wv, w1|w3), executed as one GEMM over concatenated weight images.

    Forward: y[M, sum N] = x @ [W_0; W_1; ...]^T with the members' LoRA adapters batched into one skinny product
    (t = x @ [A_0; A_1; ...]^T, 64 columns) and one block-diagonal K-extension operand; backward: one dgrad GEMM over the
    concatenated transposed image (K = sum N) and one skinny product per adapter factor.  Better tile quantisation
    (1792 tiles = 7 full waves for gate|up instead of 2 x 3.5), a third of the launches, x / dy read once.
    Falls back to per-member plans when the members cannot be fused (mixed kinds, biases, sum of ranks > 64)."""

    def __init__(self, mods: Sequence[nn.Linear]):
        self.members = [LinearPlan(m) for m in mods]
        m0 = self.members[0]
        self.K = m0.K
        self.Ns = [m.N for m in self.members]
        self.N = sum(self.Ns)
        self.n_off = [sum(self.Ns[:i]) for i in range(len(self.Ns))]
        self.ranks = [m.rank for m in self.members]
        self.R = sum(self.ranks)
        self.r_off = [sum(self.ranks[:i]) for i in range(len(self.ranks))]
        same_kind = all((m.int8, m.dynamic, m.mx4) == (m0.int8, m0.dynamic, m0.mx4) for m in self.members)
        same_scale = len({m.scale for m in self.members if m.rank > 0}) <= 1
        lora_all_or_none = all(r > 0 for r in self.ranks) or self.R == 0
        dora_all_or_none = len({m.dora_m is not None for m in self.members}) == 1
        self.dora = all(m.dora_m is not None for m in self.members)
        self.fused = (same_kind and same_scale and lora_all_or_none and dora_all_or_none and self.R <= 64
                      and all(m.bias is None for m in self.members) and all(m.K == self.K for m in self.members))
        self.int8, self.dynamic, self.mx4 = m0.int8, m0.dynamic, m0.mx4
        self.packed = None  # (a_cat, b2, bT, a2t) when prepack() built the LoRA operand images of several groups in one launch
        self.scale = next((m.scale for m in self.members if m.rank > 0), 1.0)
        # true contraction length of the (block-diagonal, zero-padded) LoRA K-extension: forward sum_i N_i r_i / N, dgrad R
        self.k2_fwd = sum(n * r for n, r in zip(self.Ns, self.ranks)) / self.N

    def tensors(self) -> list[Tensor]:
        return [t for m in self.members for t in m.tensors()]

    # ---- cached concatenated images of the (normally frozen) base weights
    def _weights(self):
        return [(m.weight.int_data if m.int8 else m.weight) for m in self.members]

    def _mx4_image(self, transpose: bool) -> Tensor:
        """MXFP4 members: their bf16 images side by side, [sum N, K] or transposed [K, sum N] - built per call and dropped after it."""
        out = torch.empty((self.K, self.N) if transpose else (self.N, self.K), device=self.members[0].weight.device, dtype=BF16)
        for m, o, n in zip(self.members, self.n_off, self.Ns):
            K.dequantize_mxfp4(m.weight.packed, m.weight.scale, transpose=transpose, out=out[:, o : o + n] if transpose else out[o : o + n])
        return out

    def w_cat(self) -> Tensor:
        if self.mx4:
            return self._mx4_image(False)
        ws = self._weights()
        if self.int8 and self.dynamic:
            return _cached_multi(ws, "cat_i8", lambda: torch.cat([w.detach() for w in ws], 0))
        if self.int8:
            return _cached_multi(ws, "cat_bf16", lambda: K.i8_to_bf16(torch.cat([w.detach() for w in ws], 0)))
        return _cached_multi(ws, "cat", lambda: torch.cat([w.detach() for w in ws], 0) if len(ws) > 1 else ws[0].detach())

    def wt_cat(self) -> Tensor:
        if self.mx4:
            return self._mx4_image(True)
        ws = self._weights()
        return _cached_multi(ws, "cat_t", lambda: K.transpose(torch.cat([w.detach() for w in ws], 0) if len(ws) > 1 else ws[0].detach()))

    def scale_cat(self) -> Tensor:
        ss = [m.weight.scale for m in self.members]
        return _cached_multi(ss, "cat_scale", lambda: torch.cat(ss, 0) if len(ss) > 1 else ss[0])

    def dora_scale_cached(self) -> Tensor:
        """c [sum N] of a fused DoRA group: the members' cached factors side by side (each built from its own weight)."""
        if len(self.members) == 1:
            return dora_scale_cached(self.members[0])
        srcs = [t for m in self.members for t in (m.weight, m.lora_a, m.lora_b, m.dora_m)]
        return _cached_multi(srcs, "dora_c_cat", lambda: torch.cat([dora_scale_cached(m) for m in self.members], 0))

    # ---- forward
    def forward(self, x: Tensor, out: Optional[Tensor] = None, residual: Optional[Tensor] = None, swiglu_h: Optional[Tensor] = None,
                rope: Optional[tuple[Tensor, int, int]] = None, xq: Optional[tuple[Tensor, Tensor]] = None, t_pre: Optional[Tensor] = None,
                cached_scale: bool = False):
        """out: [M, sum N] (row-strided view allowed; allocated when None).  ``residual`` [M, sum N] is added in the GEMM
        epilogue (x + linear(..), modelling/llama.py:172-173).  xq = quantize_int8_rowwise(x) / t_pre = x @ A_cat^T when the producer of
        x already made them (the RMSNorm forward).  cached_scale: no backward will follow - DoRA members take their factors from
        dora_scale_cached and `saved` is not fit for backward().  Returns (out, saved) - saved feeds backward()."""
        if out is None:
            out = torch.empty(x.shape[0], self.N, device=x.device, dtype=BF16)
        return out, self._forward(x, out, residual, swiglu_h, rope, xq, t_pre, cached_scale)

    def norm_can_make_t(self, dim: int) -> bool:
        """The preceding RMSNorm can emit t = xn @ A_cat^T itself: the operand images exist already (prepack) and the width fits."""
        return self.fused and self.R > 0 and self.packed is not None and K.rmsnorm_skinny_ok(dim)

    def wants_quantized_input(self) -> bool:
        """The fused group runs torchao::int8_mm_dequant on row-wise quantised activations (subclasses/int8.py:110-113)."""
        return self.fused and self.int8 and self.dynamic

    def rope_fusable(self) -> bool:
        """apply_rope can ride in the projection GEMM's epilogue (one fused bf16 GEMM writes the whole q|k|v row)."""
        return self.fused and (not self.int8 or self.dynamic) and not self.dora

    def swiglu_fusable(self) -> bool:
        """silu(g) * u can ride in the gate|up GEMM's epilogue."""
        return self.fused and (not self.int8 or self.dynamic) and not self.dora and len(self.members) == 2 and self.Ns[0] % 128 == 0

    def _forward(self, x: Tensor, out: Tensor, residual: Optional[Tensor], swiglu_h: Optional[Tensor] = None,
                 rope: Optional[tuple[Tensor, int, int]] = None, xq: Optional[tuple[Tensor, Tensor]] = None, t_pre: Optional[Tensor] = None,
                 cached_scale: bool = False):
        if not self.fused:
            assert residual is None or len(self.members) == 1
            return [m.forward(x, out=out[:, o : o + n], residual=residual, cached_scale=cached_scale)[1]
                    for m, o, n in zip(self.members, self.n_off, self.Ns)]
        t = b2 = None
        if self.R > 0:
            # the four operand images (forward: a_cat, b2; backward: bT, a2t) come out of one launch and ride along in `saved`
            a_cat, b2, bT, a2t = self.packed or K.lora_group_pack([m.lora_a.detach() for m in self.members],
                                                                  [m.lora_b.detach() for m in self.members], self.K, self.scale)
            t = (t_pre if t_pre is not None else K.skinny_nt(x, a_cat), bT, a2t)
        if self.dora:
            # DoRA members: the un-scaled product z is kept for d m; rescale (and residual) are their own HBM-bound passes, so RoPE /
            # SwiGLU run stand-alone after this group (rope_fusable / swiglu_fusable are False)
            assert swiglu_h is None and rope is None
            c, inv = (self.dora_scale_cached(), None) if cached_scale else dora_colscale(self.members, self.w_cat(), a_cat, b2)
            z = K.gemm_nt(x, self.w_cat(), a2=t[0], b2=b2, k2_eff=self.k2_fwd)
            K.scale(z, colscale=c, out=out)
            if residual is not None:
                K.add(out, residual, out=out)
            return (*t, z, c, inv)
        if not self.int8:
            if residual is not None:
                K.gemm_nt(x, self.w_cat(), out=out, a2=t[0] if t else None, b2=b2, epilogue=K.EPI_RESIDUAL, e=residual, k2_eff=self.k2_fwd)
            elif swiglu_h is not None:  # gate|up group: h = silu(g) * u leaves the same GEMM (g and u are stored as usual)
                K.gemm_nt(x, self.w_cat(), out=out, a2=t[0] if t else None, b2=b2, epilogue=K.EPI_SWIGLU_FWD, e=swiglu_h, k2_eff=self.k2_fwd)
            else:
                K.gemm_nt(x, self.w_cat(), out=out, a2=t[0] if t else None, b2=b2, rope=rope, k2_eff=self.k2_fwd)
            return t
        if self.dynamic:
            from subclasses.int8 import quantize_int8_rowwise
            from subclasses.int8_mm import _launch as i8_gemm

            xi, xs = xq if xq is not None else quantize_int8_rowwise(x)
            # one launch: int8 product dequantised in place, the adapter as bf16 K-extension, then residual / SwiGLU / RoPE epilogue
            a2, bb = (t[0], b2) if self.R > 0 else (None, None)
            if residual is not None:
                i8_gemm(xi, self.w_cat(), xs, self.scale_cat(), out=out, a2=a2, b2=bb, epilogue=K.EPI_RESIDUAL, e=residual)
            elif swiglu_h is not None:
                i8_gemm(xi, self.w_cat(), xs, self.scale_cat(), out=out, a2=a2, b2=bb, epilogue=K.EPI_SWIGLU_FWD, e=swiglu_h)
            else:
                i8_gemm(xi, self.w_cat(), xs, self.scale_cat(), out=out, a2=a2, b2=bb, rope=rope)
            return t
        else:
            direct = self.R == 0 and residual is None
            y0 = K.gemm_nt(x, self.w_cat(), out=out if direct else None, epilogue=K.EPI_COLSCALE, e=self.scale_cat())
        # (x @ W8^T) * scale is rounded to bf16 first (subclasses/int8.py:118); adapter and residual are added after
        if self.R > 0:
            y0 = K.gemm_nt(t[0], b2, out=out if residual is None else None, epilogue=K.EPI_RESIDUAL, e=y0, k2_eff=0)
        if residual is not None:
            K.add(y0, residual, out=out)
        return t

    # ---- backward: returns (dx, grads aligned with tensors())
    def _tn_segs(self) -> Optional[list[tuple[int, int, int, int]]]:
        """(n_lo, n_hi, r_lo, r_hi) of every adapted member for the segment form of skinny_tn; None when it does not apply."""
        if getattr(self, "_segs", None) is None:
            segs = [(no, no + n, ro, ro + r) for ro, r, no, n in zip(self.r_off, self.ranks, self.n_off, self.Ns) if r > 0]
            ok = 1 <= len(segs) <= 4 and all(a % 256 == 0 and (b % 256 == 0 or b == self.N) for a, b, _, _ in segs)
            self._segs = segs if ok else False
        return self._segs or None

    def _kranges(self) -> Optional[list[int]]:
        """k range of each 16-row block of the batched B^T (block-diagonal: member i owns rows r_off[i].. and k in
        n_off[i]..n_off[i]+N_i); None when a boundary is not a multiple of 64 (the kernel then treats B^T as dense)."""
        if getattr(self, "_kr", None) is None and len(self.members) == 1:
            self._kr = False  # a single member's B^T is dense
        if getattr(self, "_kr", None) is None:
            kr: list[int] = []
            for nb in range(4):
                lo, hi = None, None
                for ro, r, no, n in zip(self.r_off, self.ranks, self.n_off, self.Ns):
                    if r > 0 and ro < 16 * nb + 16 and ro + r > 16 * nb:
                        lo = no if lo is None else min(lo, no)
                        hi = no + n if hi is None else max(hi, no + n)
                kr += [lo or 0, hi or 0] if lo is not None else [0, 0]
            ok = all(v % 64 == 0 for v in kr)
            self._kr = kr if ok else False
        return self._kr or None

    def backward(self, dy: Tensor, x: Tensor, saved, needs: Sequence[bool], need_dx: bool, dx_out: Optional[Tensor] = None,
                 swiglu: Optional[tuple[Tensor, Tensor]] = None, pending: Optional[list] = None):
        """swiglu = (gate|up activations [M, 2K], dg|du output [M, 2K]): the data gradient of this linear is the gradient of
        silu(g)*u, and the dgrad GEMM applies the SwiGLU backward in its epilogue (returns the dg|du tensor instead of dx).
        pending (a list; a fused group needs it): the second stage of the adapter-gradient products is queued there instead of launched
        (K.skinny_tn_flush: the block's backward runs the second stages of its two groups - four products - in one launch before it
        returns the gradients)."""
        if not self.fused:
            grads, dx, first = [], None, True
            ni = 0
            for m, o, n, t in zip(self.members, self.n_off, self.Ns, saved):
                cnt = len(m.tensors())
                d, g = m.backward(dy[:, o : o + n], x, t, needs[ni : ni + cnt], need_dx, dx_out, not first)
                ni += cnt
                grads += g
                dx = d if d is not None else dx
                first = False
            return dx, grads
        gM = None
        ni = iter(needs)
        need = []
        for m in self.members:
            cnt = len(m.tensors())
            need.append([next(ni) for _ in range(cnt)])
        ia = -3 if self.dora else -2  # per-member needs end with (..., lora_a, lora_b[, m])
        dy_out = dy
        z = inv = None
        if self.dora:  # out = z * c: d m = colsum(dy * z) / norm; everything upstream sees dz = dy * c
            t, bT, a2t, z, c, inv = saved
            dy = K.scale(dy_out, colscale=c)
        else:
            t, bT, a2t = saved if saved is not None else (None, None, None)
        u = gA = gBt = g_scaled = None
        gB_views: Optional[list[Optional[Tensor]]] = None
        need_a, need_b = self.R > 0 and any(nd[ia] for nd in need), self.R > 0 and any(nd[ia + 1] for nd in need)
        # (issuing the dB chain, the dA chain or both on a side stream - parallel branches of the replayed hipGraph - was measured three
        # ways against the data-gradient GEMM and against each other: within +-0.2 ms per step of this plain order, so it stays plain)
        # dB = s t^T.dy (and DoRA's d m): nothing here needs u
        if self.dora and any(nd[-1] for nd in need):
            gM = K.colsum_mul(dy_out, z, inv)
        if need_b:
            segs = self._tn_segs()
            if segs is not None:  # each member's dB lands in its own contiguous block of one flat buffer: no slicing copies
                flat = _grad_dst([m.lora_b for m in self.members if m.rank > 0])  # the arena keeps a group's B factors back to back
                if flat is None:
                    flat = torch.empty(sum((b - a) * (d - c_) for a, b, c_, d in segs), device=dy.device, dtype=BF16)
                # dB's first stage also emits u = dy @ B from the dy tiles it stages (dy read once instead of twice) - and, for an
                # int8 base, (dy * scale), the operand of its data gradient (subclasses/int8.py:127)
                sc = None
                if self.int8 and need_dx:
                    g_scaled = torch.empty_like(dy)
                    sc = (self.scale_cat(), g_scaled)
                K.skinny_tn(t, dy, self.R, self.scale, flat, transpose_out=True, segs=segs, pending=pending, u_from=bT, scaled=sc)
                u = K.skinny_u_reduce(pending[-1])
                gB_views, off = [], 0
                for m_, (a, b, c_, d) in zip([m for m in self.members if m.rank > 0], segs):
                    gB_views.append(flat[off : off + (b - a) * (d - c_)].view(b - a, d - c_))
                    off += (b - a) * (d - c_)
            else:
                gBt = torch.empty(self.N, self.R, device=dy.device, dtype=BF16)
                K.skinny_tn(t, dy, self.R, self.scale, gBt, transpose_out=True)  # (sliced below: needs the finished product)
        if self.R > 0:  # u = dy.B (unless it came out of the dB pass above), then dA = s u^T.x
            if u is not None:
                pass
            elif self.int8 and need_dx:
                # ... and (dy * scale), the int8 base's data-gradient operand (subclasses/int8.py:127), from the same read of dy
                u, g_scaled = K.skinny_nt(dy, bT, self._kranges(), colscale=self.scale_cat())
            else:
                u = K.skinny_nt(dy, bT, self._kranges())  # [M,64]: column block i = dy_i @ B_i
            if need_a:
                gA = _grad_dst([m.lora_a for m in self.members if m.rank > 0], (self.R, self.K))  # ... and its A factors
                if gA is None:
                    gA = torch.empty(self.R, self.K, device=dy.device, dtype=BF16)
                # (dA's first stage launches on its own: batched with the NEXT group's dB + u stage it made one long launch of unequal
                # blocks - 105 us where the two take 25 + 39)
                K.skinny_tn(u, x, self.R, self.scale, gA, transpose_out=False, pending=pending)
        dx = None
        if need_dx:
            if self.int8:
                g = g_scaled if g_scaled is not None else K.scale(dy, colscale=self.scale_cat())  # (g * scale) rounded (subclasses/int8.py:127)
            else:
                g = dy
            if swiglu is not None:
                dx = K.gemm_nt(g, self.wt_cat(), out=swiglu[1], a2=u, b2=a2t if self.R > 0 else None, epilogue=K.EPI_SWIGLU_BWD, e=swiglu[0], k2_eff=self.R)
            else:
                dx = K.gemm_nt(g, self.wt_cat(), out=dx_out, a2=u, b2=a2t if self.R > 0 else None, k2_eff=self.R)
        grads: list[Optional[Tensor]] = []
        gb_i = 0
        for m, nd, ro, no, n in zip(self.members, need, self.r_off, self.n_off, self.Ns):
            j = 0
            if not m.int8 and not m.mx4:
                grads.append(K.gemm_tn(dy[:, no : no + n], x) if nd[j] else None)
                j += 1
            if m.rank > 0:
                grads.append(gA[ro : ro + m.rank] if nd[j] else None)
                if gB_views is not None:
                    grads.append(gB_views[gb_i] if nd[j + 1] else None)
                    gb_i += 1
                else:
                    grads.append(gBt[no : no + n, ro : ro + m.rank].contiguous() if nd[j + 1] else None)
                j += 2
            if m.dora_m is not None:
                grads.append(gM[no : no + n] if nd[j] else None)
        return dx, grads


def _grad_dst(params: Sequence[Optional[Tensor]], shape: Optional[tuple] = None) -> Optional[Tensor]:
    """Where backward may write the gradients of `params` directly: the slice of the trainable arena's gradient buffer
    (llx.arena.TrainableArena) that covers them back to back, or None - not in an arena, not adjacent in this order, one of them
    already has a ``.grad`` (accumulation micro-step: autograd has to ADD, so the product goes to a fresh buffer), or another autograd
    node of this backward has already been given the slot (a parameter with two consumers: the second product must not overwrite the
    first; the claim is released by the arena's settle() / zero_grad() / optimizer-step hook)."""
    g0 = first = end = None
    for p in params:
        slot = getattr(p, "_llx_slot", None)
        if slot is None or p.grad is not None or getattr(p, "_llx_claimed", False):
            return None
        G, off, n = slot
        if g0 is None:
            g0, first = G, off
        elif G is not g0 or off != end:
            return None
        end = off + n
    if g0 is None:
        return None
    for p in params:
        p._llx_claimed = True
    out = g0[first:end]
    return out.view(shape) if shape is not None else out


def _enc(o, flat: list):
    # module-level on purpose: a recursive CLOSURE over `flat` would be a reference cycle (function <-> its own cell) that keeps every
    # saved activation alive until the cyclic GC happens to run - exactly the memory activation checkpointing is there to release
    if isinstance(o, Tensor):
        flat.append(o)
        return ("t", len(flat) - 1)
    if isinstance(o, (tuple, list)):
        return ("l", [_enc(x, flat) for x in o])
    return ("c", o)


def _dec(sp, flat):
    kind, v = sp
    if kind == "t":
        return flat[v]
    if kind == "l":
        return tuple(_dec(x, flat) for x in v)
    return v


def _save(ctx, *objs) -> None:
    """Route EVERY tensor a backward needs through ``save_for_backward`` (nested tuples / lists / None allowed): saved-tensor hooks
    (non-reentrant ``checkpoint`` at modelling/llama.py, CPU offload) then see the activations and can drop / recompute them,
    and autograd's in-place version checks cover them.  Only the nesting structure stays on ``ctx``."""
    flat: list[Tensor] = []
    ctx._llx_spec = [_enc(o, flat) for o in objs]
    ctx.save_for_backward(*flat)


def _load(ctx) -> list:
    flat = ctx.saved_tensors
    return [_dec(sp, flat) for sp in ctx._llx_spec]


def prepack(plans: Sequence[GroupPlan]) -> None:
    """Build the LoRA operand images of several fused groups (the four of a transformer layer) in one launch instead of one per group."""
    todo = [p for p in plans if p.fused and p.R > 0]
    for i in range(0, len(todo), 4):
        chunk = todo[i : i + 4]
        if len(chunk) < 2:
            break
        imgs = K.lora_groups_pack([([m.lora_a.detach() for m in p.members], [m.lora_b.detach() for m in p.members], p.K, p.scale) for p in chunk])
        for p, im in zip(chunk, imgs):
            p.packed = im


def _norm_prologue(meta, plan: GroupPlan, x2: Tensor, norm_w: Optional[Tensor]):
    """xn = [rmsnorm(x2)] for the linear group that reads it -> (xn, rstd, xq, t_pre).  The norm kernel also emits what the group would
    otherwise make from xn in a pass of its own: xq = quantize_int8_rowwise(xn) for dynamically quantised int8 members, or t_pre = the
    adapters' xn @ A_cat^T."""
    if not meta.fuse_norm:
        return x2, None, None, None
    if plan.wants_quantized_input():
        xn, rstd, *xq = K.rmsnorm_fwd(x2, norm_w.detach(), meta.eps, quant=True)
        return xn, rstd, xq, None
    if plan.norm_can_make_t(x2.shape[1]):
        xn, rstd, t_pre = K.rmsnorm_skinny_nt(x2, norm_w.detach(), meta.eps, plan.packed[0])
        return xn, rstd, None, t_pre
    xn, rstd = K.rmsnorm_fwd(x2, norm_w.detach(), meta.eps)
    return xn, rstd, None, None


def _norm_epilogue(dxn: Optional[Tensor], x2: Tensor, norm_w: Optional[Tensor], rstd: Optional[Tensor], need_dnw: bool,
                   dres: Optional[Tensor] = None, fuse_norm: bool = True):
    """Backward of xn = [rmsnorm(x)] -> (dx, d norm_w): d(xn) goes through the norm's backward, which joins dres - the gradient that came
    around the residual connection - in the same pass (without a fused norm: one add).  (None, None) when nothing wanted d(xn)."""
    if dxn is None:
        return None, None
    if fuse_norm:
        return K.rmsnorm_bwd(dxn, x2, norm_w.detach(), rstd, need_dnw, dres, dw_out=_grad_dst([norm_w]))
    return (K.add(dxn, dres) if dres is not None else dxn), None


def _plans_tensors(plans: Sequence[LinearPlan]) -> tuple[list[Tensor], list[int]]:
    ts, counts = [], []
    for p in plans:
        t = p.tensors()
        ts += t
        counts.append(len(t))
    return ts, counts


# =================================================================================================
# generic single-linear function (LM head without labels, stand-alone LoRALinear / int8 F.linear)
# =================================================================================================
class LinearFn(Function):
    @staticmethod
    def forward(ctx, x: Tensor, plan: LinearPlan, *tensors):
        K.L.require_cuda(x)
        x2 = K._rows2d(x)
        y, t = plan.forward(x2, cached_scale=plan.no_grad or not any(ctx.needs_input_grad))
        ctx.plan = plan
        _save(ctx, x2, t)
        ctx.xshape = x.shape
        return y.view(*x.shape[:-1], plan.N)

    @staticmethod
    def backward(ctx, dy: Tensor):
        plan: LinearPlan = ctx.plan
        dy2 = K._rows2d(dy)
        needs = ctx.needs_input_grad[2:]
        x2, t = _load(ctx)
        dx, grads = plan.backward(dy2, x2, t, needs, need_dx=ctx.needs_input_grad[0])
        return (dx.view(ctx.xshape) if dx is not None else None, None, *grads)


def linear(x: Tensor, m: nn.Linear) -> Tensor:
    plan = LinearPlan(m)
    plan.no_grad = not torch.is_grad_enabled()  # (inside Function.forward grad mode is always off: noted here)
    return LinearFn.apply(x, plan, *plan.tensors())


# =================================================================================================
# RMSNorm
# =================================================================================================
class RMSNormFn(Function):
    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor, eps: float):
        y, rstd = K.rmsnorm_fwd(x.contiguous(), w.detach(), eps)
        ctx.save_for_backward(x, w, rstd)
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        x, w, rstd = ctx.saved_tensors
        dx, dw = K.rmsnorm_bwd(dy.contiguous(), x.contiguous(), w.detach(), rstd, ctx.needs_input_grad[1], dw_out=_grad_dst([w]))
        return dx, dw, None


def rmsnorm(x: Tensor, w: Tensor, eps: float) -> Tensor:
    return RMSNormFn.apply(x, w, eps)


# =================================================================================================
# attention residual branch:  [x +] wo( attn( rope(wq xn), rope(wk xn), wv xn ) ),  xn = [rmsnorm(x)]
# =================================================================================================
# Attention dropout state: one int64 [2] tensor (seed, counter) per device, created at the first training forward with dropout from
# torch.initial_seed() (so the ranks of a data-parallel job differ by their torch seeds, as in PyTorch) and counter 0.  A training step
# takes a TICKET - a clone of the state - and advances the counter, both as launches on the device (no host read: capturable, and a
# replayed graph draws a new mask on every replay).  The kernels of the step's forward and backward read the ticket, never the live
# state: two forwards before a backward keep their own masks, and recomputation under activation checkpointing sees the same ticket.
_ATTN_RNG: dict = {}


def _attn_rng(device) -> Tensor:
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    st = _ATTN_RNG.get(device)
    if st is None:
        st = _ATTN_RNG[device] = torch.tensor([torch.initial_seed() & (2**63 - 1), 0], dtype=torch.int64, device=device)
    return st


def seed_attn_dropout(seed: int, counter: int = 0, device=None) -> None:
    """Set the attention-dropout state (seed, counter) of ``device`` (default: the current one), in place: a captured training step
    that was recorded against the state keeps working and continues from the new values."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    _attn_rng(device).copy_(torch.tensor([int(seed) & (2**63 - 1), int(counter)], dtype=torch.int64))


def attn_dropout_ticket(device) -> Tensor:
    """The (seed, counter) a training step's attention kernels read: a clone of the device's state, whose counter then advances."""
    st = _attn_rng(device)
    ticket = st.clone()
    st[1:].add_(1)
    return ticket


class AttnBlockMeta:
    def __init__(self, qkv: GroupPlan, wo: GroupPlan, num_heads, num_kv_heads, head_dim, mask, eps, fuse_norm, fuse_residual,
                 dropout: Optional[tuple] = None):
        self.qkv, self.wo = qkv, wo
        self.H, self.KVH, self.hd = num_heads, num_kv_heads, head_dim
        self.mask, self.eps = mask, eps
        self.fuse_norm, self.fuse_residual = fuse_norm, fuse_residual
        self.dropout = dropout  # (threshold, stream_id) or None; the ticket travels as a tensor argument of AttnBlockFn
        self.no_grad = not torch.is_grad_enabled()  # the caller's grad mode (inside Function.forward it is always off)


class AttnBlockFn(Function):
    @staticmethod
    def forward(ctx, x: Tensor, rope: Tensor, norm_w: Optional[Tensor], meta: AttnBlockMeta, ticket: Optional[Tensor], *tensors):
        K.L.require_cuda(x)
        B, S, D = x.shape
        H, KVH, hd = meta.H, meta.KVH, meta.hd
        x2 = K._rows2d(x.contiguous())
        xn, rstd, xq, t_pre = _norm_prologue(meta, meta.qkv, x2, norm_w)
        W = (H + 2 * KVH) * hd
        qkv = torch.empty(B * S, W, device=x.device, dtype=BF16)
        fuse_rope = meta.qkv.rope_fusable()
        infer = meta.no_grad or not any(ctx.needs_input_grad)  # no backward follows: DoRA groups take their cached row factors
        _, tqkv = meta.qkv.forward(xn, qkv, rope=(rope, S, (H + KVH) * hd) if fuse_rope else None, xq=xq, t_pre=t_pre, cached_scale=infer)
        qkv3 = qkv.view(B, S, W)
        if not fuse_rope:
            K.rope_(qkv3, rope, H + KVH)
        q = qkv3[..., : H * hd].unflatten(-1, (H, hd))
        k = qkv3[..., H * hd : (H + KVH) * hd].unflatten(-1, (KVH, hd))
        v = qkv3[..., (H + KVH) * hd :].unflatten(-1, (KVH, hd))
        o, lse = K.attn_fwd(q, k, v, meta.mask, dropout=(meta.dropout[0], ticket, meta.dropout[1]) if meta.dropout else None)
        o2 = o.view(B * S, H * hd)
        y, to = meta.wo.forward(o2, None, x2 if meta.fuse_residual else None, cached_scale=infer)
        ctx.meta = meta
        # x2 is x itself (or its contiguous copy) and xn == x2 without the fused norm: saved once, by identity, below
        _save(ctx, x, rope, norm_w, x2, xn if meta.fuse_norm else None, rstd, qkv3, o, lse, tqkv, to, ticket if meta.dropout else None)
        return y.view(B, S, D)

    @staticmethod
    def backward(ctx, dy: Tensor):
        meta: AttnBlockMeta = ctx.meta
        x, rope, norm_w, x2, xn, rstd, qkv3, o, lse, tqkv, to, ticket = _load(ctx)
        if xn is None:
            xn = x2
        B, S, D = x.shape
        H, KVH, hd = meta.H, meta.KVH, meta.hd
        dy2 = K._rows2d(dy.contiguous())
        needs = list(ctx.needs_input_grad[5:])
        n_qkv = len(meta.qkv.tensors())
        nqkv, no = needs[:n_qkv], needs[n_qkv:]
        pend = []  # second stages of the four adapter-gradient products of this block: one launch at the end
        # wo
        do2, g_o = meta.wo.backward(dy2, o.view(B * S, H * hd), to, no, True, pending=pend)
        # attention
        W = (H + 2 * KVH) * hd
        dqkv = torch.empty(B, S, W, device=x.device, dtype=BF16)
        q = qkv3[..., : H * hd].unflatten(-1, (H, hd))
        k = qkv3[..., H * hd : (H + KVH) * hd].unflatten(-1, (KVH, hd))
        v = qkv3[..., (H + KVH) * hd :].unflatten(-1, (KVH, hd))
        dq = dqkv[..., : H * hd].unflatten(-1, (H, hd))
        dk = dqkv[..., H * hd : (H + KVH) * hd].unflatten(-1, (KVH, hd))
        dv = dqkv[..., (H + KVH) * hd :].unflatten(-1, (KVH, hd))
        # apply_rope's transpose rides in the dQ epilogue and the dK/dV reduce
        K.attn_bwd(q, k, v, o, do2.view(B, S, H, hd), lse, dq, dk, dv, meta.mask, rope=rope,
                   dropout=(meta.dropout[0], ticket, meta.dropout[1]) if meta.dropout else None)
        d2 = dqkv.view(B * S, W)
        need_dx = ctx.needs_input_grad[0]
        need_dxn = need_dx or (meta.fuse_norm and ctx.needs_input_grad[2])  # the norm weight gradient needs d(xn) too
        dxn = torch.empty(B * S, D, device=x.device, dtype=BF16) if need_dxn else None
        _, g_qkv = meta.qkv.backward(d2, xn, tqkv, nqkv, need_dxn, dxn, pending=pend)
        K.skinny_tn_flush(pend)
        dx, dnw = _norm_epilogue(dxn, x2, norm_w, rstd, ctx.needs_input_grad[2], dy2 if (need_dx and meta.fuse_residual) else None, meta.fuse_norm)
        return (dx.view(B, S, D) if (dx is not None and need_dx) else None, None, dnw, None, None, *g_qkv, *g_o)


# =================================================================================================
# MLP residual branch:  [x +] w2( silu(w1 xn) * w3 xn ),  xn = [rmsnorm(x)]
# =================================================================================================
_HEAD_COMPACT = os.environ.get("LLX_HEAD_COMPACT", "1") != "0"  # LM head + loss over the labelled rows only (HeadLossFn)
# K ranges of the head's d-hidden GEMM (1 = unsplit).  The row count is only known on the device, so the split is static: with 4 ranges
# a round of 256 tiles lasts a quarter of the unsplit tile time, i.e. the time follows the labelled-row count in steps of 1/4 round
# (3071 rows: 12 x 16 x 4 = 768 tiles = 3 full rounds; measured -0.5 ms against one long round, 2 ranges = 1.5 rounds gain nothing)
_HEAD_SPLITK = max(1, int(os.environ.get("LLX_HEAD_SPLITK", "4")))
_HEAD_CHUNK_FORCED = "LLX_HEAD_CHUNK_ROWS" in os.environ
_HEAD_CHUNK_ROWS = max(256, int(os.environ.get("LLX_HEAD_CHUNK_ROWS", "8192")) // 256 * 256)  # rows per logits buffer of the chunked head


class MLPBlockMeta:
    def __init__(self, w13: GroupPlan, w2: GroupPlan, eps, fuse_norm, fuse_residual):
        self.w13, self.w2 = w13, w2
        self.eps, self.fuse_norm, self.fuse_residual = eps, fuse_norm, fuse_residual
        self.no_grad = not torch.is_grad_enabled()  # the caller's grad mode (inside Function.forward it is always off)


class MLPBlockFn(Function):
    @staticmethod
    def forward(ctx, x: Tensor, norm_w: Optional[Tensor], meta: MLPBlockMeta, *tensors):
        K.L.require_cuda(x)
        shape = x.shape
        x2 = K._rows2d(x.contiguous())
        xn, rstd, xq, t_pre = _norm_prologue(meta, meta.w13, x2, norm_w)
        T, I = x2.shape[0], meta.w13.Ns[0]
        gu = torch.empty(T, 2 * I, device=x.device, dtype=BF16)
        infer = meta.no_grad or not any(ctx.needs_input_grad)  # no backward follows: DoRA groups take their cached row factors
        if meta.w13.swiglu_fusable():
            h = torch.empty(T, I, device=x.device, dtype=BF16)
            _, t13 = meta.w13.forward(xn, gu, swiglu_h=h, xq=xq, t_pre=t_pre, cached_scale=infer)  # SwiGLU in the epilogue of the gate|up GEMM
        else:
            _, t13 = meta.w13.forward(xn, gu, xq=xq, t_pre=t_pre, cached_scale=infer)
            h = K.swiglu_fwd(gu[:, :I], gu[:, I:])
        y, t2 = meta.w2.forward(h, None, x2 if meta.fuse_residual else None, cached_scale=infer)
        ctx.meta = meta
        _save(ctx, x, norm_w, x2, xn if meta.fuse_norm else None, rstd, gu, h, t13, t2)
        return y.view(shape)

    @staticmethod
    def backward(ctx, dy: Tensor):
        meta: MLPBlockMeta = ctx.meta
        x, norm_w, x2, xn, rstd, gu, h, t13, t2 = _load(ctx)
        if xn is None:
            xn = x2
        T, I = x2.shape[0], meta.w13.Ns[0]
        dy2 = K._rows2d(dy.contiguous())
        needs = list(ctx.needs_input_grad[3:])
        n_13 = len(meta.w13.tensors())
        n13, n2 = needs[:n_13], needs[n_13:]
        dgu = torch.empty(T, 2 * I, device=x.device, dtype=BF16)
        pend = []  # second stages of the four adapter-gradient products of this block: one launch at the end
        if meta.w2.fused:  # dh = dy.W2 (+LoRA) never reaches HBM: the dgrad GEMM's epilogue turns it into dg | du
            _, g_2 = meta.w2.backward(dy2, h, t2, n2, True, swiglu=(gu, dgu), pending=pend)
        else:
            dh, g_2 = meta.w2.backward(dy2, h, t2, n2, True)
            K.swiglu_bwd(dh, gu[:, :I], gu[:, I:], dgu[:, :I], dgu[:, I:])
        need_dx = ctx.needs_input_grad[0]
        need_dxn = need_dx or (meta.fuse_norm and ctx.needs_input_grad[1])
        dxn = torch.empty_like(x2) if need_dxn else None
        _, g_13 = meta.w13.backward(dgu, xn, t13, n13, need_dxn, dxn, pending=pend)
        K.skinny_tn_flush(pend)
        dx, dnw = _norm_epilogue(dxn, x2, norm_w, rstd, ctx.needs_input_grad[1], dy2 if (need_dx and meta.fuse_residual) else None, meta.fuse_norm)
        return (dx.view(x.shape) if (dx is not None and need_dx) else None, dnw, None, *g_13, *g_2)


# =================================================================================================
# final norm + LM head + cross-entropy (modelling/llama.py:216-218), and the per-token terms of that mean:
# -F.cross_entropy(..., reduction="none", ignore_index=-100).  HeadLossFn and HeadLogprobFn share the route, the row walk, the logits
# GEMMs and the whole backward after d logits; each keeps its row kernel, what it saves, its upstream gradient and its refusals.
# =================================================================================================
class HeadRoute(NamedTuple):
    plain_head: bool  # a plain head (no adapter, no bias, bf16), frozen: only d hidden is wanted from its backward
    # a plain trainable head (the reference's default, train_metamathqa.py:177-180) under compaction: its weight gradient
    # dW = d logits^T . norm(x) runs over the compacted rows too - the TN kernel reads the row count from device memory
    plain_trainable: bool
    compact: bool  # logits GEMM, row kernel and d-hidden GEMM over the labelled rows only
    chunk: int  # rows per logits buffer when the rows are walked in chunks, else 0


def _head_route(plan, weight_needs: bool, T: int, V: int) -> HeadRoute:
    """How T rows go through a head of V entries (no device work).  None of the three flags: plan.forward / plan.backward over all rows.
    T-chunked head: one [rows, V] logits buffer is limited by the GEMM's 32-bit tile offsets (4 GiB = 16.7 k rows of a 128 k vocabulary;
    the reference's packed [1, bs * S] batches get there at bs >= 5): beyond that the rows are walked in chunks - one logits buffer, one
    row-kernel launch set and (in backward) one d-hidden product per chunk.  Same per-row arithmetic: bit-identical to the unchunked
    path (LLX_HEAD_CHUNK_ROWS forces chunking for tests)."""
    plain = not plan.int8 and plan.rank == 0 and plan.bias is None and plan.dora_m is None
    chunk = _HEAD_CHUNK_ROWS if (_HEAD_CHUNK_FORCED or T * V * 2 >= 2**32) else 0
    return HeadRoute(plain and not weight_needs, plain and weight_needs and _HEAD_COMPACT, plain and _HEAD_COMPACT, chunk if T > chunk else 0)


def _head_rows(xn: Tensor, labels: Tensor, route: HeadRoute):
    """(rows_in, labels_in, idx, inv, cnt): the rows the head runs over and their labels.  Labelled-row compaction (default;
    LLX_HEAD_COMPACT=0 turns it off): F.cross_entropy(ignore_index=-100) gives a position whose label is -100 no loss term and a zero
    gradient row (modelling/llama.py:216-218), so a plain head runs over the labelled rows only - gathered in order on the device, the
    count read by the kernels from device memory (no host sync, capturable), d hidden scattered back with zero rows in between.  Same
    per-row arithmetic: every value is bit-identical to the uncompacted path; a batch with a masked prompt saves that share of the head."""
    if not route.compact:
        return xn, labels.reshape(-1).contiguous(), None, None, None
    idx, inv, labels_c, cnt = K.head_compact_index(labels)
    return K.gather_rows(xn, idx, cnt), labels_c, idx, inv, cnt


def _head_logits(plan: LinearPlan, rows_in: Tensor, route: HeadRoute, cnt: Optional[Tensor]):
    """The bf16 logits of the one buffer, or of each chunk [r0, r1) of the row walk: yields (r0, r1, logits, cnt_c, t, m_expect) with
    cnt_c the labelled rows inside the buffer (device int32, compacted rows only), t what plan.forward saved, m_expect the row count
    for the accounting of a traced eager step (one buffer only: the one host read of the head)."""
    T = rows_in.shape[0]
    step = route.chunk or T
    for r0 in range(0, T, step):
        r1 = min(T, r0 + step)
        if not route.compact:
            logits, t = plan.forward(rows_in[r0:r1])
            yield r0, r1, logits, None, t, None
            continue
        m_expect = None
        if route.chunk:
            cnt_c = torch.clamp(cnt - r0, min=0, max=r1 - r0).to(torch.int32)
        else:
            cnt_c = cnt
            m_expect = float(cnt.item()) if K.GEMM_TRACE is not None else None
        logits = torch.empty(r1 - r0, plan.N, device=rows_in.device, dtype=BF16)
        K.gemm_nt(rows_in[r0:r1], plan.w_image(), out=logits, m_valid=cnt_c, m_expect=m_expect)
        yield r0, r1, logits, cnt_c, None, m_expect


def _head_dhidden(route: HeadRoute, plan: LinearPlan, dlogits, cnt, inv: Optional[Tensor], scalar: Optional[Tensor], m_expect) -> Tensor:
    """d hidden = scalar * d logits . W of a plain head, at the positions of all rows.  [T, D] is ONE round of 256 tiles whatever the row
    count, with a contraction over the whole vocabulary - cut in K ranges computed side by side, so that fewer rows (12 x 16 tiles at
    3071 labelled rows) still fill the chip with full rounds of short tiles.  Every route uses the same split, so they stay
    bit-identical to each other.  Chunked rows: dlogits and cnt are tuples with one entry per chunk - a product per chunk into one
    buffer, then one scatter / scale over all rows."""
    wt = plan.wt_image()
    split = wt.shape[1] % (64 * _HEAD_SPLITK) == 0
    if route.chunk:
        dxc = torch.empty(sum(dl.shape[0] for dl in dlogits), wt.shape[0], device=wt.device, dtype=BF16)
        for i, (dl, cnt_c) in enumerate(zip(dlogits, cnt)):
            part = K.gemm_nt_splitk(dl, wt, _HEAD_SPLITK, m_valid=cnt_c) if split else K.gemm_nt(dl, wt, m_valid=cnt_c)
            dxc[i * route.chunk : i * route.chunk + dl.shape[0]].copy_(part)
    elif split:  # (scatter and scalar ride in the combine of the K ranges)
        return K.gemm_nt_splitk(dlogits, wt, _HEAD_SPLITK, m_valid=cnt, inv=inv, dev_scalar=scalar, m_expect=m_expect)
    else:
        dxc = K.gemm_nt(dlogits, wt, m_valid=cnt, m_expect=m_expect)
    if inv is not None:
        return K.scatter_rows(dxc, inv, scalar)
    return dxc if scalar is None else K.scale(dxc, dev_scalar=scalar)


def _head_backward(ctx, n_lead: int, saved, dlogits, inv, cnt, t, scalar: Optional[Tensor]):
    """Everything after d logits, for a head Function whose first n_lead inputs are (x, norm_w, <non-tensors>) and the rest
    plan.tensors(): scalar (device fp32, or None) multiplies every gradient."""
    route, plan = ctx.route, ctx.plan
    x, norm_w, x2, xn, rstd = saved
    needs = ctx.needs_input_grad[n_lead:]
    need_dxn = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
    if route.plain_head or route.plain_trainable:
        dx = dnw = gw = None
        if need_dxn:
            dx, dnw = _norm_epilogue(_head_dhidden(route, plan, dlogits, cnt, inv, scalar, ctx.m_expect), x2, norm_w, rstd, ctx.needs_input_grad[1])
        if route.plain_trainable:  # dW over the labelled rows (xn holds their gathered, normed activations)
            gw = K.gemm_tn(dlogits, xn, m_valid=cnt, m_expect=ctx.m_expect)
            gw = gw if scalar is None else K.scale(gw, dev_scalar=scalar)
        grads = [gw] + [None] * (len(needs) - 1) if needs else []
    else:
        dxn, grads = plan.backward(dlogits, xn, t, needs, need_dx=need_dxn)
        if scalar is not None:
            grads = [None if g is None else K.scale(g, dev_scalar=scalar) for g in grads]
            if dxn is not None:
                K.scale(dxn, dev_scalar=scalar, out=dxn)
        dx, dnw = _norm_epilogue(dxn, x2, norm_w, rstd, ctx.needs_input_grad[1])
    return (dx.view(x.shape) if dx is not None else None, dnw, *([None] * (n_lead - 2)), *grads)


class HeadLossFn(Function):
    """Mean cross-entropy of the labelled rows.  Its upstream gradient is one scalar that can be applied afterwards, so the row kernel
    writes d logits over the logits in the forward and the backward multiplies by the device scalar."""

    @staticmethod
    def forward(ctx, x: Tensor, norm_w: Tensor, labels: Tensor, eps: float, plan: LinearPlan, *tensors):
        K.L.require_cuda(x, labels)
        x2 = K._rows2d(x.contiguous())
        xn, rstd = K.rmsnorm_fwd(x2, norm_w.detach(), eps)
        need_grad = any(ctx.needs_input_grad)
        T, V = x2.shape[0], plan.N
        ctx.plan, ctx.eps, ctx.m_expect = plan, eps, None
        route = ctx.route = _head_route(plan, any(ctx.needs_input_grad[5:]), T, V)
        if route.chunk and not route.plain_head:
            raise LlxError(f"LM head over {T} rows x {V} vocabulary entries exceeds one logits buffer (4 GiB) and a trainable / adapted / "
                           "quantised head is not chunked: freeze the plain head or lower the number of positions per step")
        rows_in, labels_in, _, inv, cnt = _head_rows(xn, labels, route)
        if route.chunk:  # one CE launch set per chunk, the loss normalised by the global count of labelled rows
            ws = torch.empty(T + 2, device=x.device, dtype=torch.float32)
            loss = torch.empty((), device=x.device, dtype=torch.float32)
            parts = [(K.ce_chunk(lg, labels_in, ws, loss, r0, need_grad, cnt, r0 == 0, r1 == T), cnt_c)
                     for r0, r1, lg, cnt_c, _, _ in _head_logits(plan, rows_in, route, cnt)]
            _save(ctx, x, norm_w, x2, None, rstd, tuple(p[0] for p in parts), inv, tuple(p[1] for p in parts), None)
            return loss
        ((_, _, logits, _, t, m_expect),) = _head_logits(plan, rows_in, route, cnt)
        ctx.m_expect = m_expect
        loss, dlogits = K.ce_fwd_bwd(logits, labels_in, write_grad=need_grad, rows=cnt)
        _save(ctx, x, norm_w, x2, rows_in if (route.plain_trainable or not route.compact) else None, rstd, dlogits, inv, cnt, t)
        return loss

    @staticmethod
    def backward(ctx, gout: Tensor):
        x, norm_w, x2, xn, rstd, dlogits, inv, cnt, t = _load(ctx)
        g32 = gout.detach().to(torch.float32).reshape(1)
        return _head_backward(ctx, 5, (x, norm_w, x2, xn, rstd), dlogits, inv, cnt, t, g32)


class HeadLogprobFn(Function):
    """fp32 [T] log-probabilities of the labels (0 at ignored positions), with the row argmax as a second, non-differentiable output
    with want_top1.  The upstream gradient is per row, so - unlike the loss, whose one scalar can be applied after the fact - d logits
    is not written in the forward: the forward keeps the logits in the buffer where the loss keeps d logits, and the backward turns
    them into d logits in place once g is known (one bf16 rounding, the same traffic over forward + backward).  Without gradients
    nothing is saved, and a row set beyond one logits buffer is walked in chunks.  top_k > 0: two more non-differentiable outputs,
    int32 / fp32 [T, top_k], from one more launch per logits buffer (csrc/topk.hip) right after the forward kernel's."""

    @staticmethod
    def forward(ctx, x: Tensor, norm_w: Tensor, labels: Tensor, eps: float, plan: LinearPlan, want_top1: bool, top_k: int, *tensors):
        K.L.require_cuda(x, labels)
        x2 = K._rows2d(x.contiguous())
        xn, rstd = K.rmsnorm_fwd(x2, norm_w.detach(), eps)
        need_grad = any(ctx.needs_input_grad) and not getattr(plan, "no_grad", False)  # (needs_input_grad does not see the caller's no_grad)
        T, V = x2.shape[0], plan.N
        ctx.plan = plan
        route = ctx.route = _head_route(plan, any(ctx.needs_input_grad[7:]), T, V)
        if need_grad and V % 64 != 0:  # (as the loss path: its d-hidden GEMM contracts over the vocabulary; said here, not in the middle of backward)
            raise LlxError(f"token log-probabilities with gradients need a vocabulary that is a multiple of 64 (got {V}): the d-hidden GEMM "
                           "contracts over it in 64-column steps - score under torch.no_grad() or pad the vocabulary")
        if route.chunk and need_grad:
            raise LlxError(f"LM head over {T} rows x {V} vocabulary entries exceeds one logits buffer (4 GiB) and token log-probabilities "
                           "with gradients are not chunked: score under torch.no_grad() or lower the number of positions per step")
        rows_in, labels_in, idx, inv, cnt = _head_rows(xn, labels, route)
        parts = []
        for r0, r1, logits, cnt_c, t, m_expect in _head_logits(plan, rows_in, route, cnt):
            part = K.logprob_rows_fwd(logits, labels_in[r0:r1], rows=cnt_c, want_top1=want_top1)
            if top_k:  # here, while the buffer still holds the logits: the alternatives of the chunk's rows, the label's entry = its logp
                part += K.topk_logprobs_rows(logits, top_k, lse=part[1], label_logp=part[0], labels=labels_in[r0:r1], rows=cnt_c)
            parts.append(part)
        ctx.m_expect = m_expect
        logp, lse, top1 = parts[0][:3]
        top = parts[0][3:]
        if route.chunk:
            logp = torch.cat([p[0] for p in parts])
            top1 = torch.cat([p[2] for p in parts]) if want_top1 else None
            top = (torch.cat([p[3] for p in parts]), torch.cat([p[4] for p in parts])) if top_k else ()
        if need_grad:
            keep_rows = rows_in if (route.plain_trainable or not (route.plain_head or route.plain_trainable)) else None
            _save(ctx, x, norm_w, x2, keep_rows, rstd, logits, lse, labels_in, idx, inv, cnt, t)
        if inv is not None:  # compacted rows back to their positions: [T] vectors, zeros / -1 at the ignored positions
            logp, top1 = K.logprob_map_rows(inv, logp, 0.0, top1, -1)
            if top_k:
                top = K.topk_map_rows(inv, *top)
        extra = (() if top1 is None else (top1,)) + tuple(top)
        if not extra:
            return logp
        ctx.mark_non_differentiable(*extra)
        return (logp, *extra)

    @staticmethod
    def backward(ctx, g: Tensor, *_):
        if getattr(ctx, "consumed", False):
            raise LlxError("token log-probabilities: a second backward through the same forward - the saved logits were turned into "
                           "d logits in place by the first one; run the forward again")
        ctx.consumed = True
        x, norm_w, x2, xn, rstd, logits, lse, labels_in, idx, inv, cnt, t = _load(ctx)
        g32 = g.detach().to(torch.float32).reshape(-1).contiguous()
        if idx is not None:  # the upstream gradient of the j-th labelled row (rows past the count are ignored rows: any value)
            g32, _ = K.logprob_map_rows(idx, g32)
        dlogits = K.logprob_rows_bwd(logits, labels_in, lse, g32, rows=cnt)  # in place: the saved logits become d logits
        return _head_backward(ctx, 7, (x, norm_w, x2, xn, rstd), dlogits, inv, cnt, t, None)


def _check_labels(labels, shape, device, what: str) -> None:
    if not isinstance(labels, Tensor) or labels.dtype is not torch.int64:
        raise LlxError(f"{what}: labels must be an int64 tensor (got {getattr(labels, 'dtype', type(labels).__name__)})")
    if tuple(labels.shape) != tuple(shape):
        raise LlxError(f"{what}: labels {tuple(labels.shape)} must have the shape of tokens {tuple(shape)}")
    if not labels.is_cuda or labels.device != device:
        raise LlxError(f"{what}: labels live on {labels.device}, the hidden states on {device}: both must be on the same GPU")


def _check_top_k(k, what: str) -> None:
    if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= K.TOPK_MAX:
        raise LlxError(f"{what} must be an int in 0..{K.TOPK_MAX} (got {k!r})")


def head_logprobs(x: Tensor, norm: nn.Module, output: nn.Linear, labels: Tensor, return_top1: bool = False, top_k: int = 0):
    """fp32 log-probabilities [*labels.shape] of `labels` under output(norm(x)), 0 at labels == -100; with return_top1 also the int32
    argmax of every labelled position (-1 at the others); with top_k = k in 1..K.TOPK_MAX also, last, top_ids (int32) and top_logp
    (fp32) [*labels.shape, k]: the k likeliest tokens of every labelled position and their log-probabilities in the order of
    csrc/topk.hip (descending, equal logits by ascending index), -1 / 0.0 at the others, detached."""
    _check_labels(labels, x.shape[:-1], x.device, "token_logprobs")
    _check_top_k(top_k, "token_logprobs: top_k")
    plan = LinearPlan(output)
    plan.no_grad = not torch.is_grad_enabled()  # (inside Function.forward grad mode is always off: noted here)
    out = HeadLogprobFn.apply(x, norm.weight, labels, norm.eps, plan, bool(return_top1), top_k, *plan.tensors())
    if not return_top1 and not top_k:
        return out.view(labels.shape)
    res = [out[0].view(labels.shape)]
    if return_top1:
        res.append(out[1].view(labels.shape))
    if top_k:
        res += [out[-2].view(*labels.shape, top_k), out[-1].view(*labels.shape, top_k)]
    return tuple(res)
