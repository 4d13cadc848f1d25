"""Functional (non-autograd) wrappers over the C-ABI: shape/dtype checks in Python, raw pointers below.

Every function launches on torch's current HIP stream and returns torch tensors it allocated through
torch's caching allocator; the C side never allocates or synchronises (include/llx.h).
"""
from __future__ import annotations

import ctypes
import math
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import torch
from torch import Tensor

from . import _lib as L

BF16 = torch.bfloat16
EPI_NONE, EPI_RESIDUAL, EPI_BIAS, EPI_BIAS_GELU, EPI_COLSCALE = 0, 1, 2, 3, 4
EPI_SWIGLU_BWD = 6  # the product is dh; e = gate|up [M, 2N]; out = dg|du [M, 2N] (dh itself is not stored)
EPI_SWIGLU_FWD = 7  # b = [W_gate; W_up]; out = gate|up [M, N]; e = OUTPUT h [M, N/2] = silu(g) * u
SK_PAD = 64
# bench.py sets this to a list to collect (start_event, end_event, algorithmic ops, algorithmic bytes, "bf16" | "i8", kernel launches) per GEMM call
GEMM_TRACE = None
# likewise for the attention kernels: (start_event, end_event, "fwd" | "bwd", B, S, H) per call (the algorithmic FLOPs are the caller's to price:
# they depend on the mask)
ATTN_TRACE = None


def _trace_begin(trace):
    """Start of one GEMM_TRACE / ATTN_TRACE entry; None while tracing is off.  `trace` is the module global as the caller reads it at the
    call (bench.py rebinds the globals to fresh lists)."""
    if trace is None:
        return None
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    return ev


def _trace_end(trace, ev, *info):
    """End of the entry _trace_begin started: (start_event, end_event, *info) joins the trace."""
    if ev is not None:
        ev[1].record()
        trace.append((ev[0], ev[1], *info))


def _lib():
    return L.load()


def gemm_kernel_launches(M: int, N: int, epilogue: int) -> int:
    """Kernel launches behind one GEMM call: 2 when the launcher re-tiles the columns of a half-empty last round with 256 x 128 tiles
    (csrc/gemm_bf16.hip launch_gemm), else 1.  Accounting only (the GEMM trace of bench.py counts kernel launches, as rocprofv3 does)."""
    gm, gn = -(-M // 256), -(-N // 256)
    tail = (gm * gn) % 256
    split = epilogue != EPI_SWIGLU_FWD and N % 256 == 0 and gm * gn > 256 and 0 < tail <= 128 and tail % gm == 0
    return 2 if split else 1


def _rows2d(x: Tensor) -> Tensor:
    """View [..., C] as [R, C] with a single row stride (no copy when the leading dims are jointly contiguous)."""
    if x.dim() == 2:
        return x if x.stride(1) == 1 else x.contiguous()
    y = x.reshape(-1, x.shape[-1])
    return y if y.stride(1) == 1 else y.contiguous()


def _chk_bf16(*ts):
    for t in ts:
        if t is not None:
            assert t.dtype is BF16, f"llx kernels compute in bf16 (got {t.dtype})"
    L.require_cuda(*ts)


# ------------------------------------------------------------------------------------------------- rmsnorm
def rmsnorm_fwd(x: Tensor, w: Tensor, eps: float, quant: bool = False):
    """(y, rstd) - with quant=True also (q int8 [rows, dim], qscale bf16 [rows]) = quantize_int8_rowwise(y) from the same pass."""
    _chk_bf16(x, w)
    x2 = _rows2d(x)
    assert x2.stride(0) == x2.shape[1], "rmsnorm input rows must be dense"
    rows, dim = x2.shape
    assert w.shape == (dim,) and w.is_contiguous()
    y = torch.empty_like(x2)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    if quant:
        q = torch.empty(rows, dim, device=x.device, dtype=torch.int8)
        qs = torch.empty(rows, device=x.device, dtype=BF16)
        L.check(_lib().llx_rmsnorm_fwd_quant(L.ptr(x2), L.ptr(w), L.ptr(y), L.ptr(rstd), L.ptr(q), dim, L.ptr(qs), rows, dim, eps, L.stream()),
                "llx_rmsnorm_fwd_quant")
        return y.view(x.shape), rstd, q, qs
    L.check(_lib().llx_rmsnorm_fwd(L.ptr(x2), L.ptr(w), L.ptr(y), L.ptr(rstd), rows, dim, eps, L.stream()), "llx_rmsnorm_fwd")
    return y.view(x.shape), rstd


def rmsnorm_skinny_ok(dim: int) -> bool:
    return dim % 512 == 0 and dim <= 4096


def rmsnorm_skinny_nt(x: Tensor, w: Tensor, eps: float, a_cat: Tensor) -> tuple[Tensor, Tensor, Tensor]:
    """(y, rstd, t): y = rmsnorm(x), t = y @ a_cat^T [rows, 64] (zero beyond column R) from one read of x (csrc/skinny.hip)."""
    _chk_bf16(x, w, a_cat)
    x2 = _rows2d(x)
    rows, dim = x2.shape
    assert x2.stride(0) == dim and w.shape == (dim,) and w.is_contiguous() and rmsnorm_skinny_ok(dim)
    assert a_cat.dim() == 2 and a_cat.shape[1] == dim and a_cat.stride(1) == 1 and a_cat.shape[0] <= SK_PAD
    y = torch.empty_like(x2)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    t = torch.empty(rows, SK_PAD, device=x.device, dtype=BF16)
    L.check(_lib().llx_rmsnorm_skinny_nt(L.ptr(x2), L.ptr(w), L.ptr(a_cat), a_cat.stride(0), L.ptr(y), L.ptr(rstd), L.ptr(t), rows, dim,
                                         a_cat.shape[0], eps, L.stream()), "llx_rmsnorm_skinny_nt")
    return y.view(x.shape), rstd, t


def rmsnorm_bwd(dy: Tensor, x: Tensor, w: Tensor, rstd: Tensor, need_dw: bool, dres: Optional[Tensor] = None,
                dw_out: Optional[Tensor] = None) -> tuple[Tensor, Optional[Tensor]]:
    """dx (+ dres, the gradient coming around the residual connection, joined in the same pass), dw (into dw_out when given)."""
    _chk_bf16(dy, x, w, dres)
    x2, dy2 = _rows2d(x), _rows2d(dy)
    if dy2.stride(0) != dy2.shape[1]:
        dy2 = dy2.contiguous()
    rows, dim = x2.shape
    dx = torch.empty_like(x2)
    dw = ws = None
    if need_dw:
        dw = dw_out if dw_out is not None else torch.empty(dim, device=x.device, dtype=BF16)
        assert dw.shape == (dim,) and dw.is_contiguous() and dw.dtype is BF16
        ws = torch.empty(_lib().llx_rmsnorm_bwd_workspace_bytes(rows, dim), device=x.device, dtype=torch.uint8)
    if dres is not None:
        dres = _rows2d(dres)
        assert dres.shape == x2.shape and dres.stride(0) == dim
    L.check(_lib().llx_rmsnorm_bwd(L.ptr(dy2), L.ptr(x2), L.ptr(w), L.ptr(rstd), L.ptr(dx), L.ptr(dw), 0, L.ptr(ws), L.ptr(dres), rows, dim,
                                   L.stream()), "llx_rmsnorm_bwd")
    return dx.view(x.shape), dw


# ------------------------------------------------------------------------------------------------- gemm
def gemm_nt(a: Tensor, b: Tensor, *, out: Optional[Tensor] = None, a2: Optional[Tensor] = None, b2: Optional[Tensor] = None,
            epilogue: int = EPI_NONE, e: Optional[Tensor] = None, rope: Optional[tuple[Tensor, int, int]] = None,
            k2_eff: Optional[float] = None, m_valid: Optional[Tensor] = None, m_expect: Optional[float] = None) -> Tensor:
    """out[M,N] = a[M,K] @ b[N,K]^T (+ a2[M,K2] @ b2[N,K2]^T) with a fused epilogue; bf16, fp32 accumulate.
    m_valid (device int32 scalar): only the first m_valid rows are wanted - row tiles past them are skipped by the kernel (no host sync);
    m_expect: accounting only, the row count the GEMM trace should book for such a launch.
    rope = (fp32 table [>= S, 64, 2], S, cols): apply_rope on columns [0, cols) of out in the epilogue (row m = position m % S).
    k2_eff: accounting only - the K-extension's true contraction length (LoRA rank; the operands are zero padded to 64 columns and
    block diagonal for fused groups), used by the GEMM trace so that multiplying zeros is not counted as algorithmic work."""
    _chk_bf16(a, b, a2, b2, e, out)
    assert a.dim() == 2 and b.dim() == 2 and a.shape[1] == b.shape[1], (a.shape, b.shape)
    assert a.stride(1) == 1 and b.stride(1) == 1
    M, K = a.shape
    N = b.shape[0]
    if epilogue == EPI_SWIGLU_BWD:
        assert out is not None and e is not None and out.shape == (M, 2 * N) and e.shape == (M, 2 * N) and out.stride(1) == 1 and e.stride(1) == 1
    else:
        if out is None:
            out = torch.empty(M, N, device=a.device, dtype=BF16)
        assert out.shape == (M, N) and out.stride(1) == 1
    K2 = 0
    if a2 is not None:
        assert b2 is not None and a2.shape[0] == M and b2.shape[0] == N and a2.shape[1] == b2.shape[1]
        assert a2.stride(1) == 1 and b2.stride(1) == 1
        K2 = a2.shape[1]
    lde = 0
    if epilogue == EPI_RESIDUAL:
        assert e is not None and e.shape == (M, N) and e.stride(1) == 1
        lde = e.stride(0)
    elif epilogue == EPI_SWIGLU_BWD:
        lde = e.stride(0)
    elif epilogue == EPI_SWIGLU_FWD:
        assert e is not None and N % 256 == 0 and e.shape == (M, N // 2) and e.stride(1) == 1
        lde = e.stride(0)
    elif epilogue != EPI_NONE:
        assert e is not None and e.shape == (N,) and e.is_contiguous()
    ev = _trace_begin(GEMM_TRACE)
    if rope is not None:
        table, rs, rc = rope
        assert epilogue == EPI_NONE and table.dtype is torch.float32 and table.is_contiguous() and table.shape[0] >= rs and table.shape[1:] == (64, 2)
        L.check(_lib().llx_gemm_nt_bf16_rope(L.ptr(a), a.stride(0), L.ptr(b), b.stride(0), L.ptr(out), out.stride(0), M, N, K,
                                             L.ptr(a2), a2.stride(0) if a2 is not None else 0, L.ptr(b2), b2.stride(0) if b2 is not None else 0, K2,
                                             L.ptr(table), rs, rc, L.stream()), "llx_gemm_nt_bf16_rope")
    elif m_valid is not None:
        assert m_valid.dtype is torch.int32 and m_valid.numel() == 1 and m_valid.device == a.device
        L.check(_lib().llx_gemm_nt_bf16_rows(L.ptr(a), a.stride(0), L.ptr(b), b.stride(0), L.ptr(out), out.stride(0), M, N, K,
                                             L.ptr(a2), a2.stride(0) if a2 is not None else 0, L.ptr(b2), b2.stride(0) if b2 is not None else 0, K2,
                                             epilogue, L.ptr(e), lde, L.ptr(m_valid), L.stream()), "llx_gemm_nt_bf16_rows")
    else:
        L.check(_lib().llx_gemm_nt_bf16(L.ptr(a), a.stride(0), L.ptr(b), b.stride(0), L.ptr(out), out.stride(0), M, N, K,
                                        L.ptr(a2), a2.stride(0) if a2 is not None else 0, L.ptr(b2), b2.stride(0) if b2 is not None else 0, K2,
                                        epilogue, L.ptr(e), lde, L.stream()), "llx_gemm_nt_bf16")
    if ev is not None:
        kk = K + (K2 if k2_eff is None else min(float(k2_eff), K2))
        Mw = M if m_expect is None else float(m_expect)  # rows actually wanted (row-limited launches: the labelled rows)
        _trace_end(GEMM_TRACE, ev, 2.0 * Mw * N * kk, 2.0 * (Mw * kk + N * kk + Mw * N * (2 if epilogue == EPI_RESIDUAL else 1)), "bf16",
                   gemm_kernel_launches(M, N, 8 if rope is not None else epilogue))
    return out


def gemm_nt_splitk(a: Tensor, b: Tensor, splits: int, *, m_valid: Optional[Tensor] = None, inv: Optional[Tensor] = None,
                   dev_scalar: Optional[Tensor] = None, m_expect: Optional[float] = None) -> Tensor:
    """bf16(dev_scalar * bf16(a[M,K] @ b[N,K]^T)) with the contraction cut in `splits` ranges computed side by side (one launch, fp32
    partial products, summed by a second small kernel) - for products with few output tiles and a long K.  m_valid: only the first
    m_valid rows of a exist (device int32); inv: out row i = product row inv[i], zero where inv[i] < 0 (the scatter of compacted rows)."""
    _chk_bf16(a, b)
    assert a.dim() == 2 and b.dim() == 2 and a.shape[1] == b.shape[1] and a.stride(1) == 1 and b.stride(1) == 1
    M, K = a.shape
    N = b.shape[0]
    part = torch.empty(splits, M, N, device=a.device, dtype=torch.float32)
    ev = _trace_begin(GEMM_TRACE)
    L.check(_lib().llx_gemm_nt_bf16_splitk(L.ptr(a), a.stride(0), L.ptr(b), b.stride(0), L.ptr(part), M, N, K, splits, L.ptr(m_valid), L.stream()),
            "llx_gemm_nt_bf16_splitk")
    if ev is not None:
        Mw = M if m_expect is None else float(m_expect)
        _trace_end(GEMM_TRACE, ev, 2.0 * Mw * N * K, 2.0 * (Mw * K + N * K) + 4.0 * splits * Mw * N, "bf16", 1)
    out = torch.empty(M, N, device=a.device, dtype=BF16)
    assert inv is None or (inv.dtype is torch.int32 and inv.numel() == M)
    assert dev_scalar is None or (dev_scalar.dtype is torch.float32 and dev_scalar.numel() == 1)
    L.check(_lib().llx_splitk_combine(L.ptr(part), splits, M, N, L.ptr(inv), L.ptr(dev_scalar), L.ptr(out), N, L.stream()), "llx_splitk_combine")
    return out


def transpose(x: Tensor, pad_to: int = 1) -> Tensor:
    """[R,C] -> [C,Rp] bf16 copy (Rp = R rounded up to ``pad_to``, zero filled); int8 sources are widened to bf16."""
    L.require_cuda(x)
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype in (BF16, torch.int8)
    R, C = x.shape
    Rp = (R + pad_to - 1) // pad_to * pad_to
    out = (torch.zeros if Rp != R else torch.empty)(C, Rp, device=x.device, dtype=BF16)
    L.check(_lib().llx_transpose(L.ptr(x), x.stride(0), L.ptr(out), Rp, R, C, int(x.dtype is torch.int8), L.stream()), "llx_transpose")
    return out


def pad64(x: Tensor, scale_: float = 1.0, transposed: bool = False) -> Tensor:
    """[R,C<=64] -> [R,64] (or, transposed, [C<=64,R] -> [R,64]) bf16(scale*x), zero padded."""
    _chk_bf16(x)
    assert x.dim() == 2 and x.stride(1) == 1
    R, C = (x.shape[1], x.shape[0]) if transposed else x.shape
    out = torch.empty(R, SK_PAD, device=x.device, dtype=BF16)
    L.check(_lib().llx_pad64(L.ptr(x), x.stride(0), L.ptr(out), R, C, scale_, int(transposed), L.stream()), "llx_pad64")
    return out


def lora_pack(x: Tensor, out: Tensor, row_off: int, col_off: int, scale_: float = 1.0, transposed: bool = False) -> None:
    """Scatter scale*x (or its transpose) into ``out`` at (row_off, col_off); ``out`` is a pre-zeroed operand image."""
    _chk_bf16(x, out)
    assert x.dim() == 2 and x.stride(1) == 1 and out.dim() == 2 and out.stride(1) == 1
    R, C = x.shape
    rr, cc = (C, R) if transposed else (R, C)
    assert row_off + rr <= out.shape[0] and col_off + cc <= out.shape[1], (x.shape, out.shape, row_off, col_off, transposed)
    L.check(_lib().llx_lora_pack(L.ptr(x), x.stride(0), L.ptr(out), out.stride(0), R, C, row_off, col_off, scale_, int(transposed), L.stream()),
            "llx_lora_pack")


def lora_group_pack(lora_as: list, lora_bs: list, K_in: int, scale_: float):
    """(a_cat [R,K], b2 [N,64], bT [R,N], a2t [K,64]) for the members' LoRA factors, built by one launch."""
    nm = len(lora_as)
    Ns = [b.shape[0] for b in lora_bs]
    ranks = [a.shape[0] for a in lora_as]
    for a, b in zip(lora_as, lora_bs):
        _chk_bf16(a, b)
        assert a.is_contiguous() and b.is_contiguous() and a.shape[1] == K_in and b.shape[1] == a.shape[0]
    N, R = sum(Ns), sum(ranks)
    dev = lora_as[0].device
    buf = torch.empty(R * K_in + N * SK_PAD + R * N + K_in * SK_PAD, device=dev, dtype=BF16)
    a_cat = buf[: R * K_in].view(R, K_in)
    o = R * K_in
    b2 = buf[o : o + N * SK_PAD].view(N, SK_PAD)
    o += N * SK_PAD
    bT = buf[o : o + R * N].view(R, N)
    o += R * N
    a2t = buf[o:].view(K_in, SK_PAD)
    PA = (ctypes.c_void_p * nm)(*[a.data_ptr() for a in lora_as])
    PB = (ctypes.c_void_p * nm)(*[b.data_ptr() for b in lora_bs])
    NS = (ctypes.c_int64 * nm)(*Ns)
    RS = (ctypes.c_int64 * nm)(*ranks)
    L.check(_lib().llx_lora_group_pack(PA, PB, NS, RS, nm, K_in, scale_, L.ptr(a_cat), L.ptr(b2), L.ptr(bT), L.ptr(a2t), L.stream()),
            "llx_lora_group_pack")
    return a_cat, b2, bT, a2t


def lora_groups_pack(groups: list) -> list:
    """[(lora_as, lora_bs, K_in, scale), ...] (<= 4 linear groups, e.g. the four of one transformer layer) -> [(a_cat, b2, bT, a2t), ...]
    as lora_group_pack builds them, from ONE launch and one buffer."""
    ng = len(groups)
    assert 1 <= ng <= 4
    sizes, metas = [], []
    for las, lbs, K_in, _ in groups:
        for a, b in zip(las, lbs):
            _chk_bf16(a, b)
            assert a.is_contiguous() and b.is_contiguous() and a.shape[1] == K_in and b.shape[1] == a.shape[0]
        N, R = sum(b.shape[0] for b in lbs), sum(a.shape[0] for a in las)
        metas.append((N, R, K_in))
        sizes.append(R * K_in + N * SK_PAD + R * N + K_in * SK_PAD)
    dev = groups[0][0][0].device
    buf = torch.empty(sum(sizes), device=dev, dtype=BF16)
    out, o = [], 0
    for (N, R, K_in) in metas:
        a_cat = buf[o : o + R * K_in].view(R, K_in); o += R * K_in
        b2 = buf[o : o + N * SK_PAD].view(N, SK_PAD); o += N * SK_PAD
        bT = buf[o : o + R * N].view(R, N); o += R * N
        a2t = buf[o : o + K_in * SK_PAD].view(K_in, SK_PAD); o += K_in * SK_PAD
        out.append((a_cat, b2, bT, a2t))
    PA, PB = (ctypes.c_void_p * (4 * ng))(), (ctypes.c_void_p * (4 * ng))()
    NS, RS = (ctypes.c_int64 * (4 * ng))(), (ctypes.c_int64 * (4 * ng))()
    NM, KS, SC = (ctypes.c_int * ng)(), (ctypes.c_int64 * ng)(), (ctypes.c_float * ng)()
    OA, OB, OT, O2 = ((ctypes.c_void_p * ng)() for _ in range(4))
    for j, ((las, lbs, K_in, sc), imgs) in enumerate(zip(groups, out)):
        NM[j], KS[j], SC[j] = len(las), K_in, sc
        for i, (a, b) in enumerate(zip(las, lbs)):
            PA[4 * j + i], PB[4 * j + i], NS[4 * j + i], RS[4 * j + i] = a.data_ptr(), b.data_ptr(), b.shape[0], a.shape[0]
        OA[j], OB[j], OT[j], O2[j] = (t.data_ptr() for t in imgs)
    L.check(_lib().llx_lora_groups_pack(PA, PB, NS, RS, NM, KS, SC, OA, OB, OT, O2, ng, L.stream()), "llx_lora_groups_pack")
    return out


def gemm_tn(a: Tensor, b: Tensor, m_valid: Optional[Tensor] = None, m_expect: Optional[float] = None) -> Tensor:
    """a[M,N1]^T @ b[M,N2] -> [N1,N2] (weight gradients of dense linears / convolutions): the TN MFMA kernel reads both operands as they
    lie (token-major rows, row-strided views allowed).  Shapes it does not take (a dimension below 8 or not a multiple of 8, unaligned
    views) go through transposed, zero-padded copies and the NT kernel.  m_valid (device int32 scalar): only the first min(M, m_valid)
    rows enter the product (the compacted labelled rows of the LM head); m_expect is its value for the FLOP accounting of a traced step."""
    _chk_bf16(a, b)
    assert a.dim() == 2 and b.dim() == 2 and a.shape[0] == b.shape[0] and a.stride(1) == 1 and b.stride(1) == 1
    M, N1 = a.shape
    N2 = b.shape[1]
    ok = (N1 % 8 == 0 and N2 % 8 == 0 and N1 >= 8 and N2 >= 8 and a.stride(0) % 8 == 0 and b.stride(0) % 8 == 0
          and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0)
    if not ok:
        if m_valid is not None:
            raise L.LlxError("gemm_tn: a device-side row count needs the TN kernel's shapes (dimensions multiples of 8, 16-byte aligned rows)")
        return gemm_nt(transpose(a, 64), transpose(b, 64))
    out = torch.empty(N1, N2, device=a.device, dtype=BF16)
    ev = _trace_begin(GEMM_TRACE)
    if m_valid is not None:
        assert m_valid.dtype is torch.int32 and m_valid.is_cuda and m_valid.numel() == 1
    L.check(_lib().llx_gemm_tn_bf16_rows(L.ptr(a), a.stride(0), L.ptr(b), b.stride(0), L.ptr(out), out.stride(0), M, N1, N2,
                                         L.ptr(m_valid) if m_valid is not None else None, L.stream()), "llx_gemm_tn_bf16")
    if ev is not None:
        Me = M if m_expect is None else m_expect
        _trace_end(GEMM_TRACE, ev, 2.0 * Me * N1 * N2, 2.0 * (Me * N1 + Me * N2 + N1 * N2), "bf16_tn", 1)
    return out


def i8_to_bf16(x: Tensor) -> Tensor:
    L.require_cuda(x)
    assert x.dtype is torch.int8 and x.is_contiguous()
    out = torch.empty(x.shape, device=x.device, dtype=BF16)
    L.check(_lib().llx_i8_to_bf16(L.ptr(x), L.ptr(out), x.numel(), L.stream()), "llx_i8_to_bf16")
    return out


def scale(x: Tensor, *, dev_scalar: Optional[Tensor] = None, host_scale: float = 1.0, colscale: Optional[Tensor] = None,
          out: Optional[Tensor] = None) -> Tensor:
    _chk_bf16(x, colscale, out)
    x2 = _rows2d(x)
    rows, cols = x2.shape
    if out is None:
        out = torch.empty(rows, cols, device=x.device, dtype=BF16)
    o2 = _rows2d(out)
    if dev_scalar is not None:
        assert dev_scalar.dtype is torch.float32 and dev_scalar.numel() == 1
    L.check(_lib().llx_scale(L.ptr(x2), x2.stride(0), L.ptr(o2), o2.stride(0), L.ptr(dev_scalar), host_scale, L.ptr(colscale), rows, cols,
                             L.stream()), "llx_scale")
    return out.view(x.shape) if (out.is_contiguous() and out.numel() == x.numel()) else out


def add(x: Tensor, y: Tensor, out: Optional[Tensor] = None) -> Tensor:
    _chk_bf16(x, y, out)
    assert x.shape == y.shape
    x, y = x.contiguous(), y.contiguous()
    z = out if (out is not None and out.is_contiguous()) else torch.empty_like(x)
    L.check(_lib().llx_add(L.ptr(x), L.ptr(y), L.ptr(z), x.numel(), L.stream()), "llx_add")
    if out is not None and z is not out:
        scale(z, out=out)  # strided destination: one more pass through the strided copy kernel
        return out
    return z


_ONES: dict = {}


def colsum(dy: Tensor) -> Tensor:
    """Column sums of [M,N] -> [N] (bias gradients), as a rank-1 skinny_tn against a column of ones."""
    M, N = dy.shape
    key = (M, str(dy.device))
    ones = _ONES.get(key)
    if ones is None:
        ones = torch.zeros(M, SK_PAD, device=dy.device, dtype=BF16)
        ones[:, 0] = 1
        _ONES.clear()
        _ONES[key] = ones
    out = torch.empty(1, N, device=dy.device, dtype=BF16)
    skinny_tn(ones, dy, 1, 1.0, out, transpose_out=False)
    return out.view(N)


# ------------------------------------------------------------------------------------------------- DoRA
def rownorm2(w: Tensor) -> Tensor:
    """fp32 [N]: squared L2 norm of every row of the bf16 matrix w [N, K]."""
    _chk_bf16(w)
    assert w.dim() == 2 and w.stride(1) == 1
    out = torch.empty(w.shape[0], device=w.device, dtype=torch.float32)
    L.check(_lib().llx_rownorm2(L.ptr(w), w.stride(0), L.ptr(out), w.shape[0], w.shape[1], L.stream()), "llx_rownorm2")
    return out


def dora_colscale(wn2: Tensor, G: Tensor, b2: Tensor, AAt: Tensor, m: Tensor, c: Tensor, inv_norm: Tensor, R: int) -> None:
    """c[n] = m[n] / ||W_n + s B_n A|| (bf16), inv_norm[n] = 1 / norm (fp32) for the N rows these views cover (DoRA, lora.py:55-59)."""
    _chk_bf16(G, b2, AAt, m, c)
    N = m.shape[0]
    assert wn2.dtype is torch.float32 and inv_norm.dtype is torch.float32 and wn2.shape == (N,) and inv_norm.shape == (N,) and c.shape == (N,)
    assert G.shape == (N, SK_PAD) and b2.shape == (N, SK_PAD) and AAt.shape[1] == SK_PAD and AAt.shape[0] >= R
    for t in (wn2, G, b2, AAt, m, c, inv_norm):
        assert t.is_contiguous()
    L.check(_lib().llx_dora_colscale(L.ptr(wn2), L.ptr(G), L.ptr(b2), L.ptr(AAt), L.ptr(m), L.ptr(c), L.ptr(inv_norm), N, R, L.stream()),
            "llx_dora_colscale")


def colsum_mul(a: Tensor, b: Tensor, colscale: Optional[Tensor] = None) -> Tensor:
    """bf16 [N]: colscale[n] * sum_m a[m, n] * b[m, n] (fp32 accumulate, deterministic)."""
    _chk_bf16(a, b)
    assert a.shape == b.shape and a.dim() == 2 and a.stride(1) == 1 and b.stride(1) == 1
    M, N = a.shape
    if colscale is not None:
        assert colscale.dtype is torch.float32 and colscale.shape == (N,) and colscale.is_contiguous()
    out = torch.empty(N, device=a.device, dtype=BF16)
    ws = torch.empty(_lib().llx_colsum_mul_workspace_bytes(N), device=a.device, dtype=torch.uint8)
    L.check(_lib().llx_colsum_mul(L.ptr(a), a.stride(0), L.ptr(b), b.stride(0), L.ptr(colscale), L.ptr(out), L.ptr(ws), M, N, L.stream()),
            "llx_colsum_mul")
    return out


def colscale_bias(x: Tensor, colscale: Tensor, bias: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """bf16(bf16(x * colscale[n]) + bias[n]) on [M, N] rows (the two roundings of DoRALinear's rescale and bias add)."""
    _chk_bf16(x, colscale, bias, out)
    assert x.dim() == 2 and x.stride(1) == 1 and colscale.shape == (x.shape[1],) and colscale.is_contiguous()
    if bias is not None:
        assert bias.shape == (x.shape[1],) and bias.is_contiguous()
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=BF16)
    assert out.shape == x.shape and out.stride(1) == 1
    L.check(_lib().llx_colscale_bias(L.ptr(x), x.stride(0), L.ptr(out), out.stride(0), L.ptr(colscale), L.ptr(bias), x.shape[0], x.shape[1],
                                     L.stream()), "llx_colscale_bias")
    return out


# ------------------------------------------------------------------------------------------------- embedding
def embedding_fwd(ids: Tensor, table: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """out[b, s, :] = table[ids[b, s], :]; ``out`` may be a strided [B, S, D] view (e.g. behind an audio prefix)."""
    _chk_bf16(table)
    L.require_cuda(ids)
    assert ids.dtype is torch.int64 and ids.dim() == 2
    ids = ids.contiguous()
    B, S = ids.shape
    V, D = table.shape
    assert table.is_contiguous()
    if out is None:
        out = torch.empty(B, S, D, device=table.device, dtype=BF16)
    assert out.shape == (B, S, D) and out.stride(2) == 1
    L.check(_lib().llx_embedding_fwd(L.ptr(ids), L.ptr(table), L.ptr(out), B * S, D, V, S, out.stride(0), out.stride(1), L.stream()),
            "llx_embedding_fwd")
    return out


def embedding_bwd(ids: Tensor, dy: Tensor, vocab: int) -> Tensor:
    """fp32 [V, D] gradient of the table."""
    _chk_bf16(dy)
    ids = ids.contiguous()
    B, S = ids.shape
    D = dy.shape[-1]
    assert dy.shape == (B, S, D) and dy.stride(2) == 1
    dt = torch.zeros(vocab, D, device=dy.device, dtype=torch.float32)
    L.check(_lib().llx_embedding_bwd(L.ptr(ids), L.ptr(dy), L.ptr(dt), B * S, D, vocab, S, dy.stride(0), dy.stride(1), L.stream()),
            "llx_embedding_bwd")
    return dt


# ------------------------------------------------------------------------------------------------- rope
def rope_(x: Tensor, table: Tensor, nheads: int, backward: bool = False) -> Tensor:
    """In-place interleaved-pair rotation of the first ``nheads`` 128-wide heads of every row of x [B, S, *]."""
    _chk_bf16(x)
    assert x.dim() == 3 and x.stride(2) == 1 and x.shape[2] >= nheads * 128
    assert table.dtype is torch.float32 and table.is_contiguous() and table.shape[0] >= x.shape[1] and table.shape[1:] == (64, 2)
    B, S, _ = x.shape
    L.check(_lib().llx_rope(L.ptr(x), x.stride(0), x.stride(1), L.ptr(x), x.stride(0), x.stride(1), L.ptr(table), B, S, nheads, 128,
                            int(backward), L.stream()), "llx_rope")
    return x


# ------------------------------------------------------------------------------------------------- swiglu
def swiglu_fwd(g: Tensor, u: Tensor) -> Tensor:
    _chk_bf16(g, u)
    assert g.shape == u.shape and g.dim() == 2 and g.stride(1) == 1 and u.stride(1) == 1
    rows, cols = g.shape
    h = torch.empty(rows, cols, device=g.device, dtype=BF16)
    L.check(_lib().llx_swiglu_fwd(L.ptr(g), g.stride(0), L.ptr(u), u.stride(0), L.ptr(h), cols, rows, cols, L.stream()), "llx_swiglu_fwd")
    return h


def swiglu_bwd(dh: Tensor, g: Tensor, u: Tensor, dg: Tensor, du: Tensor) -> None:
    _chk_bf16(dh, g, u, dg, du)
    rows, cols = g.shape
    for t in (dh, g, u, dg, du):
        assert t.shape == (rows, cols) and t.stride(1) == 1
    L.check(_lib().llx_swiglu_bwd(L.ptr(dh), dh.stride(0), L.ptr(g), g.stride(0), L.ptr(u), u.stride(0), L.ptr(dg), dg.stride(0), L.ptr(du),
                                  du.stride(0), rows, cols, L.stream()), "llx_swiglu_bwd")


# ------------------------------------------------------------------------------------------------- attention
class MaskSpec:
    """Mask of a training step (replaces FlexAttention's BlockMask in the ``block_mask=`` slot).  Either the rule

    allow(q, k) = (k <= q or k < prefix_len[b]) and (doc_ids is None or doc_ids[b, q] == doc_ids[b, k])

    from per-token metadata - ``doc_ids`` int32 [B, S] (or [S], broadcast), ``prefix_len`` int32 [B] - or ``dense``: ANY bool mask
    [S, S], [B | 1, S, S] or [B | 1, 1, S, S] (True = attend; broadcast over heads), which nothing but its bytes describes: sliding
    windows, non-contiguous documents, left padding, block-sparse or bidirectional patterns.  ``dense`` excludes the other two.  Both
    forms train (attn_fwd / attn_bwd); the rule form is the faster one where it applies (MaskSpec.from_mask_mod picks it).  A query row
    without any allowed key gives NaN, as SDPA does.  Tile classes are built once on device, at the first use with a given (B, S,
    device): a ``dense`` mask must not be changed in place or replaced on the spec after that (a tile cached as fully masked or fully
    allowed is never tested byte by byte again) - build a new MaskSpec for a new mask.
    """

    def __init__(self, doc_ids: Optional[Tensor] = None, prefix_len: Optional[Tensor] = None, dense: Optional[Tensor] = None):
        if dense is not None:
            if doc_ids is not None or prefix_len is not None:
                raise L.LlxError("MaskSpec: dense= is the whole mask; it cannot be combined with doc_ids / prefix_len")
            if not isinstance(dense, Tensor) or dense.dtype is not torch.bool:
                raise L.LlxError(f"MaskSpec: dense must be a bool tensor (True = attend), got {getattr(dense, 'dtype', type(dense))}")
            if dense.dim() not in (2, 3, 4) or dense.shape[-1] != dense.shape[-2]:
                raise L.LlxError(f"MaskSpec: dense must be [S, S], [B | 1, S, S] or [B | 1, 1, S, S], got {tuple(dense.shape)}")
            if dense.dim() == 4 and dense.shape[1] != 1:
                raise L.LlxError(f"MaskSpec: a per-head dense mask (shape {tuple(dense.shape)}) is not supported: the mask is broadcast over heads")
        self.doc_ids = doc_ids
        self.prefix_len = prefix_len
        self.dense = dense
        self._flags = None
        self._key = None

    @staticmethod
    def from_mask_mod(mask_mod, B: int, S: int, device) -> "MaskSpec":
        """The MaskSpec of a FlexAttention-style ``mask_mod(b, h, q_idx, kv_idx) -> bool`` (the argument of the reference's
        create_block_mask, train_metamathqa.py:67-70), evaluated with h = 0 on [B, S, S] index grids.  Where the rule reproduces the
        mask exactly (causal, contiguous documents, prefix-LM) the rule spec is returned - the faster kernels - else MaskSpec(dense=...).
        One host synchronisation (that comparison), here at construction and never inside a forward."""
        b = torch.arange(B, device=device).view(B, 1, 1)
        q = torch.arange(S, device=device).view(1, S, 1)
        k = torch.arange(S, device=device).view(1, 1, S)
        m = torch.as_tensor(mask_mod(b, torch.zeros((), dtype=torch.int64, device=device), q, k), device=device)
        if m.dtype is not torch.bool:
            raise L.LlxError(f"MaskSpec.from_mask_mod: mask_mod must return bool, got {m.dtype}")
        m = m.expand(B, S, S).contiguous()[:, None]  # [B, 1, S, S]
        spec = maskspec_from_dense(m, B, S)
        return spec if spec is not None else MaskSpec(dense=m)

    def prepared(self, B: int, S: int, device) -> "MaskSpec":
        key = (B, S, str(device))
        if self._key == key:
            return self
        if self.dense is not None:
            norm = _mask_norm(self.dense.to(device), B, S, S)
            if norm is None:
                raise L.LlxError(f"MaskSpec: dense mask of shape {tuple(self.dense.shape)} does not fit batch {B}, sequence {S}")
            if S < 4:
                raise L.LlxError("MaskSpec: a dense mask needs S >= 4 (the kernels read it 4 bytes at a time)")
            self._rows = norm[0]  # [B | 1, 1, S, S], last dim dense: the tensor attn_mask_fwd / attn_mask_bwd are called with
            self._flags = _mask_flags(self._rows, B)  # (the cache those two look into)
            self._key = key
            return self
        d = self.doc_ids
        if d is not None:
            d = d.to(device=device, dtype=torch.int32)
            if d.dim() == 1:
                d = d.view(1, -1)
            assert d.shape[1] == S
            d = d.expand(B, S).contiguous()
        p = self.prefix_len
        if p is not None:
            p = torch.as_tensor(p, device=device).to(torch.int32).reshape(-1)
            if p.numel() == 1:
                p = p.expand(B)
            assert p.numel() == B
            p = p.contiguous()
        self.doc_ids, self.prefix_len = d, p
        self._flags = None
        if d is not None or p is not None:
            fl = torch.empty(_lib().llx_attn_flags_bytes(B, S), device=device, dtype=torch.uint8)
            L.check(_lib().llx_attn_tile_flags(L.ptr(d), L.ptr(p), L.ptr(fl), B, S, L.stream()), "llx_attn_tile_flags")
            self._flags = fl
        self._key = key
        return self


def maskspec_from_dense(mask: Tensor, B: int, S: int) -> Optional[MaskSpec]:
    """The MaskSpec whose rule  allow(q, k) = (k <= q or k < prefix_len[b]) and doc_ids[b, q] == doc_ids[b, k]  reproduces a dense
    bool mask (the reference's small-shape route ``layer(x, rope, mask=...)``, modelling/llama.py:135-137,163-172) EXACTLY, or None.
    Recognised: causal, prefix-LM (per-sample prefix), contiguous documents, and their combination.  Documents are read off the
    sub-diagonal (q-1 and q share a document iff mask[q, q-1]), the prefix off the part above the diagonal (its last visible column);
    the rule is then evaluated densely and compared bit for bit - any other mask (per-head masks, non-contiguous document ids,
    arbitrary patterns) gives None.  One host synchronisation (the comparison) per distinct mask tensor; cached on the tensor."""
    norm = _mask_norm(mask, B, S, S) if mask.dtype is torch.bool else None
    if norm is None:
        return None
    m = norm[0][:, 0].expand(B, S, S)
    idx = torch.arange(S, device=m.device)
    upper = m & (idx[None, :, None] < idx[None, None, :])            # allowed pairs with k > q: only the prefix term can make them
    seen = upper.any(dim=1)                                           # [B, S]: column k visible from some earlier row
    prefix = torch.where(seen.any(dim=1), S - seen.flip(1).float().argmax(dim=1), torch.zeros(B, device=m.device, dtype=torch.int64)).to(torch.int64)
    link = torch.diagonal(m, offset=-1, dim1=1, dim2=2)               # [B, S-1]: mask[q, q-1]
    doc = torch.cat([torch.zeros(B, 1, dtype=torch.int64, device=m.device), (~link).to(torch.int64).cumsum(1)], dim=1)
    rule = ((idx[None, None, :] <= idx[None, :, None]) | (idx[None, None, :] < prefix[:, None, None])) & (doc[:, :, None] == doc[:, None, :])
    if not bool(torch.equal(rule, m)):
        return None
    has_doc, has_prefix = bool(doc.any()), bool(prefix.any())
    if not has_doc and not has_prefix:
        return MaskSpec()  # plain causal
    return MaskSpec(doc.to(torch.int32) if has_doc else None, prefix.to(torch.int32) if has_prefix else None)


def attn_dropout_threshold(p: float) -> int:
    """t = round(p * 65536) for 0 < p < 1: the kernels drop an element with probability t / 65536 and scale a kept one by
    65536 / (65536 - t) (csrc/attn_dropout.h), so the realised probability and the scale match exactly."""
    if not (isinstance(p, (int, float)) and 0.0 < p < 1.0):
        raise L.LlxError(f"attn_dropout={p!r} must lie in [0, 1)")  # (0 itself never gets here: it takes the kernels without dropout)
    return min(65535, max(1, int(round(p * 65536))))


def _dropout_operands(dropout, device, fn: str):
    """(threshold, rng pointer, stream_id) of a ``dropout=(threshold, rng, stream_id)`` argument: rng is the int64 [2] device tensor
    (seed, counter) the kernels read - the ticket of the step, the same tensor in forward and backward."""
    t, rng, sid = dropout
    if not (isinstance(rng, Tensor) and rng.dtype is torch.int64 and rng.numel() == 2 and rng.is_contiguous() and rng.device == device):
        raise L.LlxError(f"{fn}: attn_dropout needs rng = a contiguous int64 [2] tensor (seed, counter) on {device}")
    return int(t), L.ptr(rng), int(sid)


def attn_dropout_keep(B: int, H: int, Sq: int, Skv: int, dropout) -> Tensor:
    """The keep bytes [B, H, Sq, Skv] (1 = kept, 0 = dropped) that attn_fwd / attn_bwd apply under the same
    ``dropout=(threshold, rng, stream_id)``: written by the device function the attention kernels call."""
    t, rng, sid = dropout
    keep = torch.empty(B, H, Sq, Skv, device=rng.device, dtype=torch.uint8)
    t, rp, sid = _dropout_operands(dropout, keep.device, "attn_dropout_keep")
    L.check(_lib().llx_attn_dropout_keep(L.ptr(keep), B, H, Sq, Skv, t, rp, sid, L.stream()), "llx_attn_dropout_keep")
    return keep


def attn_fwd(q: Tensor, k: Tensor, v: Tensor, mask: Optional[MaskSpec] = None, dropout=None) -> tuple[Tensor, Tensor]:
    """q [B,S,H,128], k/v [B,S,KVH,128] (last two dims dense; batch/seq strides free) -> o [B,S,H,128], lse [B,H,S].
    dropout = (threshold, rng, stream_id) or None: attention dropout as SDPA's dropout_p in training (attn_dropout_threshold,
    an int64 [2] device tensor (seed, counter), one id per attention module); lse stays that of the undropped rows."""
    _chk_bf16(q, k, v)
    B, S, H, hd = q.shape
    KVH = k.shape[2]
    for t in (q, k, v):
        assert t.stride(3) == 1 and t.stride(2) == hd
    if mask is not None and mask.dense is not None:  # any bool mask: the mask-driven tile loop, o as the rows `wo` reads
        if dropout is not None:
            raise L.LlxError("attn_dropout: MaskSpec(dense=...) has no dropout kernels (the rule forms doc_ids / prefix_len and the causal mask have)")
        mask = mask.prepared(B, S, q.device)
        o, lse = attn_mask_fwd(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), mask._rows, lse=True)
        return o.view(B, S, H, hd), lse
    o = torch.empty(B, S, H, hd, device=q.device, dtype=BF16)
    lse = torch.empty(B, H, S, device=q.device, dtype=torch.float32)
    d = p = fl = None
    if mask is not None:
        mask = mask.prepared(B, S, q.device)
        d, p, fl = mask.doc_ids, mask.prefix_len, mask._flags
    ev = _trace_begin(ATTN_TRACE)
    args = (L.ptr(q), q.stride(0), q.stride(1), L.ptr(k), k.stride(0), k.stride(1), L.ptr(v), v.stride(0), v.stride(1), L.ptr(o), o.stride(0),
            o.stride(1), L.ptr(lse), L.ptr(d), L.ptr(p), L.ptr(fl), B, S, H, KVH, hd, 1.0 / math.sqrt(hd))
    if dropout is not None:
        L.check(_lib().llx_attn_fwd_dropout(*args, *_dropout_operands(dropout, q.device, "attn_fwd"), L.stream()), "llx_attn_fwd_dropout")
    else:
        L.check(_lib().llx_attn_fwd(*args, L.stream()), "llx_attn_fwd")
    _trace_end(ATTN_TRACE, ev, "fwd", B, S, H)
    return o, lse


_ATTN_BWD_DS = os.environ.get("LLX_ATTN_BWD_DS", "0") == "1"
_ATTN_BWD_DS_MAX = int(float(os.environ.get("LLX_ATTN_BWD_DS_MAX_GB", "16")) * 2**30)


def _attn_bwd_operands(q: Tensor, k: Tensor, v: Tensor, o: Tensor, do: Tensor, lse: Tensor, dq: Tensor, dk: Tensor, dv: Tensor,
                       rope: Optional[Tensor]):
    """What attn_bwd and attn_mask_bwd share: the checks on q .. dv, lse and rope, the fp32 workspace (delta + dK/dV partials) and the
    leading (q .. dv) and trailing (B .. stream) arguments of the C entry points.  Returns (leading, trailing, workspace): the caller
    holds the workspace until its launch is issued."""
    _chk_bf16(q, k, v, o, do, dq, dk, dv)
    B, S, H, hd = q.shape
    KVH = k.shape[2]
    if rope is not None:
        assert rope.dtype is torch.float32 and rope.is_contiguous() and rope.shape[0] >= S and rope.shape[1:] == (64, 2)
    for t in (q, k, v, o, do, dq, dk, dv):
        assert t.stride(3) == 1 and t.stride(2) == hd
    assert lse.shape == (B, H, S) and lse.dtype is torch.float32 and lse.is_contiguous()
    delta = torch.empty(_lib().llx_attn_bwd_workspace_bytes(B, S, H, KVH) // 4, device=q.device, dtype=torch.float32)
    lead = [L.ptr(q), q.stride(0), q.stride(1), L.ptr(k), k.stride(0), k.stride(1), L.ptr(v), v.stride(0), v.stride(1), L.ptr(o), o.stride(0),
            o.stride(1), L.ptr(do), do.stride(0), do.stride(1), L.ptr(lse), L.ptr(delta), L.ptr(dq), dq.stride(0), dq.stride(1), L.ptr(dk),
            dk.stride(0), dk.stride(1), L.ptr(dv), dv.stride(0), dv.stride(1)]
    return lead, [B, S, H, KVH, hd, 1.0 / math.sqrt(hd), L.stream()], delta


def attn_bwd(q: Tensor, k: Tensor, v: Tensor, o: Tensor, do: Tensor, lse: Tensor, dq: Tensor, dk: Tensor, dv: Tensor,
             mask: Optional[MaskSpec] = None, rope: Optional[Tensor] = None, dropout=None) -> None:
    """rope (fp32 table [>= S, 64, 2]): q, k are the rotated projections; dq, dk come out as gradients of the un-rotated ones.
    dropout: exactly what attn_fwd was given (the rng tensor must still hold the forward's seed and counter)."""
    B, S, H = q.shape[:3]
    d = p = fl = None
    if mask is not None:
        mask = mask.prepared(B, S, q.device)
        if mask.dense is not None:
            if dropout is not None:
                raise L.LlxError("attn_dropout: MaskSpec(dense=...) has no dropout kernels (the rule forms doc_ids / prefix_len and the causal mask have)")
            return attn_mask_bwd(q, k, v, o, do, lse, dq, dk, dv, mask._rows, rope=rope)
        d, p, fl = mask.doc_ids, mask.prefix_len, mask._flags
    lead, trail, ws = _attn_bwd_operands(q, k, v, o, do, lse, dq, dk, dv, rope)
    # LLX_ATTN_BWD_DS=1: dS^T scratch (bf16 [B, H, Sp, Sp], 1.07 GB at S = 4096; capped by LLX_ATTN_BWD_DS_MAX_GB, default 16): with it every
    # product of the backward is computed once and dQ becomes a tiled product over the stored dS^T.  Measured at S = 4096: the
    # two routes take the same time (the dS^T round trip is bound by the CUs' fill rate), so the default is the route without scratch,
    # whose dQ kernel recomputes S and dP.
    ds = None
    ds_bytes = _lib().llx_attn_bwd_ds_bytes(B, S, H)
    if dropout is not None:  # the default route only: the dS scratch route has no dropout build
        ev = _trace_begin(ATTN_TRACE)
        L.check(_lib().llx_attn_bwd_dropout(*lead, L.ptr(d), L.ptr(p), L.ptr(fl), L.ptr(rope), None, *trail[:-1],
                                            *_dropout_operands(dropout, q.device, "attn_bwd"), trail[-1]), "llx_attn_bwd_dropout")
        _trace_end(ATTN_TRACE, ev, "bwd", B, S, H)
        return
    if _ATTN_BWD_DS and ds_bytes <= _ATTN_BWD_DS_MAX:
        ds = torch.empty(ds_bytes // 2, device=q.device, dtype=BF16)
    ev = _trace_begin(ATTN_TRACE)
    L.check(_lib().llx_attn_bwd(*lead, L.ptr(d), L.ptr(p), L.ptr(fl), L.ptr(rope), L.ptr(ds), *trail), "llx_attn_bwd")
    _trace_end(ATTN_TRACE, ev, "bwd", B, S, H)


def _mask_norm(mask: Tensor, B: int, Sq: int, Skv: int, H: Optional[int] = None) -> Optional[tuple[Tensor, int, int]]:
    """The one reading of a bool attention mask [Sq, Skv], [B | 1, Sq, Skv] or [B | 1, H | 1, Sq, Skv]: (m, m_sb, m_sh) with m the 4-d
    view, last dim dense, and the batch / head strides the kernels take (0 = broadcast) - or None if the mask does not fit.  With H the
    mask may be per head (attn_dense_fwd, attn_decode).  Without H it must be broadcast over heads and is bound for the MFMA tile loops
    (attn_mask_fwd / attn_mask_bwd and their tile flags), which read a row 4 bytes at a time: there a row stride below Skv
    (overlapping rows) is copied too.  No other copy is made: a dense last dim goes to the kernels as it lies."""
    m = mask
    while m.dim() < 4:
        m = m.unsqueeze(0)
    if m.dim() != 4 or m.shape[2:] != (Sq, Skv) or m.shape[0] not in (1, B) or m.shape[1] not in ((1,) if H is None else (1, H)):
        return None
    if m.stride(3) != 1 or (H is None and m.stride(2) < Skv):
        m = m.contiguous()
    return m, (m.stride(0) if m.shape[0] != 1 else 0), (m.stride(1) if m.shape[1] != 1 else 0)


def _mask_flags(mask: Tensor, B: int) -> Tensor:
    """The tile classes of a mask tensor, computed once per tensor (cached on it: every layer and both directions of a step share them)."""
    from . import ops  # (ops imports this module)

    return ops._cached(mask, f"maskflags{B}", lambda: attn_mask_flags(mask, B))


def attn_dense_fwd(q: Tensor, k: Tensor, v: Tensor, mask: Tensor) -> Tensor:
    """Inference attention with an explicit bool mask: q [B,H,Sq,128], k/v [B,KVH,Skv,128] (any strides, last dim dense),
    mask broadcastable to [B,H,Sq,Skv] -> o [B,H,Sq,128].  Forward only."""
    _chk_bf16(q, k, v)
    L.require_cuda(mask)
    B, H, Sq, hd = q.shape
    KVH, Skv = k.shape[1], k.shape[2]
    norm = _mask_norm(mask, B, Sq, Skv, H)
    assert mask.dtype is torch.bool and norm is not None, "mask must be bool and broadcastable to [B, H, Sq, Skv]"
    m, m_sb, m_sh = norm
    for t in (q, k, v):
        assert t.stride(3) == 1
    o = torch.empty(B, H, Sq, hd, device=q.device, dtype=BF16)
    L.check(_lib().llx_attn_dense_fwd(L.ptr(q), q.stride(0), q.stride(1), q.stride(2), L.ptr(k), k.stride(0), k.stride(1), k.stride(2),
                                      L.ptr(v), v.stride(0), v.stride(1), v.stride(2), L.ptr(o), o.stride(0), o.stride(1), o.stride(2),
                                      L.ptr(m), m_sb, m_sh, m.stride(2), B, H, KVH, Sq, Skv, hd, 1.0 / math.sqrt(hd), L.stream()),
            "llx_attn_dense_fwd")
    return o


def _mask_rows(mask: Tensor, B: int, Sq: int, Skv: int) -> tuple[Tensor, int]:
    """(m, m_sb) of a bool mask broadcast over heads, as the MFMA tile loops take it (m.stride(2) is their row stride)."""
    norm = _mask_norm(mask, B, Sq, Skv)
    if mask.dtype is not torch.bool or norm is None:
        raise L.LlxError(f"the mask must be bool and broadcast over heads ([B | 1, 1, Sq, Skv]), got {mask.dtype} {tuple(mask.shape)}; "
                         "per-head masks run on attn_dense_fwd")
    return norm[:2]


def attn_mask_routable(mask: Tensor, B: int, Sq: int, Skv: int) -> bool:
    """Whether attn_mask_fwd takes this mask: bool, broadcast over heads, at least 4 keys (its mask reads are 4 bytes wide)."""
    return mask.dtype is torch.bool and Skv >= 4 and _mask_norm(mask, B, Sq, Skv) is not None


def attn_mask_flags(mask: Tensor, B: int) -> Tensor:
    """Tile classes (uint8 [B, ceil(Sq/128), ceil(Skv/64)]: 0 skip, 1 partly masked, 2 unmasked) of a bool mask broadcastable to
    [B, 1, Sq, Skv]: one pass over the mask bytes."""
    L.require_cuda(mask)
    Sq, Skv = mask.shape[-2:]
    m, m_sb = _mask_rows(mask, B, Sq, Skv)
    fl = torch.empty(_lib().llx_attn_mask_flags_bytes(B, Sq, Skv), device=mask.device, dtype=torch.uint8)
    L.check(_lib().llx_attn_mask_tile_flags(L.ptr(m), m_sb, m.stride(2), L.ptr(fl), B, Sq, Skv, L.stream()), "llx_attn_mask_tile_flags")
    return fl


def attn_mask_fwd(q: Tensor, k: Tensor, v: Tensor, mask: Tensor, out: Optional[Tensor] = None, lse: bool = False):
    """Attention with an explicit bool mask broadcast over heads, on the MFMA tile loop of the training forward (KV-cache prefill, and
    the forward of training through a dense mask): q [B,H,Sq,128] as the transposed view of a row buffer (head stride 128), k/v
    [B,KVH,Skv,128] with any head / position strides (the caches, or views of the q|k|v rows), mask broadcastable to [B,1,Sq,Skv]
    -> o [B,Sq,H*128], the rows `wo` reads; with ``lse=True`` -> (o, lse), lse fp32 [B,H,Sq] in log2 units (what attn_mask_bwd takes).
    The tile classes are computed once per mask tensor (cached on it: every layer of a call shares them).  No host synchronisation."""
    _chk_bf16(q, k, v)
    L.require_cuda(mask)
    B, H, Sq, hd = q.shape
    KVH, Skv = k.shape[1], k.shape[2]
    assert v.shape == k.shape
    for t in (q, k, v):
        assert t.stride(3) == 1
    if q.stride(1) != hd:  # heads must sit side by side in a row
        q = q.transpose(1, 2).contiguous().transpose(1, 2)
    m, m_sb = _mask_rows(mask, B, Sq, Skv)
    fl = _mask_flags(mask, B)
    if out is None:
        out = torch.empty(B, Sq, H * hd, device=q.device, dtype=BF16)
    assert out.shape == (B, Sq, H * hd) and out.dtype is BF16 and out.stride(2) == 1
    lse_t = torch.empty(B, H, Sq, device=q.device, dtype=torch.float32) if lse else None
    L.check(_lib().llx_attn_mask_fwd(L.ptr(q), q.stride(0), q.stride(2), L.ptr(k), k.stride(0), k.stride(1), k.stride(2), L.ptr(v), v.stride(0),
                                     v.stride(1), v.stride(2), L.ptr(out), out.stride(0), out.stride(1), L.ptr(lse_t), L.ptr(m), m_sb, m.stride(2),
                                     L.ptr(fl), B, Sq, Skv, H, KVH, hd, 1.0 / math.sqrt(hd), L.stream()), "llx_attn_mask_fwd")
    return (out, lse_t) if lse else out


def attn_mask_bwd(q: Tensor, k: Tensor, v: Tensor, o: Tensor, do: Tensor, lse: Tensor, dq: Tensor, dk: Tensor, dv: Tensor, mask: Tensor,
                  rope: Optional[Tensor] = None) -> None:
    """Backward of attn_mask_fwd with Sq = Skv = S: q / o / do / dq [B,S,H,128], k / v / dk / dv [B,S,KVH,128] (last two dims dense,
    batch / sequence strides free: views of fused q|k|v rows work), lse [B,H,S] from attn_mask_fwd(..., lse=True), mask bool
    broadcastable to [B,1,S,S].  rope as in attn_bwd.  A key that no row attends to gets exact zeros in dk / dv.  The tile classes are
    the ones attn_mask_fwd cached on the mask tensor.  No host synchronisation."""
    L.require_cuda(mask)
    B, S, H = q.shape[:3]
    m, m_sb = _mask_rows(mask, B, S, S)
    fl = _mask_flags(mask, B)
    lead, trail, ws = _attn_bwd_operands(q, k, v, o, do, lse, dq, dk, dv, rope)
    ev = _trace_begin(ATTN_TRACE)
    L.check(_lib().llx_attn_mask_bwd(*lead, L.ptr(m), m_sb, m.stride(2), L.ptr(fl), L.ptr(rope), *trail), "llx_attn_mask_bwd")
    _trace_end(ATTN_TRACE, ev, "bwd", B, S, H)


# ------------------------------------------------------------------------------------------------- decode path (csrc/decode.hip)
GV_NONE, GV_RESIDUAL, GV_QKV, GV_SWIGLU = 0, 1, 2, 3  # csrc/wstream.h
GV_QKV_F8 = 4  # GV_QKV into FP8 caches: callers ask for GV_QKV, the cache dtype picks it (_stream_operands)
KV_DTYPES = ("bf16", "fp8")


def _kv_fp8(k_cache: Tensor, v_cache: Tensor) -> bool:
    """True for a pair of FP8 caches (uint8 E4M3 codes), False for a bf16 pair; anything else - a mixed pair too - is refused."""
    if k_cache.dtype is torch.uint8 and v_cache.dtype is torch.uint8:
        return True
    if k_cache.dtype is BF16 and v_cache.dtype is BF16:
        return False
    raise L.LlxError(f"the k and v caches must both be bf16 or both uint8 (FP8 codes), got {k_cache.dtype} and {v_cache.dtype}")


def _workspace(cache: dict, device, nbytes: int, floor: int = 0) -> Tensor:
    """The grow-only uint8 workspace of the current stream of `device`, at least nbytes long (first allocation: at least floor bytes)."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = cache[key] = torch.empty(max(nbytes, floor), device=device, dtype=torch.uint8)
    return ws


def _stream_operands(ws, x: Tensor, norm, epilogue: int, out: Optional[Tensor], res: Optional[Tensor], qkv: Optional[tuple], batched: bool,
                     wcols: Optional[int] = None):
    """What gemv and gemm_rows16 share (the StreamArgs of csrc/wstream.h): the checks on the common operands, the output tensor and the
    leading arguments of the C entry points, w0 .. v_cache.  Returns (arguments, out, N, k_cache, pos).  GV_QKV with uint8 (FP8) caches
    becomes epilogue 4: the caches' strides, which the callers append, are then bytes, as the entry points want them.  batched: the q|k|v mode of
    gemm_rows16 (table row 0 for every row, row m into cache[m]); else row m takes table row m and the cache has batch 1.  wcols: the
    stored columns of a weight row where they are not K (packed MXFP4 rows: K / 2 bytes)."""
    M, Kd = x.shape
    assert 1 <= len(ws) <= 3 and all(w.dim() == 2 and w.shape[1] == (wcols or Kd) and w.stride(1) == 1 for w in ws) and x.stride(1) == 1
    ns = [w.shape[0] for w in ws] + [0] * (3 - len(ws))
    N = sum(ns)
    wp = [L.ptr(w) for w in ws] + [None] * (3 - len(ws))
    lw = [w.stride(0) for w in ws] + [0] * (3 - len(ws))
    n_out = {GV_NONE: N, GV_RESIDUAL: N, GV_QKV: qkv[1] if qkv else 0, GV_SWIGLU: ns[0]}[epilogue]
    if out is None:
        out = torch.empty(M, n_out, device=x.device, dtype=BF16)
    assert out.shape == (M, n_out) and out.stride(1) == 1
    nw, eps = (norm[0], float(norm[1])) if norm is not None else (None, 0.0)
    rope = kc = vc = pos = None
    n_q = n_k = 0
    if epilogue == GV_QKV:
        rope, n_q, n_k, kc, vc, pos = qkv
        assert rope.dtype is torch.float32 and rope.is_contiguous() and rope.shape[0] >= (1 if batched else M) and rope.shape[1:] == (64, 2)
        assert kc.shape == vc.shape and kc.dim() == 4 and kc.shape[3] == 128 and kc.stride() == vc.stride() and kc.stride(3) == 1
        assert kc.shape[0] >= M if batched else kc.shape[0] == 1
        L.require_cuda(kc, vc)
        if _kv_fp8(kc, vc):
            epilogue = GV_QKV_F8
        assert pos.dtype is torch.int64 and pos.shape == (M,) and pos.is_contiguous() and pos.is_cuda
    if epilogue == GV_RESIDUAL:
        assert res is not None and res.shape == (M, N) and res.stride(1) == 1 and res.dtype is BF16
    args = [wp[0], lw[0], ns[0], wp[1], lw[1], ns[1], wp[2], lw[2], ns[2], L.ptr(x), x.stride(0), M, Kd, L.ptr(nw), eps, epilogue, L.ptr(out), out.stride(0),
            L.ptr(res), res.stride(0) if res is not None else 0, L.ptr(rope), n_q, n_k, L.ptr(kc), L.ptr(vc)]
    return args, out, N, kc, pos


def _chk_colscale(fn: str, ws, colscale) -> None:
    """DoRA's cached row factors as gemv and gemm_rows16 (fn: the caller, whose name begins the message) both take them."""
    if len(colscale) != len(ws) or not all(c.dtype is BF16 and c.shape == (w.shape[0],) and c.is_contiguous() for c, w in zip(colscale, ws)):
        raise L.LlxError(f"{fn}: colscale must hold one contiguous bf16 [n_s] tensor per weight")
    L.require_cuda(*colscale)


def _chk_int8_weights(fn: str, ws, x: Tensor, wscale, i8) -> None:
    """What gemv and gemm_rows16 (fn) both ask of a call with int8 weights; i8: which of ws are int8."""
    if not all(i8):
        raise L.LlxError(f"{fn}: bf16 and int8 weights in one call (all members of a fused group must be of one kind)")
    if x.shape[1] % 16 != 0:
        raise L.LlxError(f"{fn}: K={x.shape[1]} must be a multiple of 16 for int8 weights")
    assert wscale is not None and len(wscale) == len(ws), "int8 weights need their per-row scales"
    assert all(sc.shape == (w.shape[0],) and sc.is_contiguous() for sc, w in zip(wscale, ws))
    _chk_bf16(x, *wscale)
    L.require_cuda(*ws)


def _lora_operands(ws, x: Tensor, lora):
    """The adapter operands of both streams, lora = (b factors, t [M, sum r], scale) or None: (bs, ranks, t, ldt, scale) as the entry points
    take them, absent segments and an absent adapter as null / 0."""
    bs, ranks, t, ldt, lscale = [None] * 3, [0] * 3, None, 0, 0.0
    if lora is not None:
        b_list, t, lscale = lora
        assert len(b_list) == len(ws) and t.dtype is BF16 and t.shape[0] == x.shape[0] and t.stride(1) == 1
        for i, b in enumerate(b_list):
            assert b.dtype is BF16 and b.is_contiguous() and b.shape[0] == ws[i].shape[0]
            bs[i], ranks[i] = b, b.shape[1]
        assert t.shape[1] == sum(ranks)
        ldt = t.stride(0)
    return bs, ranks, t, ldt, float(lscale)


def _gemv_operands(ws, x: Tensor, norm, epilogue: int, out, res, qkv, lora, wcols: Optional[int] = None):
    """The arguments every GEMV entry point begins with (those of llx_gemv_bf16 before the stream), and the output tensor."""
    args, out, _, kc, pos = _stream_operands(ws, x, norm, epilogue, out, res, qkv, batched=False, wcols=wcols)
    args += [kc.stride(1), kc.stride(2)] if kc is not None else [0, 0]
    bs, ranks, t, ldt, lscale = _lora_operands(ws, x, lora)
    args += [L.ptr(pos), L.ptr(bs[0]), L.ptr(bs[1]), L.ptr(bs[2]), ranks[0], ranks[1], ranks[2], L.ptr(t), ldt, lscale]
    return args, out


def _gemv_mxfp4(ws, scales, x: Tensor, norm, epilogue: int, out, res, qkv, lora, alone: bool) -> Tensor:
    """gemv on packed MXFP4 rows (llx_gemv_mxfp4)."""
    if not alone:
        raise L.LlxError("gemv: mxscale (MXFP4 weights) excludes wscale, dynamic and colscale")
    Kd = x.shape[1]
    if Kd % 32 != 0:
        raise L.LlxError(f"gemv: K={Kd} must be a multiple of 32 for MXFP4 weights")
    if len(scales) != len(ws) or not all(w.dtype is torch.uint8 and sc.dtype is torch.uint8 and sc.dim() == 2 and sc.shape == (w.shape[0], Kd // 32)
                                         and sc.stride(1) == 1 for w, sc in zip(ws, scales)):
        raise L.LlxError("gemv: MXFP4 weights are uint8 [n_s, K/2] rows with one uint8 [n_s, K/32] scale tensor each")
    _chk_bf16(x)
    L.require_cuda(*ws, *scales)
    args, out = _gemv_operands(ws, x, norm, epilogue, out, res, qkv, lora, wcols=Kd // 2)
    sp = [v for sc in scales for v in (L.ptr(sc), sc.stride(0))] + [None, 0] * (3 - len(ws))
    L.check(_lib().llx_gemv_mxfp4(*args, *sp, L.stream()), "llx_gemv_mxfp4")
    return out


def quantize_mxfp4(x: Tensor) -> tuple[Tensor, Tensor]:
    """x [N, K] bf16 or fp32 (K % 32 == 0, unit column stride) -> (packed uint8 [N, K/2], scale uint8 [N, K/32]): OCP MXFP4, the rule of
    csrc/mxfp4.hip (llx_quantize_mxfp4).  Finite input is the caller's to check."""
    L.require_cuda(x)
    assert x.dim() == 2 and x.dtype in (BF16, torch.float32)
    N, Kd = x.shape
    if Kd % 32 != 0:
        raise L.LlxError(f"quantize_mxfp4: K={Kd} must be a multiple of 32")
    per16 = 4 if x.dtype is torch.float32 else 8
    if x.stride(1) != 1 or x.stride(0) % per16 != 0 or x.data_ptr() % 16 != 0:
        x = x.contiguous()
    packed = torch.empty(N, Kd // 2, device=x.device, dtype=torch.uint8)
    scale = torch.empty(N, Kd // 32, device=x.device, dtype=torch.uint8)
    L.check(_lib().llx_quantize_mxfp4(L.ptr(x), x.stride(0), int(x.dtype is torch.float32), N, Kd, L.ptr(packed), L.ptr(scale), L.stream()),
            "llx_quantize_mxfp4")
    return packed, scale


def dequantize_mxfp4(packed: Tensor, scale: Tensor, *, transpose: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """The bf16 image [N, K] of packed MXFP4 rows (exact), or with transpose [K, N]; out: a row-strided view to fill (llx_dequantize_mxfp4)."""
    L.require_cuda(packed, scale)
    assert packed.dim() == 2 and scale.dim() == 2 and packed.dtype is torch.uint8 and scale.dtype is torch.uint8
    assert packed.stride(1) == 1 and scale.stride(1) == 1
    N, Kd = packed.shape[0], packed.shape[1] * 2
    assert scale.shape == (N, Kd // 32) and Kd % 32 == 0
    shape = (Kd, N) if transpose else (N, Kd)
    if out is None:
        out = torch.empty(shape, device=packed.device, dtype=BF16)
    assert out.shape == shape and out.dtype is BF16 and out.stride(1) == 1
    L.check(_lib().llx_dequantize_mxfp4(L.ptr(packed), packed.stride(0), L.ptr(scale), scale.stride(0), N, Kd, L.ptr(out), out.stride(0),
                                        int(transpose), L.stream()), "llx_dequantize_mxfp4")
    return out


def gemv(ws: Sequence[Tensor], x: Tensor, *, norm: Optional[tuple[Tensor, float]] = None, epilogue: int = GV_NONE, out: Optional[Tensor] = None,
         res: Optional[Tensor] = None, qkv: Optional[tuple] = None, lora: Optional[tuple] = None, wscale: Optional[Sequence[Tensor]] = None,
         dynamic: bool = False, colscale: Optional[Sequence[Tensor]] = None, mxscale: Optional[Sequence[Tensor]] = None) -> Tensor:
    """out = epilogue([rmsnorm(x) | x] @ cat(ws)^T) for M = x.shape[0] <= 4 rows: every CU streams weight rows (llx_gemv_bf16).
    ws: 1-3 weights [n_s, K]; norm = (weight, eps); res [M, N] for GV_RESIDUAL; qkv = (rope_table, n_q, n_k, k_cache, v_cache, input_pos)
    for GV_QKV (caches [1, KVH, Smax, 128]; returns q [M, n_q]); GV_SWIGLU returns h [M, n_0]; lora = (b factors, t [M, sum r], scale).
    int8 ws (the int_data of Int8LinearWeights, all members of the call) with wscale = their bf16 per-row scales run llx_gemv_i8:
    weight-only arithmetic, or with dynamic=True the rows of x quantised on chip and integer dot products (subclasses/int8.py:106-121).
    colscale (bf16 weights only): one contiguous bf16 [n_s] factor per weight, DoRA's cached m / ||W + s B A||_row (ops.dora_scale_cached);
    the linear's bf16 output is multiplied by it and rounded before the epilogue (llx_gemv_bf16_dora).
    mxscale: ws are the packed uint8 [n_s, K/2] rows of MXFP4LinearWeights (all members of the call) and mxscale their uint8 [n_s, K/32]
    scale bytes (llx_gemv_mxfp4): the rounding points of the bf16 call on the dequantised image; K = x.shape[1] % 32 == 0."""
    if mxscale is not None:
        return _gemv_mxfp4(ws, mxscale, x, norm, epilogue, out, res, qkv, lora, wscale is None and not dynamic and colscale is None)
    i8 = [w.dtype is torch.int8 for w in ws]
    if colscale is not None:
        if any(i8):
            raise L.LlxError("gemv: colscale (DoRA) on int8 weights is not supported")
        _chk_colscale("gemv", ws, colscale)
    if any(i8):
        _chk_int8_weights("gemv", ws, x, wscale, i8)
    else:
        assert wscale is None and not dynamic, "wscale / dynamic belong to int8 weights"
        _chk_bf16(x, *ws)
    args, out = _gemv_operands(ws, x, norm, epilogue, out, res, qkv, lora)
    if any(i8):
        sp = [L.ptr(sc) for sc in wscale] + [None] * (3 - len(ws))
        L.check(_lib().llx_gemv_i8(*args, sp[0], sp[1], sp[2], int(bool(dynamic)), L.stream()), "llx_gemv_i8")
    elif colscale is not None:
        cp = [L.ptr(c) for c in colscale] + [None] * (3 - len(ws))
        L.check(_lib().llx_gemv_bf16_dora(*args, cp[0], cp[1], cp[2], L.stream()), "llx_gemv_bf16_dora")
    else:
        L.check(_lib().llx_gemv_bf16(*args, L.stream()), "llx_gemv_bf16")
    return out


_ROWS16_WS: dict = {}


def gemm_rows16(ws: Sequence[Tensor], x: Tensor, *, norm: Optional[tuple[Tensor, float]] = None, epilogue: int = GV_NONE, out: Optional[Tensor] = None,
                res: Optional[Tensor] = None, qkv: Optional[tuple] = None, wscale: Optional[Sequence[Tensor]] = None, lora: Optional[tuple] = None,
                colscale: Optional[Sequence[Tensor]] = None) -> Tensor:
    """gemv's product for 2 <= M = x.shape[0] <= 16 rows - a batch of sequences, one token each - on the matrix pipe (llx_gemm_rows16_bf16):
    the weights stream once whatever M is.  bf16 weights; norm, res and the GV_* epilogues as gemv, except GV_QKV, which is the batched
    mode: qkv = (rope_table, n_q, n_k, k_cache, v_cache, pos) with caches [B >= M, KVH, Smax, 128] and pos int64 [M]; row m is rotated by
    table row 0 and its k / v heads go to cache[m] at pos[m]; returns q [M, n_q].
    int8 ws (the int_data of dynamic Int8LinearWeights, all members of the call) with wscale = their bf16 per-row scales run
    llx_gemm_rows16_i8: the rows of x quantised on chip, int8 MFMA, the reference's dequantisation (the dynamic kind only: the
    weight-only kind has no batched stream).
    lora = (b factors, t [M, sum r], scale) and colscale (bf16 weights only) as gemv's: one contiguous bf16 [n_s, r_s] factor per weight
    with r_s in {16, 32, 48, 64}, t = gemm_rows16(a factors, x, norm=norm); the adapter term of a tile is an MFMA chain in its epilogue
    (llx_gemm_rows16_bf16_lora - with colscale DoRA's cached row factors - and llx_gemm_rows16_i8_lora), gemv's rounding points."""
    i8 = [w.dtype is torch.int8 for w in ws]
    if colscale is not None:
        if any(i8):
            raise L.LlxError("gemm_rows16: colscale (DoRA) on int8 weights is not supported")
        if lora is None:
            raise L.LlxError("gemm_rows16: colscale (DoRA) needs the lora operands")
        _chk_colscale("gemm_rows16", ws, colscale)
    if any(i8):
        _chk_int8_weights("gemm_rows16", ws, x, wscale, i8)
    else:
        assert wscale is None, "wscale belongs to int8 weights"
        _chk_bf16(x, *ws)
    args, out, N, kc, pos = _stream_operands(ws, x, norm, epilogue, out, res, qkv, batched=True)
    args += [kc.stride(0), kc.stride(1), kc.stride(2), kc.shape[2]] if kc is not None else [0, 0, 0, 0]
    largs = None
    if lora is not None:
        bs, ranks, t, ldt, lscale = _lora_operands(ws, x, lora)
        L.require_cuda(t, *lora[0])
        largs = [L.ptr(bs[0]), L.ptr(bs[1]), L.ptr(bs[2]), ranks[0], ranks[1], ranks[2], L.ptr(t), ldt, lscale]
    if any(i8):
        wsp = _workspace(_ROWS16_WS, x.device, _lib().llx_gemm_rows16_i8_workspace_bytes(x.shape[0], N, x.shape[1], epilogue), 1 << 20)
        sp = [L.ptr(sc) for sc in wscale] + [None] * (3 - len(ws))
        if largs is not None:
            L.check(_lib().llx_gemm_rows16_i8_lora(*args, L.ptr(pos), L.ptr(wsp), wsp.numel(), sp[0], sp[1], sp[2], *largs, L.stream()),
                    "llx_gemm_rows16_i8_lora")
            return out
        L.check(_lib().llx_gemm_rows16_i8(*args, L.ptr(pos), L.ptr(wsp), wsp.numel(), sp[0], sp[1], sp[2], L.stream()), "llx_gemm_rows16_i8")
        return out
    wsp = _workspace(_ROWS16_WS, x.device, _lib().llx_gemm_rows16_workspace_bytes(x.shape[0], N, x.shape[1], epilogue), 1 << 20)
    if largs is not None:
        cp = [L.ptr(c) for c in colscale] + [None] * (3 - len(ws)) if colscale is not None else [None] * 3
        L.check(_lib().llx_gemm_rows16_bf16_lora(*args, L.ptr(pos), L.ptr(wsp), wsp.numel(), *largs, cp[0], cp[1], cp[2], L.stream()),
                "llx_gemm_rows16_bf16_lora")
        return out
    L.check(_lib().llx_gemm_rows16_bf16(*args, L.ptr(pos), L.ptr(wsp), wsp.numel(), L.stream()), "llx_gemm_rows16_bf16")
    return out


def mask_extent(mask: Tensor) -> Tensor:
    """Device int32 [1]: 1 + the largest key index any row of the bool mask [..., Skv] allows (0 if none)."""
    L.require_cuda(mask)
    assert mask.dtype is torch.bool
    m2 = mask.reshape(-1, mask.shape[-1])
    if m2.stride(1) != 1:
        m2 = m2.contiguous()
    ext = torch.empty(1, device=mask.device, dtype=torch.int32)
    L.check(_lib().llx_mask_extent(L.ptr(m2), m2.stride(0), m2.shape[0], m2.shape[1], L.ptr(ext), L.stream()), "llx_mask_extent")
    return ext


def kv_scatter(k: Tensor, v: Tensor, k_cache: Tensor, v_cache: Tensor, input_pos: Tensor) -> None:
    """k_cache[:, :, input_pos] = k ; v_cache[:, :, input_pos] = v  (KVCache.update, modelling/llama.py:83-90); k / v [B, KVH, L, 128] views.
    input_pos [L], or [B, L]: sequence b at its own positions, cache[b, :, input_pos[b, l]] = k[b, :, l] (llx_kv_scatter_rows).
    uint8 caches (FP8) take q(k), q(v): llx_kv_scatter_f8 / llx_kv_scatter_rows_f8."""
    _chk_bf16(k, v)
    L.require_cuda(input_pos, k_cache, v_cache)
    f8 = "_f8" if _kv_fp8(k_cache, v_cache) else ""
    B, KVH, Lq, hd = k.shape
    assert v.shape == k.shape and k.stride() == v.stride() and k.stride(3) == 1 and k_cache.stride() == v_cache.stride() and k_cache.stride(3) == 1
    assert k_cache.shape[0] == B and k_cache.shape[1] == KVH and k_cache.shape[3] == hd and input_pos.shape in ((Lq,), (B, Lq))
    pos = input_pos.to(torch.int64).contiguous()
    if pos.dim() == 2:
        fn = "llx_kv_scatter_rows" + f8
        L.check(getattr(_lib(), fn)(L.ptr(k), L.ptr(v), k.stride(0), k.stride(1), k.stride(2), L.ptr(k_cache), L.ptr(v_cache), k_cache.stride(0),
                                    k_cache.stride(1), k_cache.stride(2), L.ptr(pos), pos.stride(0), B, KVH, Lq, k_cache.shape[2], hd, L.stream()), fn)
        return
    fn = "llx_kv_scatter" + f8
    L.check(getattr(_lib(), fn)(L.ptr(k), L.ptr(v), k.stride(0), k.stride(1), k.stride(2), L.ptr(k_cache), L.ptr(v_cache), k_cache.stride(0),
                                k_cache.stride(1), k_cache.stride(2), L.ptr(pos), B, KVH, Lq, k_cache.shape[2], hd, L.stream()), fn)


def kv_dequantize(cache: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """The bf16 image dq(cache) of an FP8 cache (uint8 [B, KVH, S, 128], any batch / head / position strides; exact): contiguous
    [B, KVH, S, 128] (llx_kv_dequantize_f8)."""
    L.require_cuda(cache)
    if cache.dtype is not torch.uint8 or cache.dim() != 4 or cache.stride(3) != 1:
        raise L.LlxError("kv_dequantize: an FP8 cache is a uint8 [B, KVH, S, 128] tensor with a dense last dim")
    B, KVH, S, hd = cache.shape
    if out is None:
        out = torch.empty(B, KVH, S, hd, device=cache.device, dtype=BF16)
    assert out.shape == cache.shape and out.dtype is BF16 and out.is_contiguous()
    L.check(_lib().llx_kv_dequantize_f8(L.ptr(cache), cache.stride(0), cache.stride(1), cache.stride(2), L.ptr(out), B, KVH, S, hd, L.stream()),
            "llx_kv_dequantize_f8")
    return out


_DECODE_WS: dict = {}
_DECODE_WGS = 512  # workgroups the decode attention aims for (nsplit * B * KVH)


def _decode_nsplit(B: int, KVH: int, Skv: int) -> int:
    """Key ranges per (batch, kv head) of attn_decode: workgroups = nsplit * B * KVH, two or more per CU keep more rows in flight; at
    least 32 keys per range, at most 128 ranges."""
    return max(1, min(-(-Skv // 32), -(-_DECODE_WGS // (B * KVH)), 128))


def attn_decode(q: Tensor, k_cache: Tensor, v_cache: Tensor, mask: Tensor, extent: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """SDPA over the cache for a few query tokens: q [B, H, M, 128] (any strides, last dim dense), caches [B, KVH, Skv, 128], bool mask
    broadcastable to [B, H, M, Skv] -> o [B, H, M, 128] stored as [B, M, H*128] (the layout wo reads).  M * H / KVH <= 16.
    uint8 caches (FP8) are read as codes (llx_attn_decode_f8): the result of this call on their bf16 images."""
    _chk_bf16(q)
    L.require_cuda(mask, k_cache, v_cache)
    fn = "llx_attn_decode_f8" if _kv_fp8(k_cache, v_cache) else "llx_attn_decode"
    B, H, M, hd = q.shape
    KVH, Skv = k_cache.shape[1], k_cache.shape[2]
    norm = _mask_norm(mask, B, M, Skv, H)
    assert mask.dtype is torch.bool and norm is not None and k_cache.stride() == v_cache.stride()
    m, m_sb, m_sh = norm
    nsplit = _decode_nsplit(B, KVH, Skv)
    nbytes = _lib().llx_attn_decode_workspace_bytes(B, H, M, nsplit)
    ws = _workspace(_DECODE_WS, q.device, nbytes)
    if out is None:
        out = torch.empty(B, M, H * hd, device=q.device, dtype=BF16)
    o4 = out.view(B, M, H, hd)
    L.check(getattr(_lib(), fn)(L.ptr(q), q.stride(0), q.stride(1), q.stride(2), L.ptr(k_cache), L.ptr(v_cache), k_cache.stride(0), k_cache.stride(1),
                                k_cache.stride(2), L.ptr(out), o4.stride(0), o4.stride(2), o4.stride(1), L.ptr(m), m_sb, m_sh, m.stride(2), L.ptr(extent),
                                L.ptr(ws), B, H, KVH, M, Skv, nsplit, hd, 1.0 / math.sqrt(hd), L.stream()), fn)
    return out


# ------------------------------------------------------------------------------------------------- token sampler
def sample(logits: Tensor, *, temperature: float, top_k: int = 0, top_p: float = 1.0, seed: int = 0, pos: Tensor, out: Optional[Tensor] = None,
           history: Optional[Tensor] = None, hist_base: int = 0, advance: bool = False, eos_id: Optional[int] = None,
           finished: Optional[Tensor] = None, aux: bool = False, counts: Optional[Tensor] = None, repetition_penalty: float = 1.0,
           presence_penalty: float = 0.0, frequency_penalty: float = 0.0, logprob_history: Optional[Tensor] = None):
    """One token for each row of logits [R, V] or [1, R, V] (bf16 or fp32, last dim dense, any row stride and start offset), in one launch
    and without a host read: greedy at temperature 0, else temperature / top-k / top-p by the rules of llx/sampling.py.  pos (device int64
    [R]) is the counter of the random draw; advance stores pos + 1 back.  history (int64 [R, cap]) receives the token at pos - hist_base
    when that lies inside it.  eos_id with finished (device int32 [R]): finished rows repeat eos_id and touch nothing, a sampled eos_id
    sets the flag.  Returns the tokens (int64 [R]), with aux=True (tokens, u fp32, threshold logit fp32, kept int32).

    counts (device int32 [R, >= V], last dim dense): how often each token has occurred in the row's sequence.  With it the row is read
    through the three penalties (rule 0 of llx/sampling.py; all of them at "off" change nothing) and the launch adds one at (r, token);
    without it the penalties must be off.  logprob_history (fp32, the shape and strides of history, which it needs) receives the
    token's log-probability on the raw logits where history receives the token.  A finished row touches neither.  With all five at
    their defaults this is llx_sample_rows as before; otherwise llx_sample_rows_ext."""
    from .sampling import check_params, check_penalties, penalties_on

    check_params(temperature, top_k, top_p, seed)
    check_penalties(repetition_penalty, presence_penalty, frequency_penalty)
    L.require_cuda(logits, pos, out, history, finished, counts, logprob_history)
    if logits.dim() == 3:
        if logits.shape[0] != 1:
            raise L.LlxError(f"sample: logits [B, R, V] need B == 1 (got {tuple(logits.shape)})")
        logits = logits[0]
    if logits.dim() != 2 or logits.dtype not in (BF16, torch.float32):
        raise L.LlxError(f"sample: logits must be bf16 or fp32 [R, V] (got {logits.dtype} {tuple(logits.shape)})")
    if logits.stride(1) != 1 or (logits.shape[0] > 1 and logits.stride(0) < logits.shape[1]):
        logits = logits.contiguous()
    R, V = logits.shape
    if pos.dtype is not torch.int64 or pos.shape != (R,) or not pos.is_contiguous():
        raise L.LlxError(f"sample: pos must be a contiguous device int64 [{R}] (got {pos.dtype} {tuple(pos.shape)})")
    if out is None:
        out = torch.empty(R, device=logits.device, dtype=torch.int64)
    elif out.dtype is not torch.int64 or out.numel() != R or not out.is_contiguous():
        raise L.LlxError(f"sample: out must be a contiguous int64 tensor of {R} elements")
    h_ld = h_cap = 0
    if history is not None:
        if history.dtype is not torch.int64 or history.dim() != 2 or history.shape[0] != R or history.stride(1) != 1:
            raise L.LlxError(f"sample: history must be int64 [{R}, cap] with a dense last dim")
        h_ld, h_cap = (history.stride(0) if R > 1 else history.shape[1]), history.shape[1]
    if (eos_id is None) != (finished is None):
        raise L.LlxError("sample: eos_id and finished go together")
    if finished is not None and (finished.dtype is not torch.int32 or finished.shape != (R,) or not finished.is_contiguous()):
        raise L.LlxError(f"sample: finished must be a contiguous device int32 [{R}]")
    au = at = ak = None
    if aux:
        au = torch.empty(R, device=logits.device, dtype=torch.float32)
        at = torch.empty(R, device=logits.device, dtype=torch.float32)
        ak = torch.empty(R, device=logits.device, dtype=torch.int32)
    if counts is None and penalties_on(repetition_penalty, presence_penalty, frequency_penalty):
        raise L.LlxError("sample: repetition_penalty / presence_penalty / frequency_penalty need the counts table")
    if counts is not None or logprob_history is not None:
        ldc = 0
        if counts is not None:
            if counts.dtype is not torch.int32 or counts.dim() != 2 or counts.shape[0] != R or counts.shape[1] < V or counts.stride(1) != 1 \
                    or (R > 1 and counts.stride(0) < V):
                raise L.LlxError(f"sample: counts must be a device int32 [{R}, >= {V}] with a dense last dim (got {counts.dtype} {tuple(counts.shape)})")
            ldc = counts.stride(0) if R > 1 else counts.shape[1]
        if logprob_history is not None:
            if history is None:
                raise L.LlxError("sample: logprob_history goes with history (they share one geometry)")
            if logprob_history.dtype is not torch.float32 or logprob_history.shape != history.shape or logprob_history.stride() != history.stride():
                raise L.LlxError(f"sample: logprob_history must be fp32 with the shape and strides of history {tuple(history.shape)} "
                                 f"(got {logprob_history.dtype} {tuple(logprob_history.shape)})")
        L.check(_lib().llx_sample_rows_ext(L.ptr(logits), 0 if logits.dtype is BF16 else 1, logits.stride(0) if R > 1 else V, R, V, float(temperature),
                                           int(top_k), float(top_p), int(seed), L.ptr(pos), L.ptr(out), L.ptr(history), h_ld, h_cap, int(hist_base),
                                           1 if advance else 0, int(eos_id) if eos_id is not None else -1, L.ptr(finished), L.ptr(au), L.ptr(at),
                                           L.ptr(ak), L.ptr(counts), ldc, float(repetition_penalty), float(presence_penalty),
                                           float(frequency_penalty), L.ptr(logprob_history), L.stream()), "llx_sample_rows_ext")
        tokens = out.view(R)
        return (tokens, au, at, ak) if aux else tokens
    L.check(_lib().llx_sample_rows(L.ptr(logits), 0 if logits.dtype is BF16 else 1, logits.stride(0) if R > 1 else V, R, V, float(temperature),
                                   int(top_k), float(top_p), int(seed), L.ptr(pos), L.ptr(out), L.ptr(history), h_ld, h_cap, int(hist_base),
                                   1 if advance else 0, int(eos_id) if eos_id is not None else -1, L.ptr(finished), L.ptr(au), L.ptr(at),
                                   L.ptr(ak), L.stream()), "llx_sample_rows")
    tokens = out.view(R)
    return (tokens, au, at, ak) if aux else tokens


def lookup_step(picks: Tensor, seq: Tensor, length: Tensor, step_tok: Tensor, step_pos: Tensor, finished: Tensor, counters: Tensor, *,
                P: int, n: int, k: int, g: int, eos_id: Optional[int] = None, init: bool = False) -> None:
    """The bookkeeping of one greedy step with k prompt-lookup draft tokens, in one launch and without a host read (csrc/lookup.hip;
    the host reference is sampling.lookup_accept then sampling.lookup_draft).  picks (int64 [k + 1]): the greedy picks of the logits rows
    of the step that fed step_tok (int64 [k + 1]) at step_pos (int64 [k + 1]).  The confirmed tokens are appended to seq (int64 [cap],
    cap >= P + n) at length (int64 [1]), step_tok / step_pos become the next step's, finished (int32 [1]) is set by an emitted eos_id,
    counters (int64 [2]) += (1, emitted - 1).  init: the first token after the prefill (picks [1] or longer, only picks[0] is read).
    Nothing changes once finished is set or length == P + n."""
    L.require_cuda(picks, seq, length, step_tok, step_pos, finished, counters)
    for name, t, dt, numel in (("picks", picks, torch.int64, 1 if init else k + 1), ("seq", seq, torch.int64, P + n), ("length", length, torch.int64, 1),
                               ("step_tok", step_tok, torch.int64, k + 1), ("step_pos", step_pos, torch.int64, k + 1),
                               ("finished", finished, torch.int32, 1), ("counters", counters, torch.int64, 2)):
        exact = name not in ("picks", "seq")
        if t.dtype is not dt or t.dim() != 1 or not t.is_contiguous() or (t.numel() != numel if exact else t.numel() < numel):
            raise L.LlxError(f"lookup_step: {name} must be a contiguous device {str(dt).removeprefix('torch.')} [{numel}{'' if exact else ' or more'}] "
                             f"(got {t.dtype} {tuple(t.shape)})")
    L.check(_lib().llx_lookup_step(L.ptr(picks), L.ptr(seq), seq.numel(), L.ptr(length), L.ptr(step_tok), L.ptr(step_pos), L.ptr(finished),
                                   L.ptr(counters), int(P), int(n), int(k), int(g), int(eos_id) if eos_id is not None else -1, 1 if init else 0,
                                   L.stream()), "llx_lookup_step")


# ------------------------------------------------------------------------------------------------- beam search (csrc/beam.hip)
def _beam_arr(what: str, name: str, t: Tensor, dt, shape) -> None:
    if t.dtype is not dt or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise L.LlxError(f"{what}: {name} must be a contiguous device {str(dt).removeprefix('torch.')} {list(shape)} (got {t.dtype} {tuple(t.shape)})")


def beam_rows(logits: Tensor, cand_score: Tensor, cand_token: Tensor) -> None:
    """The shortlist of every row of logits [W, V] (bf16 or fp32, last dim dense, any row stride and start offset; W in 2..16, V > W), in
    one launch: cand_score (fp32 [W, W + 1]) and cand_token (int32 [W, W + 1]) receive the log-probabilities and indices of each row's
    W + 1 best tokens by (logit descending, index ascending) - sampling.beam_shortlist."""
    L.require_cuda(logits, cand_score, cand_token)
    if logits.dim() != 2 or logits.dtype not in (BF16, torch.float32):
        raise L.LlxError(f"beam_rows: logits must be bf16 or fp32 [W, V] (got {logits.dtype} {tuple(logits.shape)})")
    if logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]:
        logits = logits.contiguous()
    W, V = logits.shape
    _beam_arr("beam_rows", "cand_score", cand_score, torch.float32, (W, W + 1))
    _beam_arr("beam_rows", "cand_token", cand_token, torch.int32, (W, W + 1))
    L.check(_lib().llx_beam_rows(L.ptr(logits), 0 if logits.dtype is BF16 else 1, logits.stride(0), W, V, L.ptr(cand_score), L.ptr(cand_token),
                                 L.stream()), "llx_beam_rows")


def beam_merge(cand_score: Tensor, cand_token: Tensor, s: Tensor, parent: Tensor, tok: Tensor, hist: Tensor, bank_tok: Tensor, bank_len: Tensor,
               bank_score: Tensor, meta: Tensor, *, n: int, eos_id: Optional[int] = None, length_penalty: float = 1.0, init: bool = False) -> None:
    """One step of beam search on the shortlists of beam_rows, in one launch and without a host read (sampling.beam_step): the walk over
    the W * (W + 1) candidates and the bookkeeping - parent (int32 [W]), tok (int64 [W] or [W, 1]: the next step's input), s (fp32 [W]),
    hist (int64 [W, n]: permuted by parent, then appended to), the bank of finished hypotheses (bank_tok int64 [W, n], bank_len int32
    [W], bank_score fp32 [W]) and meta (int32 [3]: hypotheses in the bank, done, tokens generated).  init: the first step after the
    prefill (the state is not read; only row 0 takes part).  Once done is set a launch writes identity parents and nothing else."""
    L.require_cuda(cand_score, cand_token, s, parent, tok, hist, bank_tok, bank_len, bank_score, meta)
    W = s.numel()
    for name, t, dt, shape in (("cand_score", cand_score, torch.float32, (W, W + 1)), ("cand_token", cand_token, torch.int32, (W, W + 1)),
                               ("s", s, torch.float32, (W,)), ("parent", parent, torch.int32, (W,)), ("tok", tok.view(-1), torch.int64, (W,)),
                               ("hist", hist, torch.int64, (W, n)), ("bank_tok", bank_tok, torch.int64, (W, n)),
                               ("bank_len", bank_len, torch.int32, (W,)), ("bank_score", bank_score, torch.float32, (W,)),
                               ("meta", meta, torch.int32, (3,))):
        _beam_arr("beam_merge", name, t, dt, shape)
    if not tok.is_contiguous():
        raise L.LlxError("beam_merge: tok must be contiguous")
    L.check(_lib().llx_beam_merge(L.ptr(cand_score), L.ptr(cand_token), L.ptr(s), L.ptr(parent), L.ptr(tok), L.ptr(hist), n, L.ptr(bank_tok), n,
                                  L.ptr(bank_len), L.ptr(bank_score), L.ptr(meta), W, int(n), int(eos_id) if eos_id is not None else -1,
                                  float(length_penalty), 1 if init else 0, L.stream()), "llx_beam_merge")


def kv_cache_table(caches) -> Tensor:
    """The device table of base pointers that kv_reorder_rows takes, for `caches` (bf16 [B, KVH, Smax, 128] tensors of one shape and one
    set of strides, 16-byte aligned: every layer's k and v cache).  Build it once per generate() call; the table keeps the caches' shape
    and strides and references to them.
    FP8 caches (uint8 [B, KVH, Smax, 128], Smax even, contiguous) are addressed as bf16 [B, KVH, Smax / 2, 128]: two positions per
    256-byte row, so llx_kv_reorder_rows moves them unchanged (table.fp8 tells kv_reorder_rows to halve the length)."""
    caches = list(caches)
    fp8 = caches[0].dtype is torch.uint8
    if fp8:
        for c in caches:
            if c.dtype is not torch.uint8 or c.dim() != 4 or c.shape[3] != 128 or c.shape[2] % 2 or not c.is_contiguous():
                raise L.LlxError("kv_cache_table: FP8 caches must be contiguous uint8 [B, KVH, Smax, 128] tensors with an even Smax")
        caches = [c.view(BF16).view(c.shape[0], c.shape[1], c.shape[2] // 2, 128) for c in caches]
    c0 = caches[0]
    for c in caches:
        L.require_cuda(c)
        if c.dtype is not BF16 or c.dim() != 4 or c.shape != c0.shape or c.stride() != c0.stride() or c.stride(3) != 1 or c.data_ptr() % 16:
            raise L.LlxError("kv_cache_table: the caches must be bf16 [B, KVH, Smax, 128] tensors of one shape and one set of strides, "
                             "16-byte aligned, last dim dense")
    table = torch.tensor([c.data_ptr() for c in caches], dtype=torch.int64).to(c0.device)
    table.caches = caches
    table.fp8 = fp8
    return table


def kv_reorder_rows(table: Tensor, parent: Tensor, length: int) -> None:
    """cache[b, :, :length] <- cache[parent[b], :, :length] for b < W = len(parent) (device int32, 2..16) in place, in every cache of
    `table` (kv_cache_table), in one launch.  A thread owns one 16-byte chunk of (head, position) in all W slots, loads the ones that
    move and then stores them, so no slot is read after it was overwritten.  Slots with parent[b] == b, positions >= length and slots
    >= W are not written.
    A table of FP8 caches moves ceil(length / 2) rows of two positions: when `length` is odd the position at index `length` is copied
    along.  That position holds nothing a mask allows yet - the next step's q|k|v epilogue writes it in every slot before any mask
    does - so the extra copy cannot be observed."""
    L.require_cuda(table, parent)
    c0 = table.caches[0]
    if parent.dtype is not torch.int32 or parent.dim() != 1 or not parent.is_contiguous() or parent.numel() > c0.shape[0]:
        raise L.LlxError(f"kv_reorder_rows: parent must be a contiguous device int32 [W] with W <= the caches' batch {c0.shape[0]} "
                         f"(got {parent.dtype} {tuple(parent.shape)})")
    if getattr(table, "fp8", False):
        length = (int(length) + 1) // 2
    L.check(_lib().llx_kv_reorder_rows(L.ptr(table), table.numel(), c0.stride(0), c0.stride(1), c0.stride(2), L.ptr(parent), parent.numel(),
                                       c0.shape[1], int(length), c0.shape[2], c0.shape[3], L.stream()), "llx_kv_reorder_rows")


# ------------------------------------------------------------------------------------------------- cross entropy
def head_compact_index(labels: Tensor) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """(idx, inv, labels_c, count) for the labelled rows (labels != -100) in order; everything stays on the device."""
    L.require_cuda(labels)
    labels = labels.reshape(-1).contiguous()
    assert labels.dtype is torch.int64
    T = labels.numel()
    idx = torch.empty(T, device=labels.device, dtype=torch.int32)
    inv = torch.empty(T, device=labels.device, dtype=torch.int32)
    labels_c = torch.empty(T, device=labels.device, dtype=torch.int64)
    count = torch.empty(1, device=labels.device, dtype=torch.int32)
    L.check(_lib().llx_head_compact_index(L.ptr(labels), L.ptr(idx), L.ptr(inv), L.ptr(labels_c), L.ptr(count), T, L.stream()), "llx_head_compact_index")
    return idx, inv, labels_c, count


def gather_rows(src: Tensor, idx: Tensor, count: Tensor) -> Tensor:
    """dst[j] = src[idx[j]] for j < count (zero rows up to the next multiple of 256, later rows uninitialised)."""
    _chk_bf16(src)
    assert src.dim() == 2 and src.stride(1) == 1 and idx.dtype is torch.int32 and idx.numel() == src.shape[0]
    T, D = src.shape
    dst = torch.empty(T, D, device=src.device, dtype=BF16)
    L.check(_lib().llx_gather_rows(L.ptr(src), src.stride(0), L.ptr(idx), L.ptr(count), L.ptr(dst), D, T, D, L.stream()), "llx_gather_rows")
    return dst


def scatter_rows(src: Tensor, inv: Tensor, dev_scalar: Optional[Tensor] = None) -> Tensor:
    """dst[i] = bf16(dev_scalar * src[inv[i]]) where inv[i] >= 0, zero rows elsewhere."""
    _chk_bf16(src)
    assert src.dim() == 2 and src.stride(1) == 1 and inv.dtype is torch.int32 and inv.numel() == src.shape[0]
    assert dev_scalar is None or (dev_scalar.dtype is torch.float32 and dev_scalar.numel() == 1)
    T, D = src.shape
    dst = torch.empty(T, D, device=src.device, dtype=BF16)
    L.check(_lib().llx_scatter_rows(L.ptr(src), src.stride(0), L.ptr(inv), L.ptr(dev_scalar), L.ptr(dst), D, T, D, L.stream()), "llx_scatter_rows")
    return dst


def ce_fwd_bwd(logits: Tensor, labels: Tensor, write_grad: bool, rows: Optional[Tensor] = None) -> tuple[Tensor, Optional[Tensor]]:
    """Mean CE over labels != -100.  With write_grad the logits buffer is overwritten by d loss / d logits.
    rows (device int32): the rows are compacted (head_compact_index) and only the first `rows` (rounded up to 256) exist."""
    _chk_bf16(logits)
    L.require_cuda(labels)
    lg = _rows2d(logits)
    T, V = lg.shape
    labels = labels.reshape(-1).contiguous()
    assert labels.dtype is torch.int64 and labels.numel() == T
    loss = torch.empty((), device=logits.device, dtype=torch.float32)
    ws = torch.empty(_lib().llx_ce_workspace_bytes(T), device=logits.device, dtype=torch.uint8)
    if rows is not None:
        L.check(_lib().llx_ce_fwd_bwd_rows(L.ptr(lg), lg.stride(0), L.ptr(lg) if write_grad else None, lg.stride(0), L.ptr(labels), L.ptr(loss),
                                           L.ptr(ws), T, V, L.ptr(rows), L.stream()), "llx_ce_fwd_bwd_rows")
    else:
        L.check(_lib().llx_ce_fwd_bwd(L.ptr(lg), lg.stride(0), L.ptr(lg) if write_grad else None, lg.stride(0), L.ptr(labels), L.ptr(loss),
                                      L.ptr(ws), T, V, L.stream()), "llx_ce_fwd_bwd")
    return loss, (lg if write_grad else None)


def ce_chunk(logits: Tensor, labels_all: Tensor, ws: Tensor, loss: Tensor, row0: int, write_grad: bool, rows: Optional[Tensor], first: bool,
             last: bool) -> Optional[Tensor]:
    """One chunk of ce_fwd_bwd over a row set walked in chunks: logits [n, V] are rows row0 .. row0+n of the set, labels_all / ws (float32,
    T + 2) / loss cover the whole set.  Returns the chunk's d loss / d logits (in place) when write_grad."""
    _chk_bf16(logits)
    n, V = logits.shape
    T = labels_all.numel()
    L.check(_lib().llx_ce_fwd_bwd_part(L.ptr(logits), logits.stride(0), L.ptr(logits) if write_grad else None, logits.stride(0), L.ptr(labels_all),
                                       L.ptr(loss), L.ptr(ws), T, V, row0, n, L.ptr(rows), (1 if first else 0) | (2 if last else 0), L.stream()),
            "llx_ce_fwd_bwd_part")
    return logits if write_grad else None


def logprob_rows_fwd(logits: Tensor, labels: Tensor, rows: Optional[Tensor] = None, want_top1: bool = False):
    """Per-row log-probabilities of `labels` under bf16 `logits` [T, V]: (logp, lse, top1), fp32 [T] each with zeros on ignored rows
    (label -100); top1 (None unless want_top1) int32 [T], the row's argmax (lowest index among ties), -1 on ignored rows.  The logits
    are only read.  rows (device int32): compacted rows (head_compact_index), only the first `rows` (rounded up to 256) exist."""
    _chk_bf16(logits)
    L.require_cuda(labels)
    assert logits.dim() == 2 and logits.stride(1) == 1
    T, V = logits.shape
    labels = labels.reshape(-1).contiguous()
    assert labels.dtype is torch.int64 and labels.numel() == T and labels.device == logits.device
    assert rows is None or (rows.dtype is torch.int32 and rows.numel() == 1 and rows.device == logits.device)
    logp = torch.empty(T, device=logits.device, dtype=torch.float32)
    lse = torch.empty(T, device=logits.device, dtype=torch.float32)
    top1 = torch.empty(T, device=logits.device, dtype=torch.int32) if want_top1 else None
    L.check(_lib().llx_logprob_rows_fwd(L.ptr(logits), logits.stride(0), L.ptr(labels), L.ptr(logp), L.ptr(lse), L.ptr(top1), T, V, L.ptr(rows),
                                        L.stream()), "llx_logprob_rows_fwd")
    return logp, lse, top1


def logprob_rows_bwd(logits: Tensor, labels: Tensor, lse: Tensor, g: Tensor, rows: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """d logits = bf16(g[t] * (onehot(label) - softmax(logits[t]))) for the per-row upstream gradient g (fp32 [T]) and the forward's lse;
    zero rows where the label is -100 or g is 0.  Written over `logits` (returned) unless `out` is given.  rows: as logprob_rows_fwd -
    rows at or past `rows` rounded up to 256 are left untouched."""
    _chk_bf16(logits, out)
    L.require_cuda(labels, lse, g)
    assert logits.dim() == 2 and logits.stride(1) == 1
    T, V = logits.shape
    labels = labels.reshape(-1).contiguous()
    assert labels.dtype is torch.int64 and labels.numel() == T and labels.device == logits.device
    assert lse.dtype is torch.float32 and lse.is_contiguous() and lse.numel() == T and lse.device == logits.device
    assert g.dtype is torch.float32 and g.is_contiguous() and g.numel() == T and g.device == logits.device
    assert rows is None or (rows.dtype is torch.int32 and rows.numel() == 1 and rows.device == logits.device)
    if out is None:
        out = logits
    assert out.shape == logits.shape and out.stride(1) == 1 and out.device == logits.device
    L.check(_lib().llx_logprob_rows_bwd(L.ptr(logits), logits.stride(0), L.ptr(out), out.stride(0), L.ptr(labels), L.ptr(lse), L.ptr(g), T, V,
                                        L.ptr(rows), L.stream()), "llx_logprob_rows_bwd")
    return out


def logprob_map_rows(index: Tensor, src: Tensor, fill: float = 0.0, src_i: Optional[Tensor] = None, fill_i: int = 0):
    """dst[i] = src[index[i]] where index[i] >= 0, `fill` elsewhere (index int32 [T], src fp32 [T]); with src_i (int32 [T]) the same for
    it from the same launch -> (dst, dst_i).  The per-row vectors of the compacted head rows back to their positions (index = inv), the
    per-position upstream gradient to the compacted rows (index = idx)."""
    L.require_cuda(index, src, src_i)
    T = index.numel()
    assert index.dtype is torch.int32 and index.is_contiguous() and src.dtype is torch.float32 and src.is_contiguous() and src.numel() == T
    assert src_i is None or (src_i.dtype is torch.int32 and src_i.is_contiguous() and src_i.numel() == T)
    dst = torch.empty_like(src)
    dst_i = torch.empty_like(src_i) if src_i is not None else None
    L.check(_lib().llx_logprob_map_rows(L.ptr(index), L.ptr(src), L.ptr(dst), float(fill), L.ptr(src_i), L.ptr(dst_i), int(fill_i), T, L.stream()),
            "llx_logprob_map_rows")
    return dst, dst_i


TOPK_MAX = 8  # csrc/topk.hip


def topk_logprobs_rows(logits: Tensor, k: int, *, lse: Optional[Tensor] = None, label_logp: Optional[Tensor] = None,
                       labels: Optional[Tensor] = None, rows: Optional[Tensor] = None, pos: Optional[Tensor] = None, hist_base: int = 0,
                       finished: Optional[Tensor] = None, ids: Optional[Tensor] = None, logp: Optional[Tensor] = None):
    """The k (1..TOPK_MAX) largest of every row of bf16 `logits` [R, V] as (ids int32, logp fp32), descending by value, equal values by
    ascending index (the order of csrc/topk.hip: -inf last, a NaN as -inf), ids[:, 0] the top1 of logprob_rows_fwd.  logp = x - lse[r]
    with lse (fp32 [R]), else the kernel forms the row's lse itself; label_logp (fp32 [R], with labels and lse): the alternative that is
    the row's label gets that value.  The logits are only read.
    scoring (labels int64 [R]; rows as logprob_rows_fwd): -> [R, k] each, -1 / 0.0 on rows with label -100 and past the row limit.
    generation (pos int64 [R], hist_base, finished int32 [R] or None; ids / logp given, [R, cap, k] contiguous): row r writes
    [r, pos[r] - hist_base, :] when that column exists and finished[r] is not set; pos and finished are only read.
    neither: -> [R, k] of every row."""
    _chk_bf16(logits)
    L.require_cuda(lse, label_logp, labels, rows, pos, finished, ids, logp)
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= TOPK_MAX:
        raise L.LlxError(f"topk_logprobs_rows: k must be an int in 1..{TOPK_MAX} (got {k!r})")
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise L.LlxError(f"topk_logprobs_rows: logits must be bf16 [R, V] with a dense last dim (got {tuple(logits.shape)})")
    R, V = logits.shape
    dev = logits.device
    for name, t in (("lse", lse), ("label_logp", label_logp)):
        if t is not None and (t.dtype is not torch.float32 or t.shape != (R,) or not t.is_contiguous() or t.device != dev):
            raise L.LlxError(f"topk_logprobs_rows: {name} must be a contiguous fp32 [{R}] on the logits' device")
    for name, t in (("labels", labels), ("pos", pos)):
        if t is not None and (t.dtype is not torch.int64 or t.shape != (R,) or not t.is_contiguous() or t.device != dev):
            raise L.LlxError(f"topk_logprobs_rows: {name} must be a contiguous int64 [{R}] on the logits' device")
    if finished is not None and (finished.dtype is not torch.int32 or finished.shape != (R,) or not finished.is_contiguous() or finished.device != dev):
        raise L.LlxError(f"topk_logprobs_rows: finished must be a contiguous int32 [{R}] on the logits' device")
    assert rows is None or (rows.dtype is torch.int32 and rows.numel() == 1 and rows.device == dev)
    cap = 0
    if pos is not None:
        if ids is None or logp is None:
            raise L.LlxError("topk_logprobs_rows: generation writes into the caller's ids / logp [R, cap, k] buffers")
        if ids.dim() != 3 or ids.shape[0] != R or ids.shape[2] != k or ids.shape[1] < 1:
            raise L.LlxError(f"topk_logprobs_rows: ids / logp must be [{R}, cap, {k}] (got {tuple(ids.shape)})")
        cap = ids.shape[1]
    else:
        if ids is None:
            ids = torch.empty(R, k, device=dev, dtype=torch.int32)
        if logp is None:
            logp = torch.empty(R, k, device=dev, dtype=torch.float32)
        if ids.shape != (R, k):
            raise L.LlxError(f"topk_logprobs_rows: ids / logp must be [{R}, {k}] (got {tuple(ids.shape)})")
    if ids.dtype is not torch.int32 or logp.dtype is not torch.float32 or logp.shape != ids.shape or not ids.is_contiguous() \
            or not logp.is_contiguous() or ids.device != dev or logp.device != dev:
        raise L.LlxError("topk_logprobs_rows: ids must be int32 and logp fp32, of one shape, contiguous, on the logits' device")
    L.check(_lib().llx_topk_logprobs_rows(L.ptr(logits), logits.stride(0) if R > 1 else V, R, V, k, L.ptr(lse), L.ptr(label_logp), L.ptr(labels),
                                          L.ptr(rows), L.ptr(pos), int(hist_base), L.ptr(finished), L.ptr(ids), L.ptr(logp),
                                          cap * k if pos is not None else k, cap, L.stream()), "llx_topk_logprobs_rows")
    return ids, logp


def topk_map_rows(index: Tensor, src_ids: Tensor, src_logp: Tensor):
    """dst[i, :] = src[index[i], :] where index[i] >= 0, (-1, 0.0) elsewhere, for the int32 / fp32 [T, k] pair of topk_logprobs_rows over
    compacted head rows (index = inv of head_compact_index) -> (ids, logp) at the positions."""
    L.require_cuda(index, src_ids, src_logp)
    T = index.numel()
    assert index.dtype is torch.int32 and index.is_contiguous()
    assert src_ids.dtype is torch.int32 and src_ids.dim() == 2 and src_ids.shape[0] == T and src_ids.is_contiguous()
    assert src_logp.dtype is torch.float32 and src_logp.shape == src_ids.shape and src_logp.is_contiguous()
    dst_ids, dst_logp = torch.empty_like(src_ids), torch.empty_like(src_logp)
    L.check(_lib().llx_topk_map_rows(L.ptr(index), L.ptr(src_ids), L.ptr(src_logp), L.ptr(dst_ids), L.ptr(dst_logp), T, src_ids.shape[1], L.stream()),
            "llx_topk_map_rows")
    return dst_ids, dst_logp


# ------------------------------------------------------------------------------------------------- skinny (LoRA)
def skinny_nt(x: Tensor, w: Tensor, kranges: Optional[Sequence[int]] = None, colscale: Optional[Tensor] = None):
    """[M,K] @ [R,K]^T -> [M,64] bf16, zero beyond column R.
    kranges: (lo, hi) x 4, multiples of 64 - rows 16*nb..16*nb+15 of a block-diagonal w are zero outside k in [lo_nb, hi_nb).
    colscale [K] bf16: returns (out, g) with g [M,K] = bf16(x * colscale) written from the same read of x."""
    _chk_bf16(x, w, colscale)
    assert x.dim() == 2 and w.dim() == 2 and x.shape[1] == w.shape[1] and x.stride(1) == 1 and w.stride(1) == 1
    M, K = x.shape
    R = w.shape[0]
    out = torch.empty(M, SK_PAD, device=x.device, dtype=BF16)
    kr = None
    if kranges is not None:
        assert len(kranges) == 8
        kr = (ctypes.c_int32 * 8)(*[int(v) for v in kranges])
    if colscale is not None:
        assert colscale.shape == (K,) and colscale.is_contiguous()
        g = torch.empty(M, K, device=x.device, dtype=BF16)
        L.check(_lib().llx_skinny_nt_scaled(L.ptr(x), x.stride(0), L.ptr(w), w.stride(0), L.ptr(out), M, K, R, kr, L.ptr(colscale), L.ptr(g), K,
                                            L.stream()), "llx_skinny_nt_scaled")
        return out, g
    L.check(_lib().llx_skinny_nt(L.ptr(x), x.stride(0), L.ptr(w), w.stride(0), L.ptr(out), M, K, R, kr, L.stream()), "llx_skinny_nt")
    return out


@dataclass
class TnQueued:
    """One product queued by skinny_tn(..., pending=...): its first stage has run, skinny_tn_flush runs the second."""
    ws: Tensor                      # fp32 split partials the first stage wrote
    out: Tensor
    out_ld: int
    M: int
    N: int
    R: int
    scale: float
    transpose_out: int
    accumulate: int
    segs: Optional[ctypes.Array]    # int32 (n_lo, n_hi, r_lo, r_hi) per member, or None
    n_segs: int
    upart: Optional[Tensor] = None  # column-tile partials of u = y @ u_from^T (skinny_u_reduce sums them)


def skinny_tn(u: Tensor, y: Tensor, R: int, scale_: float, out: Tensor, transpose_out: bool, accumulate: bool = False,
              segs: Optional[Sequence[tuple[int, int, int, int]]] = None, pending: Optional[list] = None,
              u_from: Optional[Tensor] = None, scaled: Optional[tuple[Tensor, Tensor]] = None) -> Tensor:
    """out ([R,N], or [N,R] when transpose_out) (+)= scale * u[:, :R]^T @ y, u [M,64], y [M,N].
    segs: members (n_lo, n_hi, r_lo, r_hi) of a fused group (block-diagonal product): out is then a flat buffer that receives the
    members' [n, r] blocks one after another, each contiguous.
    pending: a list - only the first stage (fp32 split partials) is launched and the second stage is appended to it; ``out`` is valid
    once skinny_tn_flush(pending) has run (one launch for up to 4 products: the adapter gradients of a transformer block).
    u_from (with pending): the batched B^T image [R, N] of the group - the first stage then also emits the column-tile partials of
    y @ u_from^T from the y tiles it stages (y is read once for both products); skinny_u_reduce(pending[-1]) finishes it.
    scaled = (colscale [N] bf16, g [M, N] bf16 output; with u_from): the first stage also writes g = bf16(y * colscale) - the scaled
    gradient an int8 linear's data gradient multiplies (subclasses/int8.py:127)."""
    _chk_bf16(u, y, out)
    M, N = y.shape
    assert u.shape == (M, SK_PAD) and u.is_contiguous() and y.stride(1) == 1 and out.stride(-1) == 1
    sp, ns = None, 0
    if segs is not None:
        ns = len(segs)
        assert 1 <= ns <= 4 and out.is_contiguous() and out.numel() == sum((b - a) * (d - c) for a, b, c, d in segs)
        sp = (ctypes.c_int32 * (4 * ns))(*[int(v) for sgm in segs for v in sgm])
    else:
        assert out.shape == ((N, R) if transpose_out else (R, N))
    ws = torch.empty(_lib().llx_skinny_tn_workspace_bytes(M, N, R), device=y.device, dtype=torch.uint8)
    out_ld = out.stride(0) if out.dim() == 2 else 0
    if pending is None:
        assert u_from is None and scaled is None, "the fused u / scaled-copy outputs need the queued (pending=) form"
        L.check(_lib().llx_skinny_tn(L.ptr(u), L.ptr(y), y.stride(0), L.ptr(out), out_ld, M, N, R, scale_, int(transpose_out), int(accumulate),
                                     L.ptr(ws), sp, ns, L.stream()), "llx_skinny_tn")
        return out
    q = TnQueued(ws, out, out_ld, M, N, R, scale_, int(transpose_out), int(accumulate), sp, ns)
    if u_from is None:
        assert scaled is None
        L.check(_lib().llx_skinny_tn_partial(L.ptr(u), L.ptr(y), y.stride(0), M, N, R, L.ptr(ws), sp, ns, L.stream()), "llx_skinny_tn_partial")
    else:
        assert u_from.dtype is BF16 and u_from.dim() == 2 and u_from.shape == (R, N) and u_from.stride(1) == 1
        q.upart = torch.empty(_lib().llx_skinny_u_workspace_bytes(M, N) // 4, device=y.device, dtype=torch.float32)
        cs = g = None
        if scaled is not None:
            cs, g = scaled
            assert cs.dtype is BF16 and cs.numel() == N and g.shape == (M, N) and g.stride(1) == 1
        one = lambda ctype, v: (ctype * 1)(v)  # the entry point takes arrays: up to 4 products per launch
        ptr = lambda t: one(ctypes.c_void_p, t.data_ptr() if t is not None else None)
        L.check(_lib().llx_skinny_tn_partial_many_us(1, ptr(u), ptr(y), one(ctypes.c_int64, y.stride(0)), one(ctypes.c_int64, M), one(ctypes.c_int64, N),
                                                     one(ctypes.c_int64, R), ptr(ws), one(ctypes.c_void_p, ctypes.cast(sp, ctypes.c_void_p).value if sp is not None else None),
                                                     one(ctypes.c_int, ns), ptr(u_from), one(ctypes.c_int64, u_from.stride(0)), ptr(q.upart), ptr(cs), ptr(g),
                                                     one(ctypes.c_int64, g.stride(0) if g is not None else 0), L.stream()), "llx_skinny_tn_partial_many")
    pending.append(q)
    if len(pending) == 4:
        skinny_tn_flush(pending)
    return out


def skinny_u_reduce(q: TnQueued) -> Tensor:
    """u [M, 64] bf16 (= y @ Bt^T, columns >= R zero) from the column-tile partials the first stage of `q` (a pending item queued with
    u_from) has written; call it right after that skinny_tn (the partial workspace is reused by the next product of the same parity)."""
    assert q.upart is not None, "the product must have been queued with u_from"
    out = torch.empty(q.M, SK_PAD, device=q.upart.device, dtype=BF16)
    L.check(_lib().llx_skinny_u_reduce(L.ptr(q.upart), L.ptr(out), q.M, q.N, q.R, q.segs, q.n_segs, L.stream()), "llx_skinny_u_reduce")
    return out


def skinny_tn_flush(pending: list) -> None:
    """Second stage of every product queued by skinny_tn(..., pending=...) in one launch (at most 4 per launch)."""
    while pending:
        chunk, pending[:] = pending[:4], pending[4:]
        n = len(chunk)
        WS = (ctypes.c_void_p * n)(*[q.ws.data_ptr() for q in chunk])
        OUT = (ctypes.c_void_p * n)(*[q.out.data_ptr() for q in chunk])
        LD = (ctypes.c_int64 * n)(*[q.out_ld for q in chunk])
        MM = (ctypes.c_int64 * n)(*[q.M for q in chunk])
        NN = (ctypes.c_int64 * n)(*[q.N for q in chunk])
        RR = (ctypes.c_int64 * n)(*[q.R for q in chunk])
        SC = (ctypes.c_float * n)(*[q.scale for q in chunk])
        TR = (ctypes.c_int * n)(*[q.transpose_out for q in chunk])
        AC = (ctypes.c_int * n)(*[q.accumulate for q in chunk])
        SG = (ctypes.c_void_p * n)(*[ctypes.cast(q.segs, ctypes.c_void_p).value if q.segs is not None else None for q in chunk])
        NS = (ctypes.c_int * n)(*[q.n_segs for q in chunk])
        L.check(_lib().llx_skinny_tn_reduce_many(n, WS, OUT, LD, MM, NN, RR, SC, TR, AC, SG, NS, L.stream()), "llx_skinny_tn_reduce_many")
