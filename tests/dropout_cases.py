"""Attention dropout on the CPU: the mask function restated, the float64 reference of the dropped forward and backward, and an
emulation of the kernels' rounding points with mutants.

The mask function (csrc/attn_dropout.h) is a pure integer function of (seed, counter, stream_id, b, h, q, k) and the threshold
t = round(p * 65536): a 64-bit key per (seed, counter, stream_id, b, h) from splitmix64's finaliser, then ONE 32-bit word per
element - (key.lo + q * G1) ^ (key.hi + k * G2) through two multiply-xorshift rounds - whose top 16 bits are compared with t.  An
element is dropped iff they are below t, so the realised probability is t / 65536 and a kept element is scaled by
c = 65536 / (65536 - t) (fp32).  `keep_mask` restates it in numpy, independently of the header.

Semantics (SDPA's dropout_p): O = sum_k (P keep c) V with P the ordinary softmax - row maximum, row sum and lse are those of the
undropped row; dV = (P keep c)^T dO, dP = keep c (dO V^T), dS = P (dP - delta) with the UNDROPPED P, delta = rowsum(dO . O) of the
dropped O.  `fwd64` / `bwd64` are that in float64 (delta from the bf16 O the kernel is given, as tests/attn_cases.py:bwd64);
`emulate` restates the kernels' documented rounding points (P keep c rounded to bf16 before P.V, O stored in bf16, bf16 dS) and
takes mutants, so that the bars of the GPU test (the constants of tests/attn_cases.py) can be checked for discriminating power
without a GPU (tests/test_dropout_cases.py)."""
import numpy as np
import torch

from tests import attn_cases as C

HD = C.HD
M64 = (1 << 64) - 1
G1, G2 = 0x9E3779B1, 0x85EBCA77
MUTANTS = ("head_plus_1", "qk_swapped", "bwd_counter_plus_1", "no_scale", "renormalised", "ds_from_dropped_p", "dp_unmasked",
           "one_mask_per_group")


def threshold(p: float) -> int:
    """t = round(p * 2^16)."""
    return int(round(p * 65536))


def scale_c(t: int) -> float:
    """c = 65536 / (65536 - t), in fp32 as the kernels compute it."""
    return float(np.float32(65536.0) / np.float32(65536 - t))


def _mix64(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key_of(seed: int, counter: int, stream_id: int, b: int, h: int) -> tuple[int, int]:
    z = _mix64((seed + 0x9E3779B97F4A7C15 * (counter + 1)) & M64)
    z = _mix64(z ^ ((stream_id << 32) | (b << 16) | h))
    return z & 0xFFFFFFFF, z >> 32


def keep_mask(seed: int, counter: int, stream_id: int, B: int, H: int, Sq: int, Skv: int, t: int) -> np.ndarray:
    """bool [B, H, Sq, Skv]: True where the element is kept."""
    q = np.arange(Sq, dtype=np.uint32)[:, None]
    k = np.arange(Skv, dtype=np.uint32)[None, :]
    out = np.empty((B, H, Sq, Skv), dtype=bool)
    with np.errstate(over="ignore"):
        for b in range(B):
            for h in range(H):
                lo, hi = key_of(seed, counter, stream_id, b, h)
                x = (np.uint32(lo) + q * np.uint32(G1)) ^ (np.uint32(hi) + k * np.uint32(G2))
                x = x ^ (x >> np.uint32(16))
                x = x * np.uint32(0x7FEB352D)
                x = x ^ (x >> np.uint32(15))
                x = x * np.uint32(0x846CA68B)
                out[b, h] = (x >> np.uint32(16)) >= np.uint32(t)
    return out


def keep_tensor(seed, counter, stream_id, B, H, Sq, Skv, t, device=None) -> torch.Tensor:
    m = torch.from_numpy(keep_mask(seed, counter, stream_id, B, H, Sq, Skv, t))
    return m.to(device) if device is not None else m


def _expand(q, k, v):
    g = q.shape[2] // k.shape[2]
    return (q.double().transpose(1, 2), k.double().transpose(1, 2).repeat_interleave(g, dim=1),
            v.double().transpose(1, 2).repeat_interleave(g, dim=1), g)


def fwd64(q, k, v, mask, keep, c: float):
    """o [B,S,H,128] float64 and lse [B,H,S] in nats (of the undropped rows).  keep: bool [B,H,S,S]."""
    qd, kd, vd, _ = _expand(q, k, v)
    s = ((qd @ kd.transpose(-1, -2)) * C.SCALE).masked_fill(~mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    o = (p * keep.double() * c) @ vd
    return o.transpose(1, 2), torch.logsumexp(s, dim=-1)


def bwd64(q, k, v, o, do, mask, keep, c: float):
    """((dq, dk, dv), (rq, rk, rv)): float64 gradients in the layouts of q, k, v with delta = rowsum(dO . o) from the GIVEN o, and
    their rounding scales (tests/attn_cases.py, module docstring)."""
    B, S, H, _ = q.shape
    Skv, KVH = k.shape[1], k.shape[2]
    qd, kd, vd, g = _expand(q, k, v)
    dod, od = do.double().transpose(1, 2), o.double().transpose(1, 2)
    kc = keep.double() * c
    p = torch.softmax(((qd @ kd.transpose(-1, -2)) * C.SCALE).masked_fill(~mask, float("-inf")), dim=-1)
    dp = kc * (dod @ vd.transpose(-1, -2))
    delta = (dod * od).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    ds_abs = ds.abs() + 2.0 ** -12 * p * (dp.abs() + delta.abs())
    pd = p * kc

    def fold(x):
        return x.view(B, KVH, g, Skv, HD).sum(2).transpose(1, 2)

    dq = ((ds @ kd) * C.SCALE).transpose(1, 2)
    rq = ((ds_abs @ kd.abs()) * C.SCALE).transpose(1, 2)
    dk = fold((ds.transpose(-1, -2) @ qd) * C.SCALE)
    rk = fold((ds_abs.transpose(-1, -2) @ qd.abs()) * C.SCALE)
    dv = fold(pd.transpose(-1, -2) @ dod)
    rv = fold(pd.transpose(-1, -2) @ dod.abs())
    return (dq, dk, dv), (rq, rk, rv)


def emulate(q, k, v, do, mask, keep, c: float, *, mutant: str | None = None, keep_next_counter=None):
    """The kernels' documented arithmetic in torch (fp32 where they are fp32): scores in fp32, p = exp2(s log2e / sqrt(d) - m),
    l = rowsum(p) of the UNDROPPED fp32 p, O = bf16((bf16(p keep c) . V) / l), lse = m + log2(l); backward from that bf16 O and
    lse: P = exp2(s - lse), dV from bf16(P keep c), dS = bf16(P (keep c dP - delta)), dQ and dK from it.  Returns
    (o bf16 [B,S,H,128], lse [B,H,S] in log2 units, (dq, dk, dv) fp32 in the layouts of q, k, v).

    mutant: one of MUTANTS - head_plus_1 (every head takes the mask of head h + 1), qk_swapped (keep[k, q]), bwd_counter_plus_1
    (the backward takes `keep_next_counter`), no_scale (c missing), renormalised (l summed over the kept keys only),
    ds_from_dropped_p, dp_unmasked, one_mask_per_group (every head of a GQA group takes the mask of the group's first head)."""
    assert mutant is None or mutant in MUTANTS, mutant
    B, S, H, _ = q.shape
    Skv, KVH = k.shape[1], k.shape[2]
    g = H // KVH
    if mutant == "head_plus_1":
        keep = torch.roll(keep, -1, dims=1)
    elif mutant == "qk_swapped":
        keep = keep.transpose(-1, -2)
    elif mutant == "one_mask_per_group":
        keep = keep[:, (torch.arange(H) // g) * g]
    keep_b = keep_next_counter if mutant == "bwd_counter_plus_1" else keep
    cf = 1.0 if mutant == "no_scale" else c
    kc, kcb = keep.float() * cf, keep_b.float() * cf
    qf = q.float().transpose(1, 2)
    kf = k.float().transpose(1, 2).repeat_interleave(g, dim=1)
    vf = v.float().transpose(1, 2).repeat_interleave(g, dim=1)
    dof = do.float().transpose(1, 2)
    sl2 = C.SCALE * C.LOG2E
    s = (qf @ kf.transpose(-1, -2)).masked_fill(~mask, float("-inf"))
    m = s.amax(-1, keepdim=True) * sl2
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp2(s * sl2 - m)
    l = (p * keep.float() if mutant == "renormalised" else p).sum(-1, keepdim=True)
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    o = (((p * kc).bfloat16().float() @ vf) * inv).bfloat16()
    lse = torch.where(l > 0, m + torch.log2(l), torch.full_like(l, float("-inf")))[..., 0]
    # backward, as the kernels recompute P from the stored lse
    lse_safe = torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse))
    pb = torch.exp2(s * sl2 - lse_safe[..., None])
    dp = dof @ vf.transpose(-1, -2)
    if mutant != "dp_unmasked":
        dp = dp * kcb
    delta = (dof * o.float()).sum(-1, keepdim=True)
    ds = ((pb * kcb if mutant == "ds_from_dropped_p" else pb) * (dp - delta)).bfloat16().float()
    dq = ((ds @ kf) * C.SCALE).transpose(1, 2)
    dk = ((ds.transpose(-1, -2) @ qf) * C.SCALE).view(B, KVH, g, Skv, HD).sum(2).transpose(1, 2)
    dv = ((pb * kcb).bfloat16().float().transpose(-1, -2) @ dof).view(B, KVH, g, Skv, HD).sum(2).transpose(1, 2)
    return o.transpose(1, 2), lse, (dq, dk, dv)


def excess(o, lse_log2, grads, o_ref, lse_ref, ref, rnd) -> dict:
    """How far every checked quantity sits from its bar, as a multiple of the bar (<= 1 passes): the max-norm error of O over
    FWD_O_BAR, (1 - worst row cosine) over (1 - FWD_O_COS), the lse error over LSE_REL, and for dq / dk / dv the ratio of
    attn_cases.bwd_err and (1 - cosine) over (1 - BWD_COS)."""
    out = {"o": C.max_rel(o, o_ref) / C.FWD_O_BAR, "o_cos": (1.0 - C.worst_row_cos(o, o_ref)) / (1.0 - C.FWD_O_COS),
           "lse": C.lse_rel(lse_log2, lse_ref) / C.LSE_REL}
    for name, a, b, r in zip(("dq", "dk", "dv"), grads, ref, rnd):
        ratio, cos = C.bwd_err(a, b, r)
        out[name], out[name + "_cos"] = ratio, (1.0 - cos) / (1.0 - C.BWD_COS)
    return out
