"""Attention inputs at the dynamic range of trained models, and the CPU-side arithmetic that goes with them.

Every family returns seeded bf16 q [B,S,H,128], k / v [B,S,KVH,128] and dO [B,S,H,128] drawn through the oracle's named
generators (oracle.ref.randn), so a case is reproducible from its name alone.  Scores are in nats of the scaled product
s = q.k / sqrt(128):

  unit   q, k, v of std 1: scores of std ~1 nat, flat rows (what the older tests draw)
  diag   local / previous-token heads: key j carries a component along the query of row j (even KV heads) or row j+1 (odd
         KV heads), ~22 nats above the row's typical score - the row maximum sits in the LAST key tile the row visits
  ramp   scores rise with the key index by ~8 nats (11.5 log2 units) per 64 keys: the row maximum grows on every tile
  sink   key 0 sits ~26 nats above every other key (the attention sink of trained Llamas); later tiles add ~e^-20 each
  hot    q and k of std 3.5: scores of std ~12 nats, near one-hot rows
  mixed  within one 32-row wave: rows with a ~22-nat diagonal, rows with a ~10-nat one, plain rows and hot rows; odd KV heads
         also carry a sink; in GQA groups the odd heads of a group are uncoupled hot heads

The forward kernel (csrc/attn_fwd.hip) keeps a DEFERRED running maximum: the base of the exponentials of a 32-row wave moves
only when some row's maximum has grown by more than 8 log2 units over the base (one decision for the whole wave), and only
then are l and O rescaled.  `late_base_moves` counts from the exact scores how often such a move rescales accumulated state,
and `emulate_fwd` restates the kernel's documented arithmetic (with optional mutants) so that the bars of the GPU tests can be
checked for discriminating power on the CPU.
"""
import math

import torch

from oracle import ref as O

HD = 128
SCALE = 1.0 / math.sqrt(HD)
LOG2E = 1.4426950408889634
FAMILIES = ("unit", "diag", "ramp", "sink", "hot", "mixed")

# Bars of the GPU tests (tests/test_attn_range_gpu.py), set from the rounding points the kernels document and checked against the
# emulation below on every family (tests/test_attn_cases.py): P is rounded to bf16 before P.V and O is stored in bf16, each a
# relative 2^-9; the lse is fp32 arithmetic on fp32 scores.
FWD_O_BAR = 1e-2        # max |O - O_ref| / max |O_ref|
FWD_O_COS = 0.9995      # worst per-row cosine of O against O_ref
LSE_REL = 1e-4          # |lse * ln 2 - logsumexp(s)| / max(1, |logsumexp(s)|), per row
# Backward (same bars for every family): the reference is `bwd64`, exact float64 except that delta = rowsum(dO . O) is taken from
# the bf16 O the kernel is given (its first documented rounding point: near one-hot rows make dS = P (dP - delta) cancel, and O's
# 2^-9 rounding then leaves |dO||O| 2^-9 in every dS, however small the true gradient).  The two others, bf16 P (dV) and bf16 dS
# (dQ, dK) as MFMA operands, enter through a rounding scale: max |g - g_ref| <= BWD_BAR max |g_ref| + BWD_RND max |g_rnd|, g_rnd = the
# product over absolute values (dQ: |dS| |K| / sqrt(d), plus 2^-12 of P (|dP| + |delta|) |K| / sqrt(d) for the fp32 cancellation of
# dP - delta).  It matters where the keys share a large component the gradient cancels (ramp) or the true gradient is ~0 (sink).
BWD_BAR = 1e-2          # max-norm part, relative to max |g_ref|
BWD_RND = 2.0 ** -8     # rounding-scale part, relative to max |g_rnd| (two bf16 ulps of the dS / P operands)
BWD_COS = 0.999         # worst per-row cosine, over the rows whose norm is above 1e-3 of the largest and above 2^-3 of their rounding scale
# (a row at 2^-3 of its rounding scale may carry BWD_RND * 8 = 3 % relative error, cos >= 0.9995: below that the rounding allows more
# than the cosine bar; measured on the MI355X, a diag-family dQ row at ~2^-4 of its scale: cos 0.9986 at 0.19 of the max-norm bar)


def _unit(v: torch.Tensor) -> torch.Tensor:
    return v / v.norm(dim=-1, keepdim=True)


def make_case(family: str, B: int, S: int, H: int, KVH: int, tag: str = ""):
    """(q, k, v, do) in bf16 on the CPU for one family; `tag` separates the seeds of different cases."""
    if family not in FAMILIES:
        raise ValueError(family)
    n = f"ac_{family}_{tag}_{B}_{S}_{H}_{KVH}"
    g = H // KVH
    q = O.randn(n + "q", (B, S, H, HD))
    k = O.randn(n + "k", (B, S, KVH, HD))
    v = O.randn(n + "v", (B, S, KVH, HD))
    do = O.randn(n + "do", (B, S, H, HD))
    kv_of = torch.arange(H) // g  # kv head of every query head
    if family == "hot":
        q, k = q * 3.5, k * 3.5
    elif family == "diag":
        qs = O.randn(n + "qs", (B, S, KVH, HD))
        q = qs[:, :, kv_of] + 0.5 * q  # the heads of a group share a query component
        comp = qs.clone()
        comp[:, :-1, 1::2] = qs[:, 1:, 1::2]  # odd KV heads: key j carries query j+1 (a previous-token head)
        comp[:, -1:, 1::2] = 0
        k = k + 2.0 * comp  # diagonal score ~ 2 * 128 / sqrt(128) = 22.6 nats; the rest ~N(0, 2.5^2)
    elif family == "ramp":
        u = _unit(O.randn(n + "u", (KVH, HD)))
        q = q + 4.0 * u[kv_of]
        c = 8.0 / (64 * 4.0 * SCALE)  # slope: 8 nats per 64 keys along u
        k = k + c * torch.arange(S, dtype=torch.float32)[None, :, None, None] * u[None, None]
    elif family == "sink":
        u = _unit(O.randn(n + "u", (KVH, HD)))
        uq = u[kv_of]
        q = q - (q * uq).sum(-1, keepdim=True) * uq + 4.0 * uq  # q.u = 4 exactly
        k[:, 0] = (26.0 / (4.0 * SCALE)) * u  # s(i, 0) = 26 nats for every row
    elif family == "mixed":
        qs = O.randn(n + "qs", (B, S, KVH, HD))
        coupled = (torch.arange(H) % g) % 2 == 0  # in GQA groups: even heads coupled (diagonal), odd heads hot and uncoupled
        q = torch.where(coupled[None, None, :, None], qs[:, :, kv_of] + 0.5 * q, 3.0 * q)
        r32 = torch.arange(S) % 32
        alpha = torch.where(r32 < 12, 2.0, torch.where(r32 < 20, 0.9, 0.0))  # ~22-nat, ~10-nat and no diagonal within one wave
        k = k + alpha[None, :, None, None] * qs
        hot_rows = (r32 >= 26)[None, :, None, None]
        q = torch.where(hot_rows, 2.5 * q, q)
        if KVH > 1:  # odd KV heads also carry a sink at key 0 (~18 nats for the coupled heads)
            u = _unit(O.randn(n + "u", (KVH, HD)))
            sink = torch.zeros(KVH, 1)
            sink[1::2] = 1.0
            k[:, 0] = k[:, 0] + sink * (18.0 / (4.0 * SCALE)) * u
            q = q + 4.0 * (sink[kv_of] * u[kv_of])[None, None]
    return q.bfloat16(), k.bfloat16(), v.bfloat16(), do.bfloat16()


def dense_mask(kind: str, B: int, S: int):
    """(bool mask [B,1,S,S], doc_ids [S] or None, prefix_len [B] or None) for causal / doc / prefix / docprefix: the rule of
    tests/test_kernels_gpu.py:_masks, built from the oracle's prefix_lm_mask / document_mask."""
    idx = torch.arange(S)
    mask = (idx[:, None] >= idx[None, :])[None, None].expand(B, 1, S, S).clone()
    doc = prefix = None
    if "prefix" in kind:
        prefix = torch.tensor(([S // 3, S // 2] * B)[:B], dtype=torch.int32)
        mask = mask | O.prefix_lm_mask(S, prefix)
    if "doc" in kind:
        d = torch.zeros(S, dtype=torch.int32)
        for c in (S // 7, S // 3, S // 2 + 5, (3 * S) // 4):
            d[c:] += 1
        d[S - 37 :] = 0
        doc = d
        mask = mask & (d[:, None] == d[None, :])[None, None]  # the same-document part of the rule (O.document_mask without its causal term)
    return mask, doc, prefix


def scores64(q: torch.Tensor, k: torch.Tensor, mask) -> torch.Tensor:
    """Scaled scores in float64, [B,H,S,Skv], masked entries -inf.  q [B,S,H,128], k [B,Skv,KVH,128]; mask broadcastable."""
    g = q.shape[2] // k.shape[2]
    qd = q.double().transpose(1, 2)
    kd = k.double().transpose(1, 2).repeat_interleave(g, dim=1)
    s = (qd @ kd.transpose(-1, -2)) * SCALE
    return s.masked_fill(~mask, float("-inf"))


def sdpa64(q, k, v, mask):
    """The oracle's SDPA rule (oracle.ref.sdpa) in float64: o [B,S,H,128] and lse [B,H,S] in nats.  Differentiable."""
    g = q.shape[2] // k.shape[2]
    s = scores64(q, k, mask)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.softmax(s, dim=-1)
    o = p @ v.double().transpose(1, 2).repeat_interleave(g, dim=1)
    return o.transpose(1, 2), lse


def bwd64(q, k, v, o, do, mask):
    """Attention backward in float64 with delta = rowsum(dO . o) from the GIVEN o (bf16 from the forward kernel; with the exact o
    this is the autograd gradient).  Returns ((dq, dk, dv), (rq, rk, rv)): the gradients in the layouts of q, k, v and their
    rounding scales (module docstring)."""
    B, S, H, _ = q.shape
    Skv, KVH = k.shape[1], k.shape[2]
    g = H // KVH
    qd = q.double().transpose(1, 2)
    kd = k.double().transpose(1, 2).repeat_interleave(g, dim=1)
    vd = v.double().transpose(1, 2).repeat_interleave(g, dim=1)
    dod, od = do.double().transpose(1, 2), o.double().transpose(1, 2)
    p = torch.softmax(((qd @ kd.transpose(-1, -2)) * SCALE).masked_fill(~mask, float("-inf")), dim=-1)
    dp = dod @ vd.transpose(-1, -2)
    delta = (dod * od).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    ds_abs = ds.abs() + 2.0 ** -12 * p * (dp.abs() + delta.abs())
    del dp

    def fold(x):  # sum the query heads of a group onto their kv head, back to [B, Skv, KVH, 128]
        return x.view(B, KVH, g, Skv, HD).sum(2).transpose(1, 2)

    dq = ((ds @ kd) * SCALE).transpose(1, 2)
    rq = ((ds_abs @ kd.abs()) * SCALE).transpose(1, 2)
    dk = fold((ds.transpose(-1, -2) @ qd) * SCALE)
    rk = fold((ds_abs.transpose(-1, -2) @ qd.abs()) * SCALE)
    dv = fold(p.transpose(-1, -2) @ dod)
    rv = fold(p.transpose(-1, -2) @ dod.abs())
    return (dq, dk, dv), (rq, rk, rv)


def bwd_err(got: torch.Tensor, ref: torch.Tensor, rnd: torch.Tensor) -> tuple[float, float]:
    """(max |got - ref| / (BWD_BAR max |ref| + BWD_RND max |rnd|), worst per-row cosine over the rows that carry signal): the
    first must be <= 1, the second >= BWD_COS."""
    a, b, r = got.double(), ref.double(), rnd.double()
    ratio = ((a - b).abs().max() / (BWD_BAR * b.abs().max() + BWD_RND * r.abs().max()).clamp_min(1e-300)).item()
    a2, b2, r2 = a.reshape(-1, HD), b.reshape(-1, HD), r.reshape(-1, HD)
    nb = b2.norm(dim=1)
    keep = (nb > 1e-3 * nb.max()) & (nb > 2.0 ** -3 * r2.norm(dim=1))
    if not bool(keep.any()):
        return ratio, 1.0
    cos = (a2 * b2).sum(1) / (a2.norm(dim=1) * nb).clamp_min(1e-300)
    return ratio, cos[keep].min().item()


def emulate_bwd(q, k, v, o, do, lse_log2, mask):
    """The backward's documented arithmetic in torch: fp32 scores, P = exp2(s log2e/sqrt(d) - lse), delta = rowsum(dO . O) of the
    bf16 O in fp32, dS = P (dP - delta); dV from bf16 P, dQ and dK from bf16 dS (fp32 accumulation).  Layouts as `bwd64`."""
    B, S, H, _ = q.shape
    Skv, KVH = k.shape[1], k.shape[2]
    g = H // KVH
    qf = q.float().transpose(1, 2)
    kf = k.float().transpose(1, 2).repeat_interleave(g, dim=1)
    vf = v.float().transpose(1, 2).repeat_interleave(g, dim=1)
    dof, of = do.float().transpose(1, 2), o.float().transpose(1, 2)
    s = (qf @ kf.transpose(-1, -2)).masked_fill(~mask, float("-inf"))
    lse = torch.where(torch.isfinite(lse_log2), lse_log2, torch.zeros_like(lse_log2))
    p = torch.exp2(s * (SCALE * LOG2E) - lse[..., None])
    ds = (p * (dof @ vf.transpose(-1, -2) - (dof * of).sum(-1, keepdim=True))).bfloat16().float()
    dq = ((ds @ kf) * SCALE).transpose(1, 2)
    dk = ((ds.transpose(-1, -2) @ qf) * SCALE).view(B, KVH, g, Skv, HD).sum(2).transpose(1, 2)
    dv = (p.bfloat16().float().transpose(-1, -2) @ dof).view(B, KVH, g, Skv, HD).sum(2).transpose(1, 2)
    return dq, dk, dv


def late_base_moves(q, k, mask, tile: int, rows: int = 32, thresh_log2: float = 8.0) -> int:
    """Number of (row block, key tile) steps at which the forward's deferred base moves for a row block that already holds
    accumulated state, i.e. where `l *= alpha` and the O rescale change something (alpha < 1 for a row with l > 0).  The first
    move of a row block (from -inf, alpha = 0 on empty state) is not counted.  From the float64 scores and the mask only."""
    s = scores64(q, k, mask) * LOG2E  # log2 units
    B, H, S, Skv = s.shape
    nrb, nt = -(-S // rows), -(-Skv // tile)
    s = torch.nn.functional.pad(s, (0, nt * tile - Skv, 0, nrb * rows - S), value=float("-inf"))
    tmax = s.view(B, H, nrb, rows, nt, tile).amax(-1)  # [B,H,nrb,rows,nt]
    m = torch.full((B, H, nrb, rows), float("-inf"), dtype=s.dtype)
    count = 0
    for t in range(nt):
        cand = torch.maximum(m, tmax[..., t])
        move = (cand > m + thresh_log2).any(-1)  # one decision per row block
        live = (torch.isfinite(m) & (cand > m)).any(-1)  # some row with accumulated state gets alpha < 1
        count += int((move & live).sum())
        m = torch.where(move[..., None], cand, m)
    return count


def emulate_fwd(q, k, v, mask, *, tile: int = 64, rows: int = 32, thresh_log2: float = 8.0, drop_l_rescale: bool = False,
                drop_o_rescale: bool = False):
    """The forward's documented arithmetic in torch (fp32 where the kernel is fp32): per 32-row wave and key tile, scores in fp32,
    a wave-uniform deferred base (moves only when some row's maximum exceeds the base by > 8 log2 units), p = exp2(s log2e/sqrt(d)
    - base), l += rowsum(p) of the fp32 p, O += bf16(p) . V, then O = bf16(O / l) and lse = base + log2(l) (log2 units).
    drop_l_rescale / drop_o_rescale: the mutants without `l_run *= alpha` / without the O rescale.  Returns (o [B,S,H,128] bf16,
    lse [B,H,S] fp32, log2 units)."""
    B, S, H, _ = q.shape
    Skv, KVH = k.shape[1], k.shape[2]
    g = H // KVH
    nrb, nt = -(-S // rows), -(-Skv // tile)
    Sp, Kp = nrb * rows, nt * tile
    qf = torch.nn.functional.pad(q.float().transpose(1, 2), (0, 0, 0, Sp - S)).view(B, H, nrb, rows, HD)
    kf = torch.nn.functional.pad(k.float().transpose(1, 2).repeat_interleave(g, dim=1), (0, 0, 0, Kp - Skv))
    vf = torch.nn.functional.pad(v.float().transpose(1, 2).repeat_interleave(g, dim=1), (0, 0, 0, Kp - Skv))
    mk = torch.nn.functional.pad(mask.expand(B, H, S, Skv), (0, Kp - Skv, 0, Sp - S), value=False).view(B, H, nrb, rows, Kp)
    sl2 = torch.tensor(SCALE * LOG2E, dtype=torch.float32)
    m = torch.full((B, H, nrb, rows), float("-inf"))
    l = torch.zeros(B, H, nrb, rows)
    o = torch.zeros(B, H, nrb, rows, HD)
    for t in range(nt):
        kt, vt = kf[:, :, None, t * tile : (t + 1) * tile], vf[:, :, None, t * tile : (t + 1) * tile]
        st = (qf @ kt.transpose(-1, -2)).masked_fill(~mk[..., t * tile : (t + 1) * tile], float("-inf"))
        mx = st.amax(-1) * sl2
        cand = torch.maximum(m, mx)
        move = (cand > m + thresh_log2).any(-1, keepdim=True)
        m_new = torch.where(move, cand, m)
        m_safe = torch.where(m_new == float("-inf"), torch.zeros_like(m_new), m_new)
        p = torch.exp2(st * sl2 - m_safe[..., None])
        rs = p.sum(-1)
        alpha = torch.where(move, torch.exp2(m - m_safe), torch.ones_like(m))
        if not drop_l_rescale:
            l = l * alpha
        if not drop_o_rescale:
            o = o * alpha[..., None]
        l = l + rs
        o = o + p.bfloat16().float() @ vt
        m = m_new
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    out = (o * inv[..., None]).bfloat16().view(B, H, Sp, HD)[:, :, :S].transpose(1, 2)
    lse = torch.where(l > 0, m + torch.log2(l), torch.full_like(l, float("-inf"))).view(B, H, Sp)[:, :, :S]
    return out, lse


def max_rel(a: torch.Tensor, b: torch.Tensor) -> float:
    """max |a - b| / max |b| (the `_close` measure of tests/test_model_gpu.py)."""
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def worst_row_cos(a: torch.Tensor, b: torch.Tensor, floor: float = 1e-3) -> float:
    """Worst per-row cosine over the rows (last dim) whose reference norm is above `floor` x the largest (as `_rows_close`)."""
    a2, b2 = a.reshape(-1, a.shape[-1]).double(), b.reshape(-1, b.shape[-1]).double()
    nb = b2.norm(dim=1)
    keep = nb > floor * nb.max()
    cos = (a2 * b2).sum(1) / (a2.norm(dim=1) * nb).clamp_min(1e-30)
    return cos[keep].min().item()


def lse_rel(lse_log2: torch.Tensor, lse_nats: torch.Tensor) -> float:
    """Worst per-row |lse * ln 2 - lse_ref| / max(1, |lse_ref|) (kernel lse in log2 units, reference in nats)."""
    a, b = lse_log2.double() * math.log(2.0), lse_nats.double()
    return ((a - b).abs() / b.abs().clamp_min(1.0)).max().item()
