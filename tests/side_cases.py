"""Cases for the memory-bound side kernels (csrc/rmsnorm.hip, ce.hip, elementwise.hip and the GELU / col2im / weight-reorder kernels of
audio.hip): one per dispatch class, guard, tail and stride the code distinguishes, with float64 references, the bars of the GPU test
(tests/test_side_kernels_gpu.py) and the CPU-side arithmetic that shows each bar reachable and sharp (tests/test_side_cases.py).

Every input is drawn through the oracle's named generators (oracle.ref.randn / uniform / randint): a case is reproducible from its name.

Bars are derived, not measured.  The references are exact float64 restatements of the operation on the bf16 inputs.  One rounding of a
value v to bf16 is wrong by at most 2^-8 |v|, so a result that went through k roundings is held to

    |got - ref| <= k * R1 * |ref| + atol,      R1 = 2^-8 + 2^-16

where the 2^-16 leaves room for the fp32 arithmetic in front of the rounding (a few 2^-24 relative; up to |x| 2^-24 for __expf(x)) and
atol covers fp32 error that is NOT relative to the result - sums whose terms cancel.  Each atol is stated where it is computed.
`ratio()` reports error / bound: <= 1 passes, 10 is ten times outside.  Cross-entropy is the exception (__expf / __logf): it keeps the
bars the kernel has met in tests/test_kernels_gpu.py::test_cross_entropy.

For each kernel there is also an fp32 restatement - the arithmetic a correct kernel performs, rounding where the kernel's comments say
it rounds - and, where a structural error is plausible, mutants of it (a wrong divisor, a dropped chunk, a lost wave, an early add).
"""
import math
from dataclasses import dataclass

import torch

from oracle import ref as O

BF16 = torch.bfloat16
R1 = 2.0 ** -8 + 2.0 ** -16
EPS = 1e-5


def bf(x):
    return x.to(BF16)


def ratio(got, ref, rtol: float, atol=0.0) -> float:
    """Worst |got - ref| / (atol + rtol |ref|) over the elements (0 where both sides agree exactly; inf / nan when the bound is 0 or the
    result is not a number - either fails `<= 1`)."""
    got, ref = got.detach().cpu().double(), ref.double()
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / (rtol * ref.abs() + atol))
    return float(r.max()) if r.numel() else 0.0


# --------------------------------------------------------------------------------------------------------------------------------
# RMSNorm
# --------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class RmsClass:
    """What llx_rmsnorm_{fwd,fwd_quant,bwd} make of a row width: the FULL (guard-free) instantiation or a guarded one, the chunk count
    NCH the registers are sized for, whether the backward runs its two-register-set row pipeline (NCH <= 8), and inside a guarded
    kernel how many 512-wide chunks hold data, how many of the 64 lanes the last of them keeps busy and how many chunks are absent."""
    full: bool
    nch: int
    pipe: bool
    chunks: int
    last_lanes: int
    absent: int


def rms_class(dim: int) -> RmsClass:
    """Pure-Python restatement of the dispatch in csrc/rmsnorm.hip."""
    assert dim % 8 == 0 and 0 < dim <= 8192
    chunks = -(-dim // 512)
    full = dim in (2048, 4096, 8192)
    nch = dim // 512 if full else next(n for n in (1, 2, 4, 8, 16) if chunks <= n)
    return RmsClass(full, nch, nch <= 8, chunks, ((dim - 1) % 512) // 8 + 1, nch - chunks)


RMS_DIMS = {  # dim -> the class it is in the table for
    8: RmsClass(False, 1, True, 1, 1, 0),        # NCH 1, one active lane
    520: RmsClass(False, 2, True, 2, 1, 0),      # NCH 2, second chunk one lane wide
    1536: RmsClass(False, 4, True, 3, 64, 1),    # NCH 4 with one chunk absent
    1792: RmsClass(False, 4, True, 4, 32, 0),    # NCH 4, partial last chunk
    2048: RmsClass(True, 4, True, 4, 64, 0),     # FULL 4
    3072: RmsClass(False, 8, True, 6, 64, 2),    # NCH 8, two chunks absent (Llama-3.2-3B)
    4096: RmsClass(True, 8, True, 8, 64, 0),     # FULL 8
    5120: RmsClass(False, 16, False, 10, 64, 6),  # guarded NCH 16: the single-register-set row loop
    8184: RmsClass(False, 16, False, 16, 63, 0),  # NCH 16, partial last chunk
    8192: RmsClass(True, 16, False, 16, 64, 0),  # FULL 16
}
RMS_FWD_ROWS = (1, 3, 4, 5)  # four rows (waves) per block: a lone wave, a ragged block, a whole one, a second block
RMS_BWD_ROWS_ALL = (1, 2, 5, 9, 13, 16, 17, 37)
RMS_BWD_ROWS = {dim: (RMS_BWD_ROWS_ALL if dim in (3072, 5120) else (5, 37)) for dim in RMS_DIMS}
RMS_BWD_RPB = 16


def rms_bwd_wave_rows(rows: int) -> list:
    """Rows each of the 4 waves of each backward block walks (16 rows per block, wave w takes rows w, w + 4, ...)."""
    out = []
    for r0 in range(0, rows, RMS_BWD_RPB):
        n = min(RMS_BWD_RPB, rows - r0)
        out.append([len(range(w, n, 4)) for w in range(4)])
    return out


def rms_data(dim: int, rows: int) -> dict:
    tag = f"sc_rms_{dim}_{rows}"
    return dict(x=bf(O.randn(tag + "x", (rows, dim))), w=bf(1 + O.randn(tag + "w", (dim,), 0.25)), dy=bf(O.randn(tag + "dy", (rows, dim))),
                dres=bf(O.randn(tag + "r", (rows, dim))))


def rms_ref(d: dict) -> dict:
    """float64: y, rstd, dx (without the residual), dw, and the atol of dx [rows, 1] and dw [dim].
    dx = rstd (g - xhat mean(g xhat)) with g = dy w: the fp32 error of the row mean (a 2^-24-relative error per term of a sum of
    `dim` products of size |g| |xhat|) and of the subtraction is proportional to the LARGEST |g| rstd of the row, not to the element:
    atol_dx = 2^-16 max_row(|dy w| rstd).  dw sums dy xhat over the rows in fp32 (per lane, per wave, per block, then over the
    blocks): atol_dw = 2^-18 sum_rows |dy xhat|."""
    x, w, dy = d["x"].double(), d["w"].double(), d["dy"].double()
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS)
    xhat, g = x * rstd, dy * w
    dx = rstd * (g - xhat * (g * xhat).mean(-1, keepdim=True))
    return dict(y=x * rstd * w, rstd=rstd[:, 0], dx=dx, dw=(dy * xhat).sum(0), atol_dx=2.0 ** -16 * (g.abs() * rstd).amax(-1, keepdim=True),
                atol_dw=2.0 ** -18 * (dy * xhat).abs().sum(0))


RMS_MUTANTS = ("mean_over_nch", "drop_last_chunk", "dw_lost_wave", "dres_before_rounding")


def rms_f32(d: dict, mutant=None) -> dict:
    """The kernels' arithmetic in fp32 with their rounding points: y, dx and dw rounded once, the residual joined as bf16(bf16(dx) + dres).
      mean_over_nch         the row means divide by NCH * 512 instead of dim (invisible in the FULL kernels)
      drop_last_chunk       the last chunk that holds data is neither read nor written (its outputs stay 0)
      dw_lost_wave          wave 3 of every block never adds its rows to dw
      dres_before_rounding  the residual joins the fp32 dx: one rounding instead of two"""
    assert mutant is None or mutant in RMS_MUTANTS
    x, w, dy, dres = (d[k].float() for k in ("x", "w", "dy", "dres"))
    rows, dim = x.shape
    cls = rms_class(dim)
    div = float(cls.nch * 512 if mutant == "mean_over_nch" else dim)
    keep = torch.ones(dim)
    if mutant == "drop_last_chunk":
        keep[(cls.chunks - 1) * 512:] = 0
    rstd = torch.rsqrt((x * x * keep).sum(-1, keepdim=True) / div + EPS)
    y = bf(x * rstd * w * keep)
    xhat = x * rstd
    m = (dy * w * xhat * keep).sum(-1, keepdim=True) / div
    dx0 = rstd * (dy * w - xhat * m) * keep
    dx_res = bf(dx0 + dres) if mutant == "dres_before_rounding" else bf(bf(dx0).float() + dres)
    rsel = torch.ones(rows, 1)
    if mutant == "dw_lost_wave":
        rsel[(torch.arange(rows) % RMS_BWD_RPB) % 4 == 3] = 0
    return dict(y=y, rstd=rstd[:, 0], dx=bf(dx0), dx_res=dx_res * keep.to(BF16), dw=bf((dy * xhat * rsel).sum(0) * keep))


def rms_ratios(got: dict, d: dict, ref: dict) -> dict:
    """error / bound of every RMSNorm output, as the GPU test asserts them (`join`: 0 when dx with dres equals bf16(bf16(dx) + dres)
    bit for bit, inf otherwise)."""
    out = {"y": ratio(got["y"], ref["y"], R1), "rstd": ratio(got["rstd"], ref["rstd"], 2.0 ** -20),
           "dx": ratio(got["dx"], ref["dx"], R1, ref["atol_dx"])}
    if got.get("dw") is not None:
        out["dw"] = ratio(got["dw"], ref["dw"], R1, ref["atol_dw"])
    if got.get("dx_res") is not None:
        out["join"] = 0.0 if torch.equal(got["dx_res"].cpu(), bf(got["dx"].float().cpu() + d["dres"].float())) else math.inf
    return out


# --------------------------------------------------------------------------------------------------------------------------------
# cross-entropy
# --------------------------------------------------------------------------------------------------------------------------------
CE_LOSS_BAR = dict(atol=1e-4, rtol=1e-5)    # test_cross_entropy's, met on hardware
CE_GRAD_BAR = dict(atol=1e-6, rtol=2.0 ** -7)
CE_THREADS = 512


def ce_class(V: int, T: int = 1) -> dict:
    """Restatement of ce_row_kernel's decomposition (512 threads, 8 elements per chunk) and of the single-block count / reduce kernels
    (1024 threads striding over the rows): fewest / most chunks one thread streams, threads without any, passes over the rows."""
    assert V % 8 == 0
    n = V // 8
    return dict(lo=n // CE_THREADS, hi=-(-n // CE_THREADS), idle=max(0, CE_THREADS - n), row_passes=-(-T // 1024))


@dataclass(frozen=True)
class CeCase:
    name: str
    T: int
    V: int
    kind: str = "grid"  # grid | single | all_ignored | range
    want: tuple = ()    # (lo, hi, idle, row_passes) it is in the table for


CE_V = {8: (0, 1, 511), 4088: (0, 1, 1), 4096: (1, 1, 0), 4104: (1, 2, 0), 128256: (31, 32, 0)}
CE_CASES = {c.name: c for c in (
    [CeCase(f"v{V}_t{T}", T, V, "grid", CE_V[V] + (-(-T // 1024),)) for V in (8, 4088, 4096, 4104) for T in (1, 9, 1025)]
    + [CeCase("v128256_t9", 9, 128256, "grid", CE_V[128256] + (1,)),
       CeCase("single", 9, 4104, "single", CE_V[4104] + (1,)),            # one labelled row among ignored ones: 1 / n_valid = 1
       CeCase("all_ignored", 9, 4104, "all_ignored", CE_V[4104] + (1,)),  # 0 / 0: NaN, as F.cross_entropy returns
       CeCase("range", 9, 4104, "range", CE_V[4104] + (1,))])}            # a row at +80, a peaked row with the label on / off the peak
CE_STRIDED = "v4104_t9"  # the case the GPU test also runs as a column view of a [T, V + 64] buffer
PEAK_COL, PEAK = 100, 40.0


def ce_special_labels(V: int) -> list:
    """Labels on the chunk and thread boundaries of the row decomposition: the first and last element of chunk 0, the first of chunk 1,
    the first and last of the last chunk, the last element thread 511 owns in its first chunk and the first of thread 0's second, an
    odd and an even index inside a chunk (the p1 / p0 branches of the gradient pass)."""
    out = []
    for lab in (0, 7, 8, V - 8, V - 1, 4095, 4096, 13, 10):
        if 0 <= lab < V and lab not in out:
            out.append(lab)
    return out


def ce_data(case: CeCase) -> dict:
    T, V = case.T, case.V
    logits = O.randn(f"sc_ce_{case.name}_lg", (T, V), 2.0)
    labels = O.randint(f"sc_ce_{case.name}_lb", (T,), 0, V)
    if case.kind == "grid":
        sp = ce_special_labels(V) if T > 1 else [V - 1]
        k = min(T, len(sp))
        labels[:k] = torch.tensor(sp[:k])
        labels[k::3] = -100  # ignored rows mixed in behind the placed ones
    elif case.kind == "single":
        labels[:] = -100
        labels[4] = 4095
    elif case.kind == "all_ignored":
        labels[:] = -100
    elif case.kind == "range":
        logits[0] += 80.0
        logits[1:3] = O.randn(f"sc_ce_{case.name}_flat", (2, V), 0.25)
        logits[1:3, PEAK_COL] = PEAK
        labels[1], labels[2] = PEAK_COL, PEAK_COL + 1  # losses ~0 and ~40
        labels[5] = -100
    return dict(logits=bf(logits), labels=labels)


def ce_ref(logits, labels) -> dict:
    """float64 logsumexp statement of F.cross_entropy(ignore_index=-100, reduction="mean") and its gradient (zero rows where ignored;
    loss NaN when nothing is labelled)."""
    x = logits.double()
    valid = labels != -100
    n = valid.sum().double()
    lse = torch.logsumexp(x, -1)
    lab = labels.clamp_min(0)
    row = torch.where(valid, lse - x.gather(1, lab[:, None])[:, 0], torch.zeros_like(lse))
    onehot = torch.zeros_like(x).scatter_(1, lab[:, None], 1.0)
    grad = (torch.exp(x - lse[:, None]) - onehot) / n
    grad[~valid] = 0
    return dict(loss=row.sum() / n, grad=grad, row=row)


CE_MUTANTS = ("norm_by_T", "onehot_off_by_one", "skip_last_chunk")


def ce_f32(logits, labels, mutant=None) -> dict:
    """The kernel's arithmetic in fp32 (loss fp32, gradient rounded to bf16 once).
      norm_by_T          1 / T instead of 1 / n_valid (invisible without ignored rows)
      onehot_off_by_one  the -1 of the gradient lands one column to the right
      skip_last_chunk    the last 8 columns of a row are neither summed nor overwritten (the in-place gradient keeps the logits there)"""
    assert mutant is None or mutant in CE_MUTANTS
    x = logits.float()
    T, V = x.shape
    valid = labels != -100
    n = torch.tensor(float(T) if mutant == "norm_by_T" else float(valid.sum()))
    xs = x[:, : V - 8] if (mutant == "skip_last_chunk" and V > 8) else x
    lse = torch.logsumexp(xs, -1)
    lab = labels.clamp_min(0)
    row = torch.where(valid, lse - x.gather(1, lab[:, None])[:, 0], torch.zeros_like(lse))
    hot = (lab + 1) % V if mutant == "onehot_off_by_one" else lab
    grad = (torch.exp(x - lse[:, None]) - torch.zeros_like(x).scatter_(1, hot[:, None], 1.0)) / n
    grad[~valid] = 0
    if mutant == "skip_last_chunk" and V > 8:
        grad[valid, V - 8:] = x[valid, V - 8:]
    return dict(loss=row.sum() / n, grad=bf(grad))


def ce_ratios(got: dict, ref: dict) -> dict:
    """error / bound of loss and gradient; an all-ignored case wants NaN for NaN (ratio 0) and zero gradient rows."""
    if torch.isnan(ref["loss"]):
        loss = 0.0 if torch.isnan(got["loss"].cpu()).item() else math.inf
    else:
        loss = ratio(got["loss"].cpu().reshape(()), ref["loss"], CE_LOSS_BAR["rtol"], CE_LOSS_BAR["atol"])
    return dict(loss=loss, grad=ratio(got["grad"].cpu(), ref["grad"], CE_GRAD_BAR["rtol"], CE_GRAD_BAR["atol"]))


CE_CHUNK = dict(T=700, V=4104, chunk=256, counts=(None, 255, 256, 257, 600))  # the count on, just below and just above a chunk boundary


def ce_chunk_data(count) -> dict:
    """700 rows walked in chunks of 256.  count None: labels with ignored rows mixed in, no device row count.  Otherwise the rows are
    compacted as llx_head_compact_index leaves them: `count` labelled rows first, -100 behind."""
    T, V = CE_CHUNK["T"], CE_CHUNK["V"]
    logits = bf(O.randn("sc_cechunk_lg", (T, V), 2.0))
    labels = O.randint(f"sc_cechunk_lb{count}", (T,), 0, V)
    if count is None:
        labels[5::7] = -100
    else:
        labels[count:] = -100
    return dict(logits=logits, labels=labels)


def ce_rows_limit(count: int) -> int:
    """First row a compacted launch neither reads nor writes: the end of the 256-row GEMM tile that holds the last labelled row."""
    return (count + 255) & ~255


# --------------------------------------------------------------------------------------------------------------------------------
# element-wise glue: one thread per 8 elements, 256 threads per block
# --------------------------------------------------------------------------------------------------------------------------------
def tail_block(threads: int) -> bool:
    """The launch's last block is partly past the end (the `idx >= n` guard fires)."""
    return threads % 256 != 0


def emb_passes(dim: int) -> tuple:
    """(passes of embedding_fwd's 256 threads x 8 elements over a row, lanes busy in the last pass)."""
    assert dim % 8 == 0
    return -(-dim // 2048), ((dim - 1) % 2048) // 8 + 1


EMB_DIMS = {8: (1, 1), 2048: (1, 256), 2056: (2, 1), 4096: (2, 256)}  # one lane; exactly one pass; a second pass one lane wide; two
EMB_BWD = dict(B=2, S=8, dim=520, vocab=24)  # 16 tokens: at most 16 terms per element, so fp32 atomics in ANY order are within 15 * 2^-24
#                                              sum|terms| < 2^-20 sum|terms| of the exact sum


def emb_bwd_ids(kind: str):
    B, S, V = EMB_BWD["B"], EMB_BWD["S"], EMB_BWD["vocab"]
    if kind == "one_id":
        return torch.full((B, S), 5, dtype=torch.int64)  # every token on one row: atomic contention
    assert kind == "distinct"
    return (O.randint("sc_embbwd_first", (1,), 0, V).item() + 5 * torch.arange(B * S)).remainder(V).view(B, S)  # 5 is coprime with 24


def emb_bwd_ref(ids, dy) -> dict:
    D, V = dy.shape[-1], EMB_BWD["vocab"]
    dyd = dy.double().reshape(-1, D)
    ref = torch.zeros(V, D, dtype=torch.float64).index_add_(0, ids.reshape(-1), dyd)
    mag = torch.zeros(V, D, dtype=torch.float64).index_add_(0, ids.reshape(-1), dyd.abs())
    return dict(dt=ref, atol=2.0 ** -20 * mag)


ROPE_CASES = {  # name -> B, S, nheads, row width (columns), batch stride in rows, table rows
    "one_head": (1, 5, 1, 128, 5, 5),            # nheads 1; 80 threads: a lone, partly idle block
    "ragged": (2, 7, 3, 3 * 128, 7, 7),          # B S nheads 16 = 672 threads: not a multiple of 256
    "strided": (3, 9, 2, 5 * 128, 11, 16),       # batch stride > S x row stride, columns beyond nheads * 128, a table longer than S
}


def rope_data(name: str) -> dict:
    B, S, H, W, SB, TS = ROPE_CASES[name]
    buf = bf(O.randn(f"sc_rope_{name}", (B, SB, W)))
    return dict(buf=buf, B=B, S=S, H=H, table=O.rope_table(O.TINY)[3 : 3 + TS].contiguous())  # rows 3..: angles that are not 0


def rope_bwd_ref(g, table) -> dict:
    """float64 transpose of the rotation (rotation by -theta) of g [B, S, H, 128] with the fp32 table; one rounding.  Each output is a
    difference / sum of two fp32 products: atol = 2^-22 (|g0| + |g1|) of its pair."""
    B, S, H, hd = g.shape
    t = table[:S].double().view(1, S, 1, hd // 2, 2)
    gd = g.double().view(B, S, H, hd // 2, 2)
    g0, g1, c, s = gd[..., 0], gd[..., 1], t[..., 0], t[..., 1]
    out = torch.stack([g0 * c + g1 * s, g1 * c - g0 * s], -1).view(B, S, H, hd)
    mag = (g0.abs() + g1.abs()).unsqueeze(-1).expand(B, S, H, hd // 2, 2).reshape(B, S, H, hd)
    return dict(dx=out, atol=2.0 ** -22 * mag)


def rope_bwd_f32(g, table):
    B, S, H, hd = g.shape
    t = table[:S].view(1, S, 1, hd // 2, 2)
    gf = g.float().view(B, S, H, hd // 2, 2)
    g0, g1, c, s = gf[..., 0], gf[..., 1], t[..., 0], t[..., 1]
    return bf(torch.stack([g0 * c + g1 * s, g1 * c - g0 * s], -1).view(B, S, H, hd))


SWIGLU_GATES = (0.0, 1e-3, 1.0, 8.0, 30.0, 90.0)  # and their negatives: saturation both ways, __expf overflow at -90
SWIGLU_SHAPES = {"cols8": (3, 8), "ragged": (37, 520)}  # 3 threads; 37 * 65 = 2405 threads (not a multiple of 256)
SWIGLU_FLOOR = 2.0 ** -120  # where __expf(-g) overflows (g < -88.7) the kernel returns 0 for |silu(g)| < 90 e^-88.7 = 2.7e-37 < 2^-120 * 1


def swiglu_data(name: str) -> dict:
    rows, cols = SWIGLU_SHAPES[name]
    g = O.randn(f"sc_swiglu_{name}_g", (rows, cols), 2.0)
    g.view(-1)[:12] = torch.tensor([s * v for v in SWIGLU_GATES for s in (1.0, -1.0)])
    return dict(g=bf(g), u=bf(O.randn(f"sc_swiglu_{name}_u", (rows, cols))), dh=bf(O.randn(f"sc_swiglu_{name}_dh", (rows, cols))))


def swiglu_ref(d: dict) -> dict:
    """float64 h = silu(g) u, dg = dh u silu'(g), du = dh silu(g), and the atol of each.  The kernel rounds s = bf16(silu(g)) and then
    bf16(s u) / bf16(dh s): k = 2 for h and du; it rounds bf16(dh u) and then the product with silu'(g): k = 2 for dg.  The sigmoid is
    rcp(1 + __expf(-g)): relative error |g| 2^-24 <= 2^-17.5 up to the overflow, inside the 2 * 2^-16 slack of k R1.
    silu'(g) = sg (1 + g (1 - sg)) cancels around its root g = -1.278: fp32 leaves 2^-23 (1 + |g|) sg there, so
    atol_dg = 2^-20 |dh u| sg (1 + |g|).  All three get the overflow floor 2^-120 max(1, |other factor|)."""
    g, u, dh = d["g"].double(), d["u"].double(), d["dh"].double()
    sg = torch.sigmoid(g)
    silu, dsilu = g * sg, sg * (1 + g * (1 - sg))
    one = torch.ones_like(g)
    return dict(h=silu * u, dg=dh * u * dsilu, du=dh * silu, atol_h=SWIGLU_FLOOR * torch.maximum(one, u.abs()),
                atol_du=SWIGLU_FLOOR * torch.maximum(one, dh.abs()),
                atol_dg=2.0 ** -20 * (dh * u).abs() * sg * (1 + g.abs()) + SWIGLU_FLOOR * torch.maximum(one, (dh * u).abs()))


SWIGLU_MUTANTS = ("no_g_term",)


def swiglu_f32(d: dict, mutant=None) -> dict:
    """swiglu_fwd8 / swiglu_bwd8 of csrc/common.h in fp32 with their roundings.  no_g_term: silu'(g) = sg, the g (1 - sg) term lost."""
    g, u, dh = d["g"].float(), d["u"].float(), d["dh"].float()
    sg = 1.0 / (1.0 + torch.exp(-g))
    silu = bf(g * sg).float()
    ds = bf(dh * u).float()
    dsilu = sg if mutant == "no_g_term" else sg * (1.0 + g * (1.0 - sg))
    return dict(h=bf(silu * u), dg=bf(ds * dsilu), du=bf(dh * silu))


def swiglu_ratios(got: dict, ref: dict) -> dict:
    return {k: ratio(got[k], ref[k], 2 * R1, ref["atol_" + k]) for k in ("h", "dg", "du") if got.get(k) is not None}


SCALE_SHAPE = (5, 24)  # 15 threads: the guard of a lone, partly idle block
SCALE_DEV, SCALE_HOST = 0.75, 1.5  # both exact in fp32 (and not 1: a forgotten factor shows)
ADD_SHAPE = (5, 24)


def scale_data() -> dict:
    r, c = SCALE_SHAPE
    return dict(x=bf(O.randn("sc_scale_x", (r, c))), cs=bf(1 + O.randn("sc_scale_cs", (c,), 0.5)))


def scale_ref(d: dict):
    """y = bf16(x * (dev * host) * colscale[c]): one rounding, no cancellation (atol 0)."""
    return d["x"].double() * (SCALE_DEV * SCALE_HOST) * d["cs"].double()


def scale_f32(d: dict):
    return bf(d["x"].float() * (torch.tensor(SCALE_DEV) * SCALE_HOST) * d["cs"].float())


def add_data() -> dict:
    return dict(x=bf(O.randn("sc_add_x", ADD_SHAPE)), y=bf(O.randn("sc_add_y", ADD_SHAPE)))


# --------------------------------------------------------------------------------------------------------------------------------
# audio glue
# --------------------------------------------------------------------------------------------------------------------------------
GELU_SHAPE = (5, 40)  # 25 threads; the GPU test passes rows of a wider buffer (row stride 56)
GELU_LD = 56


def gelu_data() -> dict:
    r, c = GELU_SHAPE
    z = torch.linspace(-6.0, 6.0, r * c - 1)
    z = torch.cat([z, torch.zeros(1)]).view(r, c)  # the grid holds no exact 0 (an even count of points): add one
    return dict(z=bf(z), dy=bf(O.randn("sc_gelu_dy", (r, c))))


def gelu_ref(d: dict) -> dict:
    """float64 y = z Phi(z), dz = dy (Phi(z) + z phi(z)); one rounding each.  1 + erf cancels for negative z: erff is good to a few
    ulp of 1 there, not of the result, which leaves 2^-21 max(1, |z|) absolute on y (8 ulp of 1, times the 0.5 |z| in front) and the same
    times |dy| on dz (its cdf term cancels the same way; z phi(z) <= 0.25 adds less than one ulp of 1)."""
    z, dy = d["z"].double(), d["dy"].double()
    cdf = 0.5 * (1 + torch.erf(z / math.sqrt(2)))
    pdf = torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    a = 2.0 ** -21 * z.abs().clamp_min(1.0)
    return dict(y=z * cdf, dz=dy * (cdf + z * pdf), atol_y=a, atol_dz=a * dy.abs())


def gelu_f32(d: dict) -> dict:
    z, dy = d["z"].float(), d["dy"].float()
    cdf = 0.5 * (1.0 + torch.erf(z * 0.70710678118654752440))
    pdf = 0.3989422804014327 * torch.exp(-0.5 * z * z)
    return dict(y=bf(0.5 * z * (1.0 + torch.erf(z * 0.70710678118654752440))), dz=bf(dy * (cdf + z * pdf)))


def gelu_ratios(got: dict, ref: dict) -> dict:
    return {k: ratio(got[k], ref[k], R1, ref["atol_" + k]) for k in ("y", "dz")}


COL2IM_CASES = {  # name -> M (im2col rows), C, P (padded rows = L + 2), stride
    "s1_odd": (7, 8, 9, 1), "s1_even": (8, 24, 10, 1),  # stride 1: M = L; rows P - 1 (tap 0) ask for row M + 1 >= M
    "s2_odd": (6, 8, 13, 2), "s2_even": (5, 24, 12, 2),  # stride 2: M = (L - 1) // 2 + 1; P odd / even; the last rows ask for row M
    "s2_blocks": (51, 64, 103, 2),                      # the AudioPrefixFn shape (L 101): 824 threads, four blocks, the last ragged
}


def col2im_guard_fires(M: int, P: int, stride: int) -> bool:
    return any((p - kk) >= 0 and (p - kk) % stride == 0 and (p - kk) // stride >= M for p in range(P) for kk in range(3))


def col2im_data(name: str) -> dict:
    M, C, P, stride = COL2IM_CASES[name]
    return dict(dA=bf(O.randn(f"sc_col2im_{name}", (M, 3 * C))), M=M, C=C, P=P, stride=stride)


def col2im_terms(d: dict):
    """[3, P, C] float64: the contribution of tap kk to dpad[p] (zero where the tap has no row)."""
    M, C, P, stride = d["M"], d["C"], d["P"], d["stride"]
    t = torch.zeros(3, P, C, dtype=torch.float64)
    for p in range(P):
        for kk in range(3):
            q = p - kk
            if q >= 0 and q % stride == 0 and q // stride < M:
                t[kk, p] = d["dA"][q // stride, kk * C : (kk + 1) * C].double()
    return t


def col2im_ref(d: dict) -> dict:
    """Sum of at most three bf16 terms in fp32, one rounding: atol = 2^-23 sum|terms| (two fp32 additions)."""
    t = col2im_terms(d)
    return dict(dpad=t.sum(0), atol=2.0 ** -23 * t.abs().sum(0))


def col2im_f32(d: dict):
    t = col2im_terms(d).float()
    return bf(t[0] + t[1] + t[2])


REORDER_SHAPE = (5, 12)  # D, C: C not a multiple of 8; 180 elements, one partly idle block

MEL_LENGTHS = (257, 16077, 16160)  # the shortest length reflect padding allows (both reflections inside one frame); not a multiple of
#                                    the hop (160); a multiple of it
MEL_B = 3


def mel_audio(L: int):
    """Three clips; the last quarter of clip 1 is silent (the 1e-12 clip of log-mel).  Half a clip of silence would put 1 / 6 of the
    frame x bin positions below the `strong` floor of the comparison - more than the tenth allowed - so the silence is a quarter."""
    a = O.uniform(f"sc_mel_{L}", (MEL_B, L), -0.1, 0.1)
    a[1, L - L // 4:] = 0.0
    return a


def mel_strong(ref):
    """test_mel_spectrogram_kernel's mask: positions whose mel energy is above the fp32 noise floor, [B, T, n_mels] of the frames kept."""
    return (ref[..., :-1] > 1e-9 * ref.max()).transpose(1, 2)


PREFIX = dict(B=2, L1=101, L2=51, D=64, C=128, St=5, vocab=32)  # odd feature-frame count: L2 = (L1 - 1) // 2 + 1, the stride-2 conv's last
#                                                                  window ends on the padding row


def prefix_data() -> dict:
    p = PREFIX
    feat = torch.zeros(p["B"], p["L1"] + 2, p["C"])
    feat[:, 1:-1] = O.randn("sc_prefix_feat", (p["B"], p["L1"], p["C"]))
    D, C = p["D"], p["C"]
    return dict(feat=bf(feat), tokens=O.randint("sc_prefix_tok", (p["B"], p["St"]), 0, p["vocab"]), emb=bf(O.randn("sc_prefix_emb", (p["vocab"], D))),
                w1=bf(O.randn("sc_prefix_w1", (D, C, 3), 1 / math.sqrt(3 * C))), b1=bf(O.randn("sc_prefix_b1", (D,), 0.1)),
                w2=bf(O.randn("sc_prefix_w2", (D, D, 3), 1 / math.sqrt(3 * D))), b2=bf(O.randn("sc_prefix_b2", (D,), 0.1)),
                dx=bf(O.randn("sc_prefix_dx", (p["B"], p["L2"] + p["St"], D))))


def prefix_ref(d: dict) -> dict:
    """float64 Conv1d(k3, s1, p1) - GELU - Conv1d(k3, s2, p1) - GELU on the unpadded frames, the token embeddings behind it, and the
    gradients of the four convolution parameters summed over the batch."""
    import torch.nn.functional as F

    ps = {k: d[k].double().requires_grad_() for k in ("w1", "b1", "w2", "b2")}
    f = d["feat"][:, 1:-1].double().transpose(1, 2)  # [B, C, L1]
    h = F.gelu(F.conv1d(f, ps["w1"], ps["b1"], stride=1, padding=1))
    h = F.gelu(F.conv1d(h, ps["w2"], ps["b2"], stride=2, padding=1)).transpose(1, 2)
    x = torch.cat([h, F.embedding(d["tokens"], d["emb"].double())], 1)
    x.backward(d["dx"].double())
    return dict(x=x.detach(), **{"d" + k: v.grad for k, v in ps.items()})


def prefix_f32(d: dict):
    """The audio rows of x as AudioPrefixFn computes them: fp32 convolutions with z1, h1, z2 and x each rounded to bf16."""
    import torch.nn.functional as F

    f = d["feat"][:, 1:-1].float().transpose(1, 2)
    z1 = bf(F.conv1d(f, d["w1"].float(), d["b1"].float(), stride=1, padding=1)).float()
    h1 = bf(F.gelu(z1)).float()
    z2 = bf(F.conv1d(h1, d["w2"].float(), d["b2"].float(), stride=2, padding=1)).float()
    return bf(F.gelu(z2)).transpose(1, 2)


def prefix_x_ratio(x_audio, ref: dict) -> float:
    """error / bound of the audio rows of x: four roundings on the path, |err| <= 4 R1 max|ref| (tests/test_side_kernels_gpu.py)."""
    r = ref["x"][:, : PREFIX["L2"]]
    return ((x_audio.detach().cpu().double() - r).abs().max() / (4 * R1 * r.abs().max())).item()
