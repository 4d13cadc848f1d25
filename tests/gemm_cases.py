"""Cases for the GEMM family (gemm_nt_kernel of csrc/gemm_bf16.hip with its ten epilogues, split-K and its combine, gemm_tn_kernel of
csrc/gemm_tn.hip): one per class of every axis the launcher and the tile loop distinguish, operands on which the kernel's arithmetic has
exactly one correct answer, the float64 reference that computes it, and planted faults - what plausibly wrong kernels would return.
tests/test_gemm_cases.py checks all of this on the CPU, tests/test_gemm_exact_gpu.py runs the table on the GPU with torch.equal as the bar.

Why exact.  The kernels accumulate products in fp32 on the matrix pipe in an order of their own.  With integer-valued bf16 operands in
[-LIM, LIM] (LIM = 15) every product and every partial sum of any subset is an integer below 2^24 (`bound` computes max sum |a||b| from the
data of each case), so the fp32 accumulation is exact in ANY order and the rounding points that follow are fully determined:

    bf16 NT          v = bf16(S + S2)                                   S = a . b^T, S2 = a2 . b2^T (same accumulators, one sum)
    int8, bf16 scales v = bf16(((float)S * sa[m]) * sb[n])              two fp32 multiplies, restated with fp32 torch ops; int8 entries use
                                                                         the full range [-127, 127], scales are arbitrary bf16 values
    int8, f32 scales  v = ((float)S * sa[m]) * sb[n]                    the unrounded fp32 value
    int8 + extension  v = bf16(bf16(S sa[m] sb[n]) + S2)                entries in [-15, 15], sa in {1/2, 1/4, 1/8} per row, sb in {1/2, 1/4} per
                                                                         column: everything is a multiple of 2^-5 (the quantum of `bound`)
    none              out = v
    residual, bias    out = bf16(v + e)                                 e integers in [-128, 128] (exact in bf16)
    colscale          out = bf16(v * e[n])                              e bf16 in [0.5, 2]: bf16 x bf16 is exact in fp32
    bias + GELU       z = bf16(v + e) exact; out within one bf16 neighbour of bf16(gelu_float64(z))
    RoPE              (y0, y1) = (x0 c - x1 s, x1 c + x0 s) per pair of v with table row m % rope_S, rounded once, columns < rope_cols; the
                      fp32 table is synthetic, (c, s) from ROPE_PAIRS per (position, pair): every product is exact, contraction cannot matter
    SwiGLU forward    gate|up = v bit for bit; h = the stand-alone swiglu_fwd kernel on those exact halves
    SwiGLU backward   dg|du = the stand-alone swiglu_bwd kernel on dh = v and the gate|up operand
    split-K           out = bf16(S), with a scale bf16(scale * bf16(S)) (scale 0.375: the product is exact in fp32), row i = product row
                      inv[i], zeros where inv[i] < 0
    TN                out = bf16(a[:m]^T . b[:m]), m = min(M, max(m_valid, 0)); +0 everywhere for m = 0

Dispatch, re-derived from launch_gemm / gemm_nt_kernel (`dispatch`): grid_m = ceil(M / 256), grid_n = ceil(N / 256) (SwiGLU forward:
N / 256 tiles of 128 gate + 128 up columns); nk1 = K / TK / splits main K-tiles (TK = 64 bf16 | 128 int8) of which the first nk1 - 2 run
the guard-free steady loop, then K2 / 64 extension tiles; with tiles = grid_m grid_n > 256, N % 256 == 0 and tail = tiles % 256 in
[1, 128] a multiple of grid_m, the last tail / grid_m * 256 columns are relaunched with 256 x 128 half tiles.
"""
import functools
import math
from dataclasses import dataclass
from typing import Optional

import torch

from oracle import ref as O

BF16 = torch.bfloat16
LIM = 15                      # operand entries are integers in [-LIM, LIM]; the premise (exact accumulation on the pipe) holds at 15
SENT16 = 0x5A5A               # bit pattern every output buffer is prefilled with (bf16 1.5e16; int32 0x5A5A5A5A for fp32 outputs)
SK_SCALE = 0.375
ROPE_S = 100
ROPE_PAIRS = ((1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (0.5, 0.5), (-0.5, 0.5), (0.5, -0.5))
EPI_CODE = {"none": 0, "res": 1, "bias": 2, "gelu": 3, "colscale": 4, "swiglu_bwd": 6, "swiglu_fwd": 7, "rope": 8}


# ------------------------------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    id: str
    cls: str                        # the class the GPU test is parametrised by
    kind: str                       # bf16 | i8 (bf16 scales) | i8f32 | splitk
    M: int
    N: int
    K: int
    K2: int = 0
    epi: str = "none"
    layout: str = ""                # "" | "s1" | "s2": the strided forms (`strides`)
    m_valid: Optional[int] = None
    rope_cols: int = 0
    splits: int = 1
    inv: bool = False
    scale: bool = False

    @property
    def ext(self):                  # the int8 entry point with the K-extension, epilogues and in-place dequantisation
        return self.kind == "i8" and (self.K2 > 0 or self.epi != "none")

    @property
    def tk(self):
        return 128 if self.kind in ("i8", "i8f32") else 64


@dataclass(frozen=True)
class TnCase:
    id: str
    cls: str
    M: int                          # contraction length (token rows)
    N1: int
    N2: int
    form: str = ""                  # "" | "slice" (columns of a wider buffer) | "im2col" (rows overlap: row stride 88 < N1)
    m_valid: Optional[int] = None

    @property
    def m_eff(self):
        return self.M if self.m_valid is None else min(self.M, max(self.m_valid, 0))


HALF = (129, 65792)                 # 257 tiles: tail 1, the last 256 columns go as two half tiles
TN_PAIRS = ((8, 8), (248, 264), (256, 256), (264, 520), (520, 8))


def _nt_cases():
    cs = []

    def add(cls, kind, M, N, K, K2=0, epi="none", **kw):
        tag = "".join(f"-{k}{v}" for k, v in kw.items() if v not in (None, False, "", 0))
        cs.append(Case(f"{cls}-{kind}-{M}x{N}x{K}+{K2}-{epi}{tag}", cls, kind, M, N, K, K2, epi, **kw))

    for K, K2 in ((64, 0), (128, 0), (192, 0), (256, 0), (320, 0), (64, 64), (64, 128), (128, 64), (192, 64), (128, 256), (320, 128)):
        add("loop", "bf16", 257, 264, K, K2)
    for K, K2 in ((128, 0), (256, 0), (384, 0), (512, 0), (640, 0), (128, 64), (256, 64), (384, 128), (640, 128)):
        add("loop", "i8", 257, 264, K, K2)
    for K in (128, 384, 640):
        add("loop", "i8f32", 257, 264, K)
    for M in (1, 17, 64, 129, 255, 256, 257, 520, 1100):
        add("rows", "bf16", M, 520, 128, 64)
    for M in (1, 257, 1100):
        add("rows", "i8", M, 520, 128, 64)
        add("rows", "i8f32", M, 520, 128)
    for N in (8, 120, 128, 136, 248, 256, 264, 520, 776):
        for epi in ("none", "res", "bias"):
            add("cols", "bf16", 129, N, 128, 0, epi)
    for N in (8, 264, 776):
        add("cols", "i8", 129, N, 128, 0)
        add("cols", "i8", 129, N, 128, 64, "res")
        add("cols", "i8f32", 129, N, 128)
    for lay in ("s1", "s2"):
        add("strides", "bf16", 257, 264, 128, 64, "none", layout=lay)
        add("strides", "bf16", 257, 264, 128, 64, "res", layout=lay)
        add("strides", "bf16", 257, 264, 128, 64, "swiglu_bwd", layout=lay)
        add("strides", "i8", 257, 264, 256, 64, "res", layout=lay)
        add("strides", "i8", 257, 264, 256, 0, layout=lay)
        add("strides", "i8f32", 257, 264, 256, layout=lay)
    # every epilogue of the three entry points at a whole tile, at ragged edges (and, below, on the half-tile shape)
    for M, N in ((256, 256), (257, 264)):
        for epi in ("none", "res", "bias", "colscale", "swiglu_bwd"):
            add("epilogue", "bf16", M, N, 192, 64, epi)
        add("gelu", "bf16", M, N, 192, 64, "gelu")
        add("epilogue", "bf16", M, N, 192, 64, "rope", rope_cols=128 if N == 256 else 256)
        for K2 in (0, 64):
            for epi in ("none", "res"):
                add("epilogue", "i8", M, N, 256, K2, epi)
            add("epilogue", "i8", M, N, 256, K2, "rope", rope_cols=128 if N == 256 else 256)
    for M, N in ((256, 512), (257, 768)):
        add("epilogue", "bf16", M, N, 192, 64, "swiglu_fwd")
        for K2 in (0, 64):
            add("epilogue", "i8", M, N, 256, K2, "swiglu_fwd")
    # the launcher's tail split
    add("tail", "bf16", 17, 98304, 64)       # tail 128: split
    add("tail", "bf16", 17, 98560, 64)       # tail 129: one launch
    add("tail", "bf16", 300, 33024, 64)      # grid_m 2, tail 2: split
    add("tail", "bf16", 520, 22016, 64)      # grid_m 3, tail 2: no multiple of grid_m, one launch
    add("tail", "bf16", 129, 65800, 64)      # N % 256 != 0: one launch
    hm, hn = HALF
    add("tail", "bf16", hm, hn, 64, 64)
    for epi in ("none", "res", "bias", "colscale", "swiglu_bwd"):
        add("tail", "bf16", hm, hn, 64, 0, epi)
    add("gelu", "bf16", hm, hn, 64, 0, "gelu")
    add("tail", "bf16", hm, hn, 64, 0, "rope", rope_cols=65536 + 128)   # the boundary falls between the two half tiles
    add("tail", "i8", hm, hn, 128, 0)
    add("tail", "i8", hm, hn, 128, 64)
    add("tail", "i8", hm, hn, 128, 0, "res")
    add("tail", "i8", hm, hn, 128, 64, "rope", rope_cols=65536 + 128)
    add("tail", "i8f32", hm, hn, 128)
    for mv in (0, 1, 255, 256, 257, 700, 707):
        add("rowlimit", "bf16", 700, 264, 128, 64, "res", m_valid=mv)
    cs.append(Case("rowlimit-bf16-300x33024x64-mv100", "rowlimit", "bf16", 300, 33024, 64, m_valid=100))   # a split launch whose row grid shrinks
    for M, N, K, s in ((64, 8, 64, 1), (257, 264, 256, 2), (129, 520, 576, 3), (300, 136, 640, 2), (257, 264, 1024, 16)):
        for inv, scale, mv in ((False, False, None), (True, False, None), (False, True, None), (True, True, None), (True, True, (M + 1) // 2)):
            add("splitk", "splitk", M, N, K, splits=s, inv=inv, scale=scale, m_valid=mv)
    return cs


def _tn_cases():
    cs = []
    for M in (1, 8, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200):
        for n1, n2 in TN_PAIRS:
            cs.append(TnCase(f"tn-{M}x{n1}x{n2}", "tn", M, n1, n2))
    for form in ("slice", "im2col"):
        for n1, n2 in ((248, 264), (264, 520)):
            cs.append(TnCase(f"tn-200x{n1}x{n2}-{form}", "tn-strided", 200, n1, n2, form))
    for mv in (-3, 0, 1, 63, 64, 65, 200, 250):
        cs.append(TnCase(f"tn-200x264x520-mv{mv}", "tn-rowlimit", 200, 264, 520, "", mv))
    return cs


CASES = _nt_cases()
TN_CASES = _tn_cases()
BY_ID = {c.id: c for c in CASES + TN_CASES}
assert len(BY_ID) == len(CASES) + len(TN_CASES)


def strides(c: Case) -> dict:
    """Row strides (elements) of every buffer of the case; every base pointer sits 16 bytes into its allocation.  The default already pads
    every row (8 elements, 16 for int8); "s1" takes a2 from columns [64:128] of an [M, 192] buffer with ldb2 = 72, "s2" widens lda and ldc."""
    pad = 16 if c.tk == 128 else 8
    wide = 2 * c.N if c.epi == "swiglu_bwd" else c.N
    s = dict(lda=c.K + pad, ldb=c.K + pad, ldc=wide + 8, lde=wide + 8, lda2=c.K2 + 8, ldb2=c.K2 + 8, a2_col0=0)
    if c.epi == "swiglu_fwd":
        s["lde"] = c.N // 2 + 8
    if c.layout == "s1":
        assert c.K2 in (0, 64)
        s.update(lda2=192, a2_col0=64, ldb2=72)
    elif c.layout == "s2":
        s.update(lda=c.K + (80 if c.tk == 128 else 72), ldc=wide + 264)
        if c.epi == "swiglu_bwd":
            s["lde"] = s["ldc"]
    return s


# ------------------------------------------------------------------------------------------------------------------------ dispatch
def dispatch(c: Case) -> tuple:
    """(grid_m, grid_n, nk1, next, split?, tail_cols) as launch_gemm and gemm_nt_kernel derive them (grid_m before a row limit shrinks it)."""
    gm = -(-c.M // 256)
    gn = c.N // 256 if c.epi == "swiglu_fwd" else -(-c.N // 256)
    nk1, nxt = c.K // c.tk // c.splits, c.K2 // 64
    tiles = gm * gn
    tail = tiles % 256
    split = (c.kind != "splitk" and c.epi != "swiglu_fwd" and c.N % 256 == 0 and tiles > 256 and 0 < tail <= 128 and tail % gm == 0)
    return gm, gn, nk1, nxt, split, (tail // gm * 256 if split else 0)


def classes(c) -> set:
    """The dispatch classes a case exercises, from the restatement alone (the coverage table of tests/test_gemm_cases.py)."""
    if isinstance(c, TnCase):
        m = c.m_eff
        t = {"tn:" + ("empty" if m == 0 else "lt64" if m < 64 else "eq64" if m == 64 else "multi" if m % 64 == 0 else "ragged" if m > 64 else "")}
        t.add(f"tn:grid{-(-c.N1 // 256)}x{-(-c.N2 // 256)}")
        if c.form:
            t.add("tn:" + c.form)
        if c.m_valid is not None:
            t.add("tn:mv<=0" if c.m_valid <= 0 else "tn:mv>M" if c.m_valid > c.M else "tn:mv")
        return t
    gm, gn, nk1, nxt, split, tail_cols = dispatch(c)
    steady = max(nk1 - 2, 0)
    t = {f"{c.kind}:{c.epi}", f"{c.kind}:steady{min(steady, 2)}", f"{c.kind}:exit_stage{steady & 1}", f"{c.kind}:ext{nxt}"}
    if nk1 <= 3:
        t.add(f"{c.kind}:nk{nk1}" + ("+ext" if nxt else ""))
    if c.kind == "splitk":
        t.add(f"splitk:tiles_per_range{min(nk1, 3)}")
        t.add("splitk:" + "+".join(n for n, on in (("inv", c.inv), ("scale", c.scale), ("mv", c.m_valid is not None)) if on) if (c.inv or c.scale) else "splitk:plain")
    if split:
        t |= {f"{c.kind}:{c.epi}:half", f"half:grid_m{gm}", f"half:tail{(gm * gn) % 256}"}
        if c.M % 256:
            t.add("half:ragged_rows")
        if c.K2:
            t.add(f"{c.kind}:half+ext")
        if c.rope_cols and c.N - tail_cols < c.rope_cols < c.N:
            t.add("half:rope_boundary_inside")
    elif gm * gn > 256:
        tail = (gm * gn) % 256
        t.add("nosplit:" + ("ragged_n" if c.N % 256 else "tail>128" if tail > 128 else "tail%grid_m" if tail % gm else "other"))
    if gm == 5:
        t.add("rows:group4+1")
    if gm * gn * c.splits > 8 and (gm * gn * c.splits) % 8:
        t.add("xcd:remainder")
    t.add("rows:" + ("lt_tile" if c.M < 256 else "whole" if c.M % 256 == 0 else "ragged"))
    t.add("cols:" + ("lt_half" if c.N < 128 else "lt_tile" if c.N < 256 else "whole" if c.N % 256 == 0 else "ragged"))
    if c.layout:
        t.add(f"{c.kind}:strided")
    if c.m_valid is not None and c.kind != "splitk":
        mv = c.m_valid
        t.add("mv:" + ("zero" if mv == 0 else "gt_M" if mv > c.M else "eq_M" if mv == c.M else "tile_edge" if mv % 256 == 0 else "inside"))
        if split and -(-mv // 256) < gm:
            t.add("mv:split_grid_shrinks")
    return t


# ------------------------------------------------------------------------------------------------------------------------ operands
def _ints(name, shape, lim=LIM):
    return O.randint("gemm." + name, shape, -lim, lim + 1).double()


@functools.lru_cache(maxsize=8)
def operands(kind: str, M: int, N: int, K: int, K2: int, ext: bool = False) -> dict:
    """The dense operands of a shape as float64 (exact small values); named by shape, so that the epilogue variants of a shape share them."""
    i8 = kind in ("i8", "i8f32")
    lim = 127 if (i8 and not ext) else LIM
    t = f"{'i' if i8 else 'b'}{lim}"
    d = dict(a=_ints(f"a.{t}.{M}x{K}", (M, K), lim), b=_ints(f"b.{t}.{N}x{K}", (N, K), lim))
    if K2:
        d["a2"], d["b2"] = _ints(f"a2.{M}x{K2}", (M, K2)), _ints(f"b2.{N}x{K2}", (N, K2))
    if i8 and ext:
        d["sa"] = 2.0 ** -O.randint(f"gemm.sa.{M}", (M,), 1, 4).double()
        d["sb"] = 2.0 ** -O.randint(f"gemm.sb.{N}", (N,), 1, 3).double()
    elif i8:
        sa, sb = O.uniform(f"gemm.sa.{M}", (M,), 0.001, 0.01), O.uniform(f"gemm.sb.{N}", (N,), 0.001, 0.01)
        if kind == "i8":
            sa, sb = sa.bfloat16().float(), sb.bfloat16().float()
        d["sa"], d["sb"] = sa.double(), sb.double()
    return d


def _ops(c: Case) -> dict:
    return operands(c.kind, c.M, c.N, c.K, c.K2, c.ext)


def epi_operand(c: Case) -> Optional[torch.Tensor]:
    """The epilogue operand as float64 of bf16-exact values: residual [M, N] / bias [N] integers in [-128, 128], colscale [N] in [0.5, 2],
    gate|up [M, 2N] in [-4, 4] for the SwiGLU backward."""
    if c.epi == "res":
        return _ints(f"res.{c.M}x{c.N}", (c.M, c.N), 128)
    if c.epi in ("bias", "gelu"):
        return _ints(f"bias.{c.N}", (c.N,), 128)
    if c.epi == "colscale":
        return O.uniform(f"gemm.colscale.{c.N}", (c.N,), 0.5, 2.0).bfloat16().double()
    if c.epi == "swiglu_bwd":
        return O.uniform(f"gemm.gu.{c.M}x{c.N}", (c.M, 2 * c.N), -4.0, 4.0).bfloat16().double()
    return None


def rope_table() -> torch.Tensor:
    """fp32 [ROPE_S, 64, 2]: (cos, sin) of every (position, pair) drawn from ROPE_PAIRS."""
    pick = O.randint("gemm.rope", (ROPE_S, 64), 0, len(ROPE_PAIRS))
    return torch.tensor(ROPE_PAIRS, dtype=torch.float32)[pick]


def sk_inv(c: Case) -> torch.Tensor:
    """Split-K output row -> product row: a permutation of the rows that exist (all, or the first m_valid) with every fifth row -1."""
    rows = c.M if c.m_valid is None else c.m_valid
    g = torch.Generator().manual_seed(c.M * 131 + c.N)
    inv = torch.randperm(rows, generator=g)[torch.arange(c.M) % rows].to(torch.int32)
    inv[torch.arange(c.M) % 5 == 3] = -1
    return inv


def tn_operands(c: TnCase):
    return _ints(f"tn.a.{c.M}x{c.N1}.{c.form}", (c.M, c.N1)), _ints(f"tn.b.{c.M}x{c.N2}.{c.form}", (c.M, c.N2))


def tn_im2col_source(c: TnCase, which: str):
    """The overlapping form: a 1-D source x with a[m, j] = x[88 m + j] (rows overlap: 88 < N1).  Returns (x, the [M, N] view of it)."""
    n = c.N1 if which == "a" else c.N2
    x = _ints(f"tn.x{which}.{c.M}x{n}", ((c.M - 1) * 88 + n,))
    return x, x.as_strided((c.M, n), (88, 1))


def tn_dense(c: TnCase):
    if c.form == "im2col":
        return tn_im2col_source(c, "a")[1].clone(), tn_im2col_source(c, "b")[1].clone()
    return tn_operands(c)


# ------------------------------------------------------------------------------------------------------------------------ roundings
def rnd(x: torch.Tensor, mode: str = "rne", exact: bool = True) -> torch.Tensor:
    """fp32 -> bf16.  A float64 argument is the exact value of an fp32 quantity: it must be representable in fp32 (`exact`, asserted).
    mode: rne (round to nearest even: f2bf of csrc/common.h:49) | trunc | away (ties away from zero): the planted converts."""
    if x.dtype is torch.float64:
        f = x.float()
        assert not exact or torch.equal(f.double(), x), "the value at a rounding point is not representable in fp32"
        x = f
    if mode == "rne":
        return x.bfloat16()
    bits = x.contiguous().view(torch.int32)
    bits = (bits if mode == "trunc" else bits + 0x8000) & -65536
    return bits.view(torch.float32).bfloat16()


def gelu64(z: torch.Tensor) -> torch.Tensor:
    """z Phi(z) in float64, through erfc so that the negative tail keeps its relative accuracy."""
    return z * 0.5 * torch.special.erfc(-z / math.sqrt(2.0))


# ------------------------------------------------------------------------------------------------------------------------ products
@functools.lru_cache(maxsize=6)
def _product(kind, M, N, K, K2, ext):
    d = operands(kind, M, N, K, K2, ext)
    S = d["a"] @ d["b"].T + 0.0  # the accumulators start at +0: a sum of zero products is +0 whatever their signs
    S2 = d["a2"] @ d["b2"].T + 0.0 if K2 else None
    return S, S2


@functools.lru_cache(maxsize=6)
def _abs_product(kind, M, N, K, K2, ext):
    d = operands(kind, M, N, K, K2, ext)
    S = d["a"].abs() @ d["b"].abs().T
    S2 = d["a2"].abs() @ d["b2"].abs().T if K2 else None
    return S, S2


def quantum(c) -> float:
    return 2.0 ** -5 if (isinstance(c, Case) and c.ext) else 1.0


def bound(c) -> float:
    """max over the outputs of sum |a||b| in quanta: below 2^24 every partial sum of any order is exact in fp32."""
    if isinstance(c, TnCase):
        a, b = tn_dense(c)
        return float((a.abs().T @ b.abs()).max())
    S, S2 = _abs_product(c.kind, c.M, c.N, c.K, c.K2, c.ext)
    if c.ext:
        d = _ops(c)
        S = S * d["sa"][:, None] * d["sb"][None, :]
    if S2 is not None:
        S = S + S2
    return float(S.max()) / quantum(c)


def _tile(c: Case, which: str):
    """The contribution of one K-tile: first | last (main operands) | last_ext."""
    d = _ops(c)
    if which == "last_ext":
        return d["a2"][:, -64:] @ d["b2"][:, -64:].T
    sl = slice(0, c.tk) if which == "first" else slice(c.K - c.tk, c.K)
    return d["a"][:, sl] @ d["b"][:, sl].T


MUTANTS = ("trunc", "away", "drop_first", "drop_last", "drop_last_ext", "drop_ext", "single_res", "single_colscale", "single_i8ext",
           "scale_order", "scale_local", "clamp_chunk", "single_splitk")


def live(c, mutant: str) -> bool:
    """Whether the class of the planted fault exists in the case."""
    if isinstance(c, TnCase):
        return c.m_eff > 0 and mutant in ("trunc", "away", "drop_first", "drop_last")
    if c.m_valid == 0:
        return False
    i8 = c.kind in ("i8", "i8f32")
    return {
        "trunc": c.kind != "i8f32", "away": c.kind != "i8f32" and not (c.kind == "i8" and not c.ext),  # arbitrary scales make no ties
        "drop_first": True, "drop_last": True, "drop_last_ext": c.K2 > 0, "drop_ext": c.K2 > 0,
        "single_res": c.epi in ("res", "bias"), "single_colscale": c.epi == "colscale", "single_i8ext": c.ext and c.K2 > 0,
        # the two fp32 multiplies in the other order differ in the last place of fp32: the unrounded f32 entry shows it everywhere, a bf16
        # output only where that place straddles a bf16 boundary (about 2^-16 of the outputs) - not claimed
        "scale_order": c.kind == "i8f32", "scale_local": i8 and (c.M > 256 or c.N > 256),
        "clamp_chunk": c.kind != "splitk" and c.N % 256 != 0 and c.N >= 16 and c.m_valid is None,
        "single_splitk": c.kind == "splitk" and c.scale,
    }[mutant]


def linear(c: Case, mutant: str = "") -> tuple:
    """(v, pre): the linear's value as the epilogue sees it (bf16; fp32 for the f32-scale entry) and, where one exists, the exact
    float64 value before its last rounding (what a fused single rounding would start from)."""
    d = dict(_ops(c))
    S, S2 = _product(c.kind, c.M, c.N, c.K, c.K2, c.ext)
    mode = mutant if mutant in ("trunc", "away") else "rne"
    if mutant in ("drop_first", "drop_last"):
        S = S - _tile(c, mutant[5:])
    if mutant == "drop_last_ext":
        S2 = S2 - _tile(c, "last_ext")
    if mutant == "drop_ext":
        S2 = None
    if mutant == "clamp_chunk":  # the last 8 columns from the B row (scale, epilogue operand: `epilogue`) one chunk early
        S = torch.cat([S[:, :-8], S[:, -9:-8].expand(-1, 8)], 1)
        S2 = None if S2 is None else torch.cat([S2[:, :-8], S2[:, -9:-8].expand(-1, 8)], 1)
        if "sb" in d:
            d["sb"] = torch.cat([d["sb"][:-8], d["sb"][-9:-8].expand(8)])
    if mutant == "scale_local":
        d["sa"], d["sb"] = d["sa"][torch.arange(c.M) % 256], d["sb"][torch.arange(c.N) % 256]
    if c.kind in ("bf16", "splitk"):
        pre = S if S2 is None else S + S2
        return rnd(pre, mode), pre
    sa, sb = d["sa"][:, None], d["sb"][None, :]
    if not c.ext:  # gemm_bf16.hip:395 / :464: ((float)acc * rs) * sb, two fp32 multiplies
        v32 = (S.float() * sb.float()) * sa.float() if mutant == "scale_order" else (S.float() * sa.float()) * sb.float()
        return (v32, None) if c.kind == "i8f32" else (rnd(v32, mode), None)
    deq = S * sa * sb  # powers of two: exact
    if S2 is None:     # the extension entry without extension tiles: one rounding at the pack (gemm_bf16.hip:464, :471)
        return rnd(deq, mode), deq
    if mutant == "single_i8ext":
        return rnd(deq + S2, mode), deq + S2
    pre = rnd(deq, mode).double() + S2  # gemm_bf16.hip:226: dequantised in place, rounded to bf16, kept as fp32 bits; the extension adds on top
    return rnd(pre, mode), pre


def epilogue(c: Case, v: torch.Tensor, pre, mutant: str = "") -> dict:
    """What the kernel stores for the linear's value v: {"out": ...} and per epilogue "z" (GELU pre-activation) / "dh"."""
    mode = mutant if mutant in ("trunc", "away") else "rne"
    e = epi_operand(c)
    if e is not None and mutant == "clamp_chunk" and c.epi != "swiglu_bwd":
        e = torch.cat([e[..., :-8], e[..., -16:-8]], -1)
    if c.kind == "i8f32" or c.epi in ("none", "swiglu_fwd"):
        return {"out": v}
    x = v.double()
    if c.epi in ("res", "bias"):      # gemm_bf16.hip:508 / :513: bf16(bf16(acc) + e)
        return {"out": rnd(pre + e if mutant == "single_res" else x + e, mode)}
    if c.epi == "colscale":           # gemm_bf16.hip:535: bf16(bf16(acc) * e[n])
        return {"out": rnd(pre * e, mode, exact=False) if mutant == "single_colscale" else rnd(x * e, mode)}
    if c.epi == "gelu":               # gemm_bf16.hip:515: gelu_erf(bf16(bf16(acc) + bias))
        z = rnd(x + e, mode)
        return {"z": z, "out": rnd(gelu64(z.double()), exact=False)}
    if c.epi == "swiglu_bwd":
        return {"dh": v, "out": v}
    assert c.epi == "rope"            # gemm_bf16.hip:530, common.h:162 rope8 on the bf16-rounded projection
    t = rope_table().double()[torch.arange(c.M) % ROPE_S]                      # [M, 64, 2]
    y = x.clone()
    xr = x[:, : c.rope_cols].reshape(c.M, -1, 64, 2)                            # [M, heads, pair, 2]
    cs, sn = t[:, None, :, 0], t[:, None, :, 1]
    yr = torch.stack([xr[..., 0] * cs - xr[..., 1] * sn, xr[..., 1] * cs + xr[..., 0] * sn], -1)
    y[:, : c.rope_cols] = yr.reshape(c.M, c.rope_cols)
    return {"out": rnd(y, mode)}


def expected(c: Case, mutant: str = "") -> dict:
    """The one correct result of a case (or what the planted fault `mutant` would store), see the table in the module docstring."""
    assert not mutant or live(c, mutant), (c.id, mutant)
    v, pre = linear(c, mutant)
    if c.kind != "splitk":
        return epilogue(c, v, pre, mutant)
    mode = mutant if mutant in ("trunc", "away") else "rne"
    out = v                            # gemm_bf16.hip:709-712: bf16(scale * bf16(sum)) | bf16(sum)
    if c.scale:
        out = rnd(pre * SK_SCALE, mode, exact=False) if mutant == "single_splitk" else rnd(v.double() * SK_SCALE, mode)
    if c.inv:
        inv = sk_inv(c).long()
        out = torch.where((inv >= 0)[:, None], out[inv.clamp(min=0)], torch.zeros((), dtype=out.dtype))
    return {"out": out}


def first_rounding(c) -> torch.Tensor:
    """The exact float64 values at the first bf16 rounding point of the case (what the rounding and tie shares are counted on)."""
    if isinstance(c, TnCase):
        a, b = tn_dense(c)
        return a[: c.m_eff].T @ b[: c.m_eff]
    S, S2 = _product(c.kind, c.M, c.N, c.K, c.K2, c.ext)
    d = _ops(c)
    if c.kind in ("bf16", "splitk"):
        return S if S2 is None else S + S2
    if c.ext:
        return S * d["sa"][:, None] * d["sb"][None, :]
    return ((S.float() * d["sa"].float()[:, None]) * d["sb"].float()[None, :]).double()


def tn_expected(c: TnCase, mutant: str = "") -> torch.Tensor:
    """bf16(a[:m]^T . b[:m]) with m = min(M, max(m_valid, 0)) (gemm_tn.hip:97); all +0 for m = 0."""
    assert not mutant or live(c, mutant)
    a, b = tn_dense(c)
    m = c.m_eff
    lo, hi = 0, m
    if mutant == "drop_first":
        lo = min(64, m)
    if mutant == "drop_last":
        hi = (m - 1) // 64 * 64
    # + 0.0: the accumulators start at +0, so a sum of zero products is +0 whatever the signs of the products (-0 + +0 = +0)
    return rnd(a[lo:hi].T @ b[lo:hi] + 0.0, mutant if mutant in ("trunc", "away") else "rne")
