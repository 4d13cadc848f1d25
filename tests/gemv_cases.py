"""Cases for the decode GEMV (gemv_kernel / gemv_run of csrc/decode.hip, the epilogues of csrc/wstream.h, reached through
llx.kernels.gemv): one per class of every axis the code distinguishes, operands on which the kernel's arithmetic has exactly one correct
answer, the float64 reference that computes it, and planted faults - what plausibly wrong kernels would return.  tests/test_gemv_cases.py
checks all of this on the CPU, tests/test_gemv_classes_gpu.py runs the table on the GPU with torch.equal as the bar.

Why exact.  The kernel sums products in fp32 in an order of its own (fmas along a lane's 8 or 16 elements, one partial sum per lane and
row, the DPP / permlane butterfly over the 64 lanes).  When every product and every partial sum of any subset is exactly representable in
fp32 the order does not matter; the sum is THE sum.  The operands below are small integers (half-integers with LoRA), so that holds, and
the linear's sum additionally fits bf16 (|sum| <= 256 for integers, <= 128 for multiples of 1/2): the first rounding point, bf16(sum), is
the identity and a dropped or doubled product always changes it.  Everything after the sum is a chain of single fp32 operations on known
values, each correctly rounded, which float64 followed by a rounding to fp32 reproduces bit for bit:

    bf16 rows        v = bf16(S + s L)                       S = x . W[row], L = t . Bext[row], s = lora_scale (one fp32 sum)
    bf16 + DoRA      v = bf16(bf16(S + s L) * c[row])
    int8 weight-only v = bf16(bf16(S) * scale[row]);          with LoRA  v <- bf16(v + s L)     (adapter after the base's rounding)
    int8 dynamic     v = bf16(((float)S_int * xscale[m]) * scale[row]);  with LoRA  v <- bf16(v + s L)
                     (S_int over the codes of quantize_int8_rowwise on the (normalised) row: oracle.ref.int8_mm_dequant's formula)
    none             out = v
    residual         out = bf16(v + res)
    q|k|v            q, k: (y0, y1) = (v0 c - v1 s, v1 c + v0 s) per pair with table row m, rounded once; v rows stored as they are;
                     k, v at cache[head, pos[m]]
    SwiGLU           h = bf16(bf16(g sigmoid(g)) * u), g = v of the gate row, u = v of the up row

Operand families.
  A "probe x": W dense integers in [-15, 15]; every row of x has at most 6 non-zeros from {+-1, +-2} on the boundary columns of the case
    (0, 7, 8, the last element of a lane load, PIECE - 1, PIECE, STEP - 1, STEP, the start of the last step, K - 8, K - 1), K - 1
    always, the others rotating with the token.  |S| <= 180.  Under an adapter with scale 0.5 the non-zeros are two +-2 and four +-1
    (sum |x| = 8, |S| <= 120): half-integer adapter terms ride on top and S + s L has to stay within 128.
  B "probe W": x dense +-1 (mean square exactly 1), norm weight in {+-1, +-2}, eps 1e-5: rstd = 1 - 5e-6 to within rsqrtf's few ulp, so
    bf16(x rstd w) = x w whatever those last bits are.  Every row of W has at most 8 integer non-zeros in [-15, 15], four on boundary
    columns, four anywhere: |S| <= 240.  Under an adapter the range is [-7, 7] (|S| <= 112, so that S + s L stays within 128 for
    half-integers and within 256 for integers).  Dynamic int8: norm weight in {+-1} only - with a 2 in the row the code of 1 is rint(63.5), a tie;
    every code is then +-127, asserted by `_codes`.
  G Gaussian x and row-wise quantised Gaussian W: the dynamic int8 kind without norm, whose integer sums are exact on any data and
    whose target has always been oracle.ref.int8_linear.
  LoRA: t (an input here) integers in [-1, 1], at most 4 non-zeros per segment on ranks 0, 7, 8, r - 1; B integers in [-3, 3]; scale 0.5
    or 2: |s L| <= 24.  Residual: multiples of 1/4 in [-32, 32].  DoRA factors / int8 row scales: seeded bf16 values in [0.5, 2] /
    [0.25, 4], different for every row (bf16 x bf16 is exact in fp32).  RoPE table: (c, s) from {(1,0), (0,1), (-1,0), (0,-1),
    (+-1/2, +-1/2)} per (token, pair): products by them are exact, so the rotation is one rounding however it is contracted.
`reference` asserts all of it: representable in fp32 at every fp32 intermediate, in bf16 at the linear's sum, |S| <= 256.

Dispatch, re-derived from gemv_run / gemv_kernel (two rows per wave):
  elements per 16-byte lane load EPL = 8 (bf16) | 16 (int8); PIECE = 64 EPL = 512 | 1024; STEP = 4 PIECE = 2048 | 4096;
  LDS row Kp = ceil(K / STEP) STEP (bf16) | (ceil(K / PIECE) + 1) PIECE (int8); staged bytes per element xb = 2, 1 for dynamic int8;
  a pass of mt in {4, 2, 1} staged rows fits when mt Kp xb + 64 <= 65536:
    bf16         mt Kp <= 32736: 4 rows Kp <= 6144 (K <= 6144); 2 rows Kp <= 14336 (K <= 14336); 1 row Kp <= 30720; K = 30728 rejects
    int8 dynamic mt Kp <= 65472: 4 rows Kp <= 15360 (K <= 14336); 2 rows Kp <= 31744 (K <= 30720); 1 row always (K <= 32768)
    int8 w-only  no 4-row build: M = 3, 4 always go as pairs; 2 rows Kp <= 15360 (K <= 14336); 1 row Kp <= 31744 (K <= 30720)
  M = 3 in one pass is the 4-row build with a clamped fourth row; per pass x, out, res, rope (+ m0 128), pos and t are offset by hand.
  rows: groups = ceil(N / 2) (SwiGLU: N / 2 hidden units, one gate and one up row each); per_wave = ceil(groups / 2048);
  grid = ceil(ceil(groups / per_wave) / 4) workgroups of 4 waves; wave w takes groups w, w + 4 grid, ...; N = 4096 -> 2048 groups, one
  each; N = 4098 -> 2049 groups on 1028 waves (1021 with two, 7 with one); N = 8194 -> 4097 groups on 1368 waves (1361 with three).
  An odd N leaves the last group one live row: clamped loads, guarded store.  LoRA: lane l holds ranks 8 l .. 8 l + 7 while 8 l < rank.
"""
import functools
from dataclasses import dataclass

import torch

from oracle import ref as O

BF16 = torch.bfloat16
EPS = 1e-5
SENTINEL = -(2.0 ** 100)  # exact in bf16 and far beyond any output of these cases (`reference` checks that none equals it)
KINDS = ("bf16", "dora", "i8w", "i8d")
ROPE_PAIRS = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0), (0.5, 0.5), (0.5, -0.5), (-0.5, 0.5), (-0.5, -0.5))


# ------------------------------------------------------------------------------------------------------------------------ dispatch
def geometry(kind: str) -> tuple:
    """(EPL, PIECE, STEP, staged bytes per activation element)."""
    epl = 8 if kind in ("bf16", "dora") else 16
    return epl, 64 * epl, 256 * epl, 1 if kind == "i8d" else 2


def lds_row(kind: str, K: int) -> int:
    _, piece, step, _ = geometry(kind)
    return -(-K // step) * step if kind in ("bf16", "dora") else (-(-K // piece) + 1) * piece


def nsteps(kind: str, K: int) -> int:
    return -(-K // geometry(kind)[2])


def passes(kind: str, K: int, M: int):
    """The (first token, token count) of every launch gemv_run makes, or None where it rejects."""
    epl, _, _, xb = geometry(kind)
    if not (1 <= M <= 4 and K > 0 and K % epl == 0 and K <= 32768):
        return None
    kp = lds_row(kind, K)
    fits = lambda mt: mt * kp * xb + 64 <= 64 * 1024  # noqa: E731
    per = 4 if M > 2 else M
    if per == 4 and (kind == "i8w" or not fits(4)):
        per = 2
    if per == 2 and not fits(2):
        per = 1
    if not fits(per):
        return None
    return [(m0, min(per, M - m0)) for m0 in range(0, M, per)]


def pass_class(kind: str, K: int, M: int) -> str:
    p = passes(kind, K, M)
    if p is None:
        return "reject"
    return "one" if len(p) == 1 else ("pairs" if p[0][1] == 2 else "single")


def launch_shape(N: int, swiglu: bool = False) -> tuple:
    """(row groups, groups per wave at most, workgroups, waves)."""
    groups = N // 2 if swiglu else -(-N // 2)
    per_wave = -(-groups // 2048)
    grid = -(-(-(-groups // per_wave)) // 4)
    return groups, per_wave, grid, 4 * grid


def boundary_cols(kind: str, K: int) -> list:
    epl, piece, step, _ = geometry(kind)
    last_step = (nsteps(kind, K) - 1) * step
    cand = (0, 7, 8, epl - 1, epl, piece - 1, piece, step - 1, step, last_step - 1, last_step, K - 8, K - 1)
    return sorted({c for c in cand if 0 <= c < K})


# ------------------------------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    id: str
    kind: str                # bf16 | dora | i8w | i8d
    K: int
    ns: tuple                # rows of each weight (SwiGLU: (I, I))
    M: int
    epi: str = "none"        # none | res | qkv | swiglu
    fam: str = "A"           # A | B | G
    norm: bool = False
    ranks: tuple = ()        # LoRA rank of each weight; () = no adapter
    lscale: float = 2.0
    strided: bool = False    # x, out, res, t as column slices of wider buffers (the weights are always row-strided views)

    @property
    def N(self):
        return sum(self.ns)

    @property
    def n_out(self):
        return {"none": self.N, "res": self.N, "qkv": 256, "swiglu": self.ns[0]}[self.epi]


def _table() -> list:
    cs = []

    def add(id_, kind, K, ns, M, **kw):
        if kind == "i8d" and kw.get("fam", "A") == "A":  # the dynamic kind quantises x: family A would put the code of 1 on a tie
            kw["fam"] = "B"
        cs.append(Case(f"{kind}-{id_}", kind, K, tuple(ns), M, **kw))

    for kind in KINDS:
        i8 = kind in ("i8w", "i8d")
        ks = (16, 1008, 1024, 1040, 4096, 4112, 9216) if i8 else (8, 504, 512, 520, 2040, 2048, 2056, 4608)
        k1, k2 = (1040, 4112) if i8 else (520, 2056)  # one step with a one-lane last piece | two steps, the second one lane wide
        # K against PIECE and STEP, N odd, M cycling 1..4, the two families alternating
        for i, K in enumerate(ks):
            fam = "B" if i % 2 else "A"
            add(f"K{K}", kind, K, (37,), 1 + i % 4, fam=fam, norm=fam == "B" and i % 4 == 1)
            add(f"K{K}-norm", kind, K, (37,), 1 + (i + 2) % 4, fam="B", norm=True, epi="res" if i % 2 else "none")
        if kind == "i8d":
            for M, K in ((1, 1040), (4, 4112), (3, 14352)):  # Gaussian data, no norm: the bit-exact target this kind always had
                add(f"gauss-K{K}-M{M}", kind, K, (37,), M, fam="G", epi="res" if M == 3 else "none")
        # rows: the clamp of N = 1, idle waves behind the barrier, exactly 2048 groups, then waves that own 2 and 3 groups
        add("N1", kind, k1, (1,), 2)
        add("N10", kind, k1, (10,), 3, fam="B", norm=True, epi="res")
        add("N4096", kind, k1, (4096,), 1, epi="res", strided=True)
        add("N4098-2steps", kind, k2, (4098,), 1)
        add("N4098-B", kind, k1, (4098,), 4, fam="B", norm=True, epi="res", ranks=(16,), lscale=0.5)
        add("N8194", kind, k1, (8194,), 3)
        # segments: two and three weights, inner sizes 4 and 8, the last one odd
        add("seg-4-8-5", kind, k1, (4, 8, 5), 2, epi="res", strided=True)
        add("seg-8-3", kind, k2, (8, 3), 3, fam="B", norm=True)
        add("seg-8-8", kind, k1, (8, 8), 1)
        # epilogues: q|k|v as three weights and as one, SwiGLU with I = 5 and I = 2049 (UPG = 1: a wave's second unit)
        add("qkv-3w", kind, k1, (256, 256, 256), 4, epi="qkv", strided=True)
        add("qkv-1w", kind, k2, (768,), 1, epi="qkv", fam="B", norm=True)
        add("qkv-q-kv", kind, k1, (256, 512), 3, epi="qkv", fam="B", norm=True, ranks=(8, 16), strided=True)
        add("swiglu-I5", kind, k1, (5, 5), 3, epi="swiglu", strided=True)
        add("swiglu-I2049", kind, k1, (2049, 2049), 2, epi="swiglu", fam="B", norm=True)
        add("swiglu-I5-lora", kind, k2, (5, 5), 4, epi="swiglu", ranks=(8, 24), lscale=0.5, strided=True)
        # LoRA: one lane, eight lanes, all 64; one segment (bext / t_off of segments 1, 2 alias segment 0), unequal ranks over three
        for r in (8, 64, 512):
            add(f"lora-r{r}", kind, k1, (37,), 1 + (r // 8) % 4, ranks=(r,), lscale=0.5 if r == 64 else 2.0, epi="res" if r == 512 else "none", strided=r == 8)
        add("lora-r8-24-16", kind, k1, (8, 12, 9), 2, ranks=(8, 24, 16), strided=True, epi="res")
        add("lora-r8-24-16-B", kind, k2, (8, 12, 9), 4, fam="B", norm=True, ranks=(8, 24, 16), lscale=0.5)
        add("lora-r64-8", kind, k1, (40, 41), 3, ranks=(64, 8))
        # strides alone
        add("strided", kind, k2, (37,), 2, strided=True)
        # tokens per pass: every multi-pass class with residual and with q|k|v, LoRA on both
        kp, k1p = {"bf16": (6152, 14344), "dora": (6152, 14344), "i8d": (14352, 30736), "i8w": (1040, 14352)}[kind]
        for K, Ms in ((kp, (3, 4)), (k1p, (2, 3, 4))):
            for M in Ms:
                tag = f"{pass_class(kind, K, M)}-K{K}-M{M}"
                fam = "B" if (M % 2 or kind == "i8d") else "A"
                add(f"{tag}-res", kind, K, (8, 5), M, epi="res", fam=fam, norm=fam == "B", ranks=(8, 16), strided=True)
                add(f"{tag}-qkv", kind, K, (256, 256, 256), M, epi="qkv", fam="B", norm=M != 3, ranks=(16, 8, 24), lscale=0.5, strided=M == 4)
    return cs


CASES = {c.id: c for c in _table()}
assert len(CASES) == len(_table())
# (entry, kind, K, M, rank): LlxError before any launch
REJECTS = (("K too large for the LDS stage", "bf16", 30728, 1, 0), ("K too large for the LDS stage", "i8w", 30736, 1, 0),
           ("ranks must be multiples of 8, at most 512", "bf16", 520, 1, 520), ("outside 1..4", "bf16", 520, 5, 0))


# ------------------------------------------------------------------------------------------------------------------------ operands
def _bf(x):
    return x.to(BF16)


def _slice(rows: int, cols: int, off: int, tail: int, fill: float, dtype=BF16):
    """A [rows, cols] column slice of a wider buffer filled with `fill`."""
    base = torch.full((rows, off + cols + tail), fill, dtype=dtype)
    return base[:, off:off + cols]


def _scales(tag: str, n: int, lo: float, hi: float):
    """Seeded bf16 values in [lo, hi], a different one for neighbouring rows."""
    v = _bf(O.uniform(tag, (n,), lo, hi))
    same = torch.nonzero(v[1:] == v[:-1]).flatten() + 1
    v[same] = v[same] * 1.5
    return v.contiguous()


@functools.lru_cache(maxsize=24)
def build(cid: str) -> dict:
    """The CPU operands of a case.  Strided operands are views; their ._base holds the gaps."""
    c = CASES[cid]
    M, K, N = c.M, c.K, c.N
    epl = geometry(c.kind)[0]
    i8 = c.kind in ("i8w", "i8d")
    wdt = torch.int8 if i8 else BF16
    bcols = boundary_cols(c.kind, K)
    d = {"case": c}
    # ---- x
    if c.fam == "A":
        x = torch.zeros(M, K)
        for m in range(M):
            rest = [b for b in bcols if b != K - 1]
            cols = [K - 1] + [rest[(5 * m + j) % len(rest)] for j in range(min(5, len(rest)))]
            sign = (O.randint(f"gc_xs_{cid}_{m}", (6,), 0, 2) * 2 - 1).float()
            if c.ranks and c.lscale == 0.5:  # half-integer adapter terms on top: sum |x| = 8 keeps S + s L within 128
                vals = torch.tensor([2.0, 1.0, 1.0, 2.0, 1.0, 1.0])[O.randint(f"gc_xp_{cid}_{m}", (6,), 0, 6).argsort()] * sign
            else:
                vals = (1 + O.randint(f"gc_xm_{cid}_{m}", (6,), 0, 2)).float() * sign
            for col, v in zip(cols, vals):
                x[m, col] = v  # (a repeated column keeps its last value)
    elif c.fam == "B":
        x = (O.randint(f"gc_x_{cid}", (M, K), 0, 2) * 2 - 1).float()
    else:
        x = O.randn(f"gc_x_{cid}", (M, K), 1.0)
    xv = _slice(M, K, 8, 16, float("nan")) if c.strided else torch.empty(M, K, dtype=BF16)
    xv.copy_(x)
    d["x"] = xv
    if c.norm:
        assert c.fam == "B"
        nw = O.randint(f"gc_nw_{cid}", (K,), 0, 2) * 2 - 1
        if c.kind != "i8d":
            nw = nw * (1 + O.randint(f"gc_nw2_{cid}", (K,), 0, 2))
        d["norm_w"] = _bf(nw.float())
    # ---- weights: row-strided views with a stride of their own, the gaps poisoned
    ws, sparse = [], []
    for s, n in enumerate(c.ns):
        ld = K + epl * (s + 1)
        base = torch.full((n, ld), 127 if i8 else float("nan"), dtype=wdt)
        w = base[:, :K]
        if c.fam == "A":
            w.copy_(O.randint(f"gc_w_{cid}_{s}", (n, K), -15, 16))
            sparse.append(None)
        elif c.fam == "B":
            bi = torch.tensor(bcols)[O.randint(f"gc_wb_{cid}_{s}", (n, 4), 0, len(bcols))]
            idx = torch.cat([bi, O.randint(f"gc_wi_{cid}_{s}", (n, 4), 0, K)], 1).sort(1).values
            val = O.randint(f"gc_wv_{cid}_{s}", (n, 8), 1, 8 if c.ranks else 16) * (O.randint(f"gc_wg_{cid}_{s}", (n, 8), 0, 2) * 2 - 1)
            val[:, 1:][idx[:, 1:] == idx[:, :-1]] = 0  # a column drawn twice counts once
            w.copy_(torch.zeros(n, K, dtype=torch.int16).scatter_add_(1, idx, val.to(torch.int16)))
            sparse.append((idx, val.double()))
        else:
            q, sc = O.quantize_int8_rowwise(_bf(O.randn(f"gc_w_{cid}_{s}", (n, K), 0.05)))
            w.copy_(q)
            d.setdefault("wscale", []).append(sc.contiguous())
            sparse.append(None)
        ws.append(w)
    d["ws"], d["sparse"] = ws, sparse
    if i8 and c.fam != "G":
        d["wscale"] = [_scales(f"gc_sc_{cid}_{s}", n, 0.25, 4.0) for s, n in enumerate(c.ns)]
    if c.kind == "dora":
        d["colscale"] = [_scales(f"gc_c_{cid}_{s}", n, 0.5, 2.0) for s, n in enumerate(c.ns)]
    # ---- LoRA
    if c.ranks:
        R = sum(c.ranks)
        t = torch.zeros(M, R)
        off = 0
        for s, r in enumerate(c.ranks):
            at = sorted({p for p in (0, 7, 8, r - 1) if p < r})
            sg = O.randint(f"gc_t_{cid}_{s}", (M, len(at)), -1, 2)
            sg[:, -1] = sg[:, -1] + (sg[:, -1] == 0)  # rank r - 1 always carries something
            for j, p in enumerate(at):
                t[:, off + p] = sg[:, j].float()
            off += r
        tv = _slice(M, R, 8, 8, float("nan")) if c.strided else torch.empty(M, R, dtype=BF16)
        tv.copy_(t)
        d["t"] = tv
        d["bext"] = [_bf(O.randint(f"gc_b_{cid}_{s}", (n, r), -3, 4).float()).contiguous() for s, (n, r) in enumerate(zip(c.ns, c.ranks))]
    # ---- epilogue operands
    if c.epi == "res":
        r = O.randint(f"gc_r_{cid}", (M, N), -128, 129).float() / 4
        rv = _slice(M, N, 1, 2, float("nan")) if c.strided else torch.empty(M, N, dtype=BF16)
        rv.copy_(r)
        d["res"] = rv
    if c.epi == "qkv":
        pick = O.randint(f"gc_rope_{cid}", (M, 64), 0, len(ROPE_PAIRS))
        d["rope"] = torch.tensor(ROPE_PAIRS)[pick].float().contiguous()  # [M, 64, 2]
        kvh, smax = (N - 256) // 256, 9
        for name in ("kc", "vc"):  # [1, KVH, Smax, 128] views of [1, Smax, KVH, 160]: c_sh = 160, c_ss = KVH * 160
            d[name] = torch.full((1, smax, kvh, 160), SENTINEL, dtype=BF16).permute(0, 2, 1, 3)[..., :128]
        d["pos"] = torch.tensor([5, 2, 7, 0][:M], dtype=torch.int64)
    off = (4 if c.epi == "qkv" else 3) if c.strided else 0
    d["out"] = _slice(M, c.n_out, off, 8 - off if c.strided else 0, SENTINEL)
    return d


# ------------------------------------------------------------------------------------------------------------------------ reference
def rbf(v):
    """float64 -> fp32 -> bf16, back in float64: a value formed in fp32 and rounded to bf16."""
    return v.float().to(BF16).double()


def _f32(v, exact: bool, what: str):
    r = v.float().double()
    if exact:
        assert torch.equal(r, v), f"{what}: not representable in fp32"
    return r


def _dot(d: dict, s: int, x64):
    """x64 [M, K] . W_s^T in float64 through whichever operand is sparse."""
    if d["sparse"][s] is not None:
        idx, val = d["sparse"][s]
        return (x64[:, idx] * val).sum(-1)
    cols = torch.nonzero(x64.abs().sum(0)).flatten()
    if cols.numel() > 256:
        return x64 @ d["ws"][s].double().T
    return x64[:, cols] @ d["ws"][s][:, cols].double().T


def _codes(xn_bf16, check: bool):
    """quantize_int8_rowwise of the (normalised) rows; check: no quotient within 1e-3 of a rounding tie."""
    q, sc = O.quantize_int8_rowwise(xn_bf16)
    if check:
        quo = xn_bf16.float() / (xn_bf16.float().abs().amax(1) / 127).clip(1e-12).view(-1, 1)
        assert ((quo - quo.floor() - 0.5).abs() > 1e-3).all(), "a quantiser code sits on a tie"
    return q, sc


FAULTS = ("drop_last8", "lds_pad", "seg1_from_seg0", "pass2_stale", "t_off1_zero", "ranks_ge64_ignored", "tok2_from_tok1", "i8w_halves_swapped",
          "scale_row_plus1", "group_repeat", "res_before_round", "i8_adapter_before_round")


def reference(d: dict, fault: str = None) -> dict:
    """float64 evaluation with the kernel's rounding points.  Returns out [M, n_out] bf16 (SwiGLU: also h64, the float64 value of
    bf16(g sigmoid(g)) u before its last rounding, and g, u) and for q|k|v the whole expected cache buffers kc, vc.
    fault: what a kernel with that defect would return instead (the exactness assertions are then off)."""
    c = d["case"]
    assert fault is None or fault in FAULTS
    exact = fault is None and c.fam != "G"
    M, K, N = c.M, c.K, c.N
    # ---- the activation rows the linear sees
    x = d["x"].double()
    if c.norm:
        w = d["norm_w"].double()
        rstd = 1.0 / torch.sqrt(x.pow(2).mean(1, keepdim=True) + EPS)
        xn = rbf(x * rstd * w)
        if exact:  # mean square exactly 1: bf16(x rstd w) = x w for any rstd within 2^-10 of 1
            assert torch.equal(x.pow(2).mean(1), torch.ones(M, dtype=torch.float64)) and torch.equal(xn, x * w)
            assert torch.equal(rbf(x * (rstd * (1 + 2.0 ** -10)) * w), xn) and torch.equal(rbf(x * (rstd * (1 - 2.0 ** -10)) * w), xn)
    else:
        xn = x
    xsc = None
    if c.kind == "i8d":
        q, xsc = _codes(xn.to(BF16), exact)
        if exact:
            assert (q.abs() == 127).all()
        xn = q.double()
    if fault == "drop_last8":
        xn = xn.clone(); xn[:, K - 8:] = 0
    if fault == "lds_pad":  # the lanes past the row end re-read the row's start: harmless only against a zero pad
        xn = xn.clone(); xn[:, :8] *= 2
    if fault == "i8w_halves_swapped":
        xn = xn.reshape(M, K // 16, 2, 8).flip(2).reshape(M, K)
    # ---- the linear's sums
    parts = [_dot(d, 0 if (fault == "seg1_from_seg0" and s == 1) else s, xn)[:, :n] for s, n in enumerate(c.ns)]
    S = torch.cat(parts, 1)
    if fault == "group_repeat":
        _, per_wave, _, nwaves = launch_shape(N)
        assert per_wave > 1
        S = S.clone(); S[:, 2 * nwaves:4 * nwaves] = S[:, :2 * nwaves][:, :S[:, 2 * nwaves:4 * nwaves].shape[1]]
    if fault == "tok2_from_tok1":
        S = S.clone(); S[2] = S[1]
    if exact:  # (dynamic int8: every code is +-127, the integer sum is 127 x a sum of at most 8 weights; it is exact in int32 anyway)
        assert (S / 127 if c.kind == "i8d" else S).abs().max() <= 256, "a linear sum beyond 256"
        assert c.kind != "i8d" or torch.equal(S, (S / 127).round() * 127)
    S = _f32(S, exact, "linear sum")
    # first pass's rows for the later passes
    side = list(range(M))
    if fault == "pass2_stale":
        p = passes(c.kind, K, M)
        assert len(p) > 1
        side = [m - m0 for m0, mc in p for m in range(m0, m0 + mc)]
    L = None
    if c.ranks:
        t = d["t"].double()[side]
        offs = [sum(c.ranks[:s]) for s in range(len(c.ranks))]
        if fault == "t_off1_zero":
            offs[1] = 0
        ls = []
        for s, r in enumerate(c.ranks):
            ts = t[:, offs[s]:offs[s] + r].clone()
            if fault == "ranks_ge64_ignored":
                ts[:, 64:] = 0
            ls.append(ts @ d["bext"][s].double().T)
        L = _f32(c.lscale * torch.cat(ls, 1), exact, "adapter sum")
        if exact:
            assert L.abs().max() <= 24
    # ---- the per-row factors
    fac = None
    if c.kind != "bf16":
        fs = d["colscale"] if c.kind == "dora" else d["wscale"]
        if fault == "scale_row_plus1":
            fs = [f[torch.arange(1, f.numel() + 1).clamp(max=f.numel() - 1)] for f in fs]
        fac = torch.cat(fs).double().view(1, N)
    # ---- v: the linear's bf16 output; pre: the fp32 value in front of its last rounding
    if c.kind in ("bf16", "dora"):
        tot = _f32(S + L if L is not None else S, exact, "sum + adapter")
        if exact:
            assert torch.equal(rbf(tot), tot), "the linear's sum is not representable in bf16"
        pre = tot
        if c.kind == "dora":
            pre = _f32(rbf(tot) * fac, exact, "sum x DoRA factor")
    else:
        if c.kind == "i8w":
            if exact:
                assert torch.equal(rbf(S), S)
            pre = _f32(rbf(S) * fac, exact, "sum x scale")
        else:
            pre = _f32(_f32(S * xsc.double().view(M, 1), False, "") * fac, False, "")  # two fp32 products, each correctly rounded
            if fault is None and not any(sp is not None for sp in d["sparse"]):  # dense weights: the formula above IS the oracle's
                want = O.int8_linear(d["x"].contiguous() if not c.norm else xn.to(BF16), torch.cat([w for w in d["ws"]]), torch.cat(d["wscale"]), dynamic=True)
                assert c.norm or torch.equal(rbf(pre), want.double())
        if L is not None:
            pre = _f32(pre + L, exact, "base + adapter") if fault == "i8_adapter_before_round" else _f32(rbf(pre) + L, exact, "base + adapter")
    v = rbf(pre)
    out = {}
    if c.epi == "none":
        o = v
    elif c.epi == "res":
        res = d["res"].double()[side]
        o = rbf(_f32((pre if fault == "res_before_round" else v) + res, exact, "linear + residual"))
    elif c.epi == "swiglu":
        I = c.ns[0]
        g, u = v[:, :I], v[:, I:]
        sg = g * torch.sigmoid(g)
        out["g"], out["u"] = g.to(BF16), u.to(BF16)
        out["h64"] = rbf(sg) * u
        o = rbf(out["h64"])
    else:
        rope = d["rope"].double()[side]  # [M, 64, 2]
        n_q, n_k = 256, (N - 256) // 2
        y = v.clone()
        pairs = v[:, :n_q + n_k].reshape(M, -1, 64, 2)  # [M, head, pair, 2]
        cs, sn = rope[:, None, :, 0], rope[:, None, :, 1]
        y0 = _f32(pairs[..., 0] * cs - pairs[..., 1] * sn, exact, "rotation")
        y1 = _f32(pairs[..., 1] * cs + pairs[..., 0] * sn, exact, "rotation")
        y[:, :n_q + n_k] = rbf(torch.stack([y0, y1], -1)).reshape(M, n_q + n_k)
        o = y[:, :n_q]
        pos = d["pos"][side]
        for name, lo in (("kc", n_q), ("vc", n_q + n_k)):
            base = d[name]._base.clone()
            view = base.permute(0, 2, 1, 3)[..., :128]
            for m in range(M):
                view[0, :, pos[m]] = y[m, lo:lo + n_k].reshape(-1, 128).to(BF16)
            out[name] = base
    out["out"] = o.to(BF16)
    if fault is None:
        assert not (out["out"].float() == SENTINEL).any()
    return out


def swiglu_bar(h64):
    """|h - h64| allowed for the SwiGLU epilogue against float64, h64 = bf16(g sigmoid(g)) u evaluated exactly.  The kernel's only inexact
    steps: (1) g * sigmoidf_(g) in fp32 (__expf and v_rcp_f32, about 2^-21 relative) is rounded to bf16; where the exact value sits
    that close to a rounding boundary the kernel may take the neighbour: one bf16 ulp of silu, at most 2^-7 relative, so |u| times that
    = 2^-7 |h64| (times 1 + 2^-7 for the neighbour's own size); (2) the final rounding of the exact fp32 product: half an ulp of the
    result, at most 2^-8 relative to it.  Sum: (2^-7 (1 + 2^-7) + 2^-8 (1 + 2^-6)) |h64|, plus 1e-30 absolute for gates below -87, where
    silu leaves fp32's normal range and the hardware's exp / rcp flush."""
    return (2.0 ** -7 * (1 + 2.0 ** -7) + 2.0 ** -8 * (1 + 2.0 ** -6)) * h64.abs() + 1e-30


# ------------------------------------------------------------------------------------------------------------------------ faults
# fault -> the case aimed at its class
FAULT_CASES = {
    "drop_last8": ("bf16-K2056", "i8w-K4112", "i8d-K1040", "dora-K8"),
    "lds_pad": ("bf16-K520", "i8w-K1040", "i8d-K4112-norm", "dora-K2056"),
    "seg1_from_seg0": ("bf16-seg-8-8", "i8d-seg-8-3", "dora-qkv-3w"),
    "pass2_stale": ("bf16-pairs-K6152-M3-res", "bf16-pairs-K6152-M4-qkv", "dora-single-K14344-M2-res", "i8w-pairs-K1040-M4-qkv",
                    "i8w-single-K14352-M3-res", "i8d-pairs-K14352-M3-qkv", "i8d-single-K30736-M4-res"),
    "t_off1_zero": ("bf16-lora-r8-24-16", "i8w-lora-r8-24-16-B", "dora-swiglu-I5-lora"),
    "ranks_ge64_ignored": ("bf16-lora-r512", "i8d-lora-r512", "dora-lora-r512"),
    "tok2_from_tok1": ("bf16-K512", "dora-N8194", "i8d-seg-8-3"),
    "i8w_halves_swapped": ("i8w-K16", "i8w-K1040", "i8w-strided"),
    "scale_row_plus1": ("dora-K520", "i8w-K1024", "i8d-N4096"),
    "group_repeat": ("bf16-N4098-2steps", "i8w-N8194", "i8d-N4098-B", "dora-N4098-2steps"),
    "res_before_round": ("dora-N10", "i8w-N4096", "i8d-seg-4-8-5"),
    "i8_adapter_before_round": ("i8w-lora-r8", "i8d-lora-r64", "i8w-N4098-B"),
}


def old_bar_accepts(got, want, rel: float = 0.01) -> bool:
    """The bar the GEMV had before: max error within rel x the largest reference magnitude (tests/test_decode_gpu.py::_close)."""
    return (got - want).abs().max().item() <= rel * want.abs().max().item() + 1e-6
