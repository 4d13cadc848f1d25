"""Cases and oracle for the MXFP4 weight-only linears (csrc/mxfp4.hip, subclasses/mxfp4.py): the format, hand-computed vectors, the
cases of the decode GEMV on packed rows with operands on which its arithmetic has exactly one correct answer, the float64 reference that
computes it, and planted faults - what plausibly wrong kernels would return.  tests/test_mx_cases.py checks all of this on the CPU,
tests/test_mxfp4_gpu.py runs the table on the GPU with torch.equal as the bar.  Written from the format's statement, not
from the product code: numpy float64, a nearest-point search with the tie rule applied afterwards.

The format.  W [N, K], K % 32 == 0; a block = 32 consecutive k of a row.  packed uint8 [N, K/2]: byte j = element 2j in bits 0-3,
element 2j+1 in bits 4-7; code = sign << 3 | e2m1, magnitudes GRID.  scale uint8 [N, K/32] = biased exponent b, block scale 2^(b-127).
Quantise in fp32: amax = max |x|; amax == 0: b = 127; else e = clamp(floor(log2 amax) - 2, -125, 125), b = e + 127; v = |x| 2^-e to
the nearest grid point, ties to the code with mantissa bit 0 (an even code), above 6 -> 6; sign bit = the input's.

Why the GEMV cases are exact.  Scale exponents in {-1, 0, 1} make every weight a multiple of 1/4 of magnitude <= 12; activations are
integers in [-2, 2].  Every product is a multiple of 1/4 up to 24 and any partial sum over K <= 30720 terms stays below 2^22 in units
of 1/4: exact in fp32 in any order.  The linear's fp32 sum is therefore THE sum, and the first rounding point bf16(S + s L) has one
answer.  Family P ("probe x": at most 4 non-zeros of +-1 on boundary columns, K - 1 always) keeps |S| <= 48, a multiple of 1/4: exact
in bf16 too, so that a dropped, doubled or re-scaled product always shows.  Family D (dense x in {-2..2}; under the norm x = +-1 with
mean square exactly 1 and norm weights in {+-1, +-2}, so bf16(x rstd w) = x w) is the dense stream.  LoRA: t integers in [-1, 1] on a
few ranks, B integers in [-3, 3], scale 0.5 or 2.  Everything behind the sum is the chain of tests/gemv_cases.py (residual, RoPE with
exact table entries, cache scatter, SwiGLU with its bar).

Dispatch, re-derived from llx_gemv_mxfp4 / gemv_mx4_kernel: a lane's 16-byte load is one block; PIECE = 64 blocks = 2048 elements;
a step = 2 pieces of 4 rows; LDS row Kp = ceil(K / 2048) 2048; the kernel is built for 1 and 2 staged rows, 2 rows fit while
2 Kp 2 + 64 <= 65536 (K <= 14336), 1 row while Kp <= 30720; M = 3, 4 go as (2, 1) and (2, 2), beyond K = 14336 row by row.  Rows:
groups = ceil(N / 4) (SwiGLU: ceil(I / 2) groups of two hidden units); per_wave = ceil(groups / 2048); grid = ceil(ceil(groups /
per_wave) / 4) workgroups of 4 waves; N = 8192 -> 2048 groups, one each; N = 8196 -> 2049 groups, waves with two.
"""
import functools
from dataclasses import dataclass

import numpy as np
import torch

from oracle import ref as O
from tests.gemv_cases import ROPE_PAIRS, SENTINEL, _f32, _slice, rbf, swiglu_bar  # noqa: F401  (the chain behind the sum is shared)

BF16 = torch.bfloat16
EPS = 1e-5
GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
BLOCK, PIECE, STEP = 32, 2048, 4096


# ------------------------------------------------------------------------------------------------------------------------ the format
def quantize(x: torch.Tensor):
    """(packed uint8 [N, K/2], scale uint8 [N, K/32]) of x [N, K] (bf16 or fp32), by the statement of the format."""
    assert x.dim() == 2 and x.shape[1] % BLOCK == 0
    xf = x.float().numpy()
    N, K = xf.shape
    blk = xf.astype(np.float64).reshape(N, K // BLOCK, BLOCK)
    amax = np.abs(blk).max(-1)
    _, ex = np.frexp(amax)  # amax = m 2^ex with m in [0.5, 1): floor(log2 amax) = ex - 1
    e = np.clip(ex.astype(np.int64) - 1 - 2, -125, 125)
    e = np.where(amax == 0, 0, e)
    v = np.ldexp(np.abs(blk), -e[..., None].astype(np.int32))  # exact in float64
    dist = np.abs(v[..., None] - GRID)  # [N, KB, 32, 8]
    best = dist.min(-1, keepdims=True)
    tied = dist == best  # one code, or two neighbours: exactly one of them is even
    even = np.array([c % 2 == 0 for c in range(8)])
    code = np.where(tied.sum(-1) == 1, tied.argmax(-1), (tied & even).argmax(-1)).astype(np.uint8)
    code |= np.signbit(xf.reshape(N, K // BLOCK, BLOCK)).astype(np.uint8) << 3
    code = code.reshape(N, K // 2, 2)
    packed = code[..., 0] | (code[..., 1] << 4)
    return torch.from_numpy(packed.copy()), torch.from_numpy((e + 127).astype(np.uint8))


def dequantize64(packed: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """float64 [N, K]: (-1)^sign GRID[e2m1] 2^(b - 127)."""
    p = packed.numpy()
    N, K = p.shape[0], p.shape[1] * 2
    code = np.stack([p & 15, p >> 4], -1).reshape(N, K)
    val = GRID[code & 7] * np.where(code & 8, -1.0, 1.0)
    s = np.ldexp(1.0, scale.numpy().astype(np.int32) - 127)
    return torch.from_numpy((val.reshape(N, K // BLOCK, BLOCK) * s[..., None]).reshape(N, K))


def dequantize(packed, scale) -> torch.Tensor:
    d = dequantize64(packed, scale)
    out = d.to(BF16)
    assert torch.equal(out.double(), d), "a dequantised value is not a bf16"
    return out


def _pack(codes):
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8)


# hand-computed vectors: (name, one block of 32 inputs as (value, ...) padded with zeros, expected 32 codes, expected scale byte)
def _hand():
    out = []

    def add(name, vals, codes, b, dtype=torch.float32):
        x = torch.zeros(32, dtype=torch.float32)
        x[:len(vals)] = torch.tensor(vals, dtype=torch.float32)
        c = torch.zeros(32, dtype=torch.uint8)
        c[:len(codes)] = torch.tensor(codes, dtype=torch.uint8)
        out.append((name, x.to(dtype).view(1, 32), c, b))

    # amax = 6 -> e = 0: v = x.  The whole tie table, each tie to the even code, both signs
    add("ties", [6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0],
        [7, 0, 2, 2, 4, 4, 6, 6, 8, 10, 10, 12, 12, 14, 14], 127)
    # just off the ties
    add("off-ties", [6.0, 0.2500001, 0.7499999, 1.2500001, 1.7499999, 2.5000002, 3.4999998, 5.0000005], [7, 1, 1, 3, 3, 5, 5, 7], 127)
    # amax = 7.5 -> floor(log2) = 2, e = 0: 6.5, 7 (the tie between 6 and the missing 8) and 7.5 saturate at 6
    add("saturate", [7.5, 6.5, 7.0, -7.0, 6.0, 5.5], [7, 7, 7, 15, 7, 7], 127)
    # a zero block keeps b = 127 and its signs
    add("zeros", [0.0, -0.0, 0.0, -0.0], [0, 8, 0, 8], 127)
    # -0.0 and values that round to zero next to a live amax (e = 0 - 2 = -2: v = 4 x)
    add("signs", [1.0, -0.0, -0.05, 0.05, -0.0625], [6, 8, 8, 0, 8], 125)
    # amax an exact power of two: 2^5 -> e = 3, v = 4 (code 6), never 8; the same just below: 31.9 -> e = 2, v = 7.98 -> 6
    add("pow2", [32.0, 16.0, 8.0, 4.0, 2.0, 1.0, -32.0], [6, 4, 2, 1, 0, 0, 14], 130)
    add("below-pow2", [31.9, 16.0], [7, 6], 129)
    # nibble order: element 0 = 0.5 (code 1), element 1 = 6 (code 7): byte 0 must be 0x71
    add("nibbles", [0.5, 6.0, -1.0, 1.5], [1, 7, 10, 3], 127)
    # the two ends of e.  High: the largest finite fp32 exponent gives floor(log2 amax) = 127, e = 125 - the bound itself, b = 252
    add("clamp-high", [3 * 2.0 ** 126, 2.0 ** 126, 2.0 ** 125], [7, 4, 2], 252)
    # 2^-126 -> e would be -128 -> clamped to -125: v = 0.5; a denormal amax 2^-130 -> v = 2^-5 -> 0
    add("clamp-low", [2.0 ** -126, -(2.0 ** -125), 3 * 2.0 ** -126], [1, 10, 3], 2)
    add("clamp-low-denormal", [2.0 ** -130, -(2.0 ** -130)], [0, 8], 2)
    # the same ties from bf16 input (all exactly representable)
    add("ties-bf16", [6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], [7, 0, 2, 2, 4, 4, 6, 6], 127, dtype=BF16)
    return out


HAND = _hand()


# ------------------------------------------------------------------------------------------------------------------------ dispatch
def lds_row(K: int) -> int:
    return -(-K // PIECE) * PIECE


def passes(K: int, M: int):
    """The (first row, row count) of every launch of llx_gemv_mxfp4, or None where it rejects."""
    if not (1 <= M <= 4 and K > 0 and K % BLOCK == 0 and K <= 32768):
        return None
    fits = lambda mt: mt * lds_row(K) * 2 + 64 <= 64 * 1024  # noqa: E731
    per = 2 if (M >= 2 and fits(2)) else 1
    if not fits(per):
        return None
    return [(m0, min(per, M - m0)) for m0 in range(0, M, per)]


def pass_class(K: int, M: int) -> str:
    p = passes(K, M)
    if p is None:
        return "reject"
    return "one" if len(p) == 1 else ("pairs" if p[0][1] == 2 else "single")


def launch_shape(N: int, swiglu: bool = False) -> tuple:
    """(row groups, groups per wave at most, workgroups, waves); N = all weight rows (SwiGLU: 2 I)."""
    groups = -(-(N // 2) // 2) if swiglu else -(-N // 4)
    per_wave = -(-groups // 2048)
    grid = -(-(-(-groups // per_wave)) // 4)
    return groups, per_wave, grid, 4 * grid


def boundary_cols(K: int) -> list:
    last_step = (-(-K // STEP) - 1) * STEP
    cand = (0, 1, 7, 8, 31, 32, 63, 64, PIECE - 1, PIECE, STEP - 1, STEP, last_step - 1, last_step, K - 32, K - 2, K - 1)
    return sorted({c for c in cand if 0 <= c < K})


# ------------------------------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    id: str
    K: int
    ns: tuple                # rows of each weight (SwiGLU: (I, I))
    M: int
    epi: str = "none"        # none | res | qkv | swiglu
    fam: str = "P"           # P (probe x) | D (dense)
    norm: bool = False       # family D only
    ranks: tuple = ()
    lscale: float = 2.0
    strided: bool = False    # x, out, res, t as column slices of wider buffers; packed rows and scale rows with strides of their own

    @property
    def N(self):
        return sum(self.ns)

    @property
    def n_out(self):
        return {"none": self.N, "res": self.N, "qkv": 256, "swiglu": self.ns[0]}[self.epi]


def _table() -> list:
    cs = []

    def add(id_, K, ns, M, **kw):
        cs.append(Case(id_, K, tuple(ns), M, **kw))

    # K against the block, the piece and the step; N ragged; M cycling 1..4; the two families alternating, the norm on the dense one
    for i, K in enumerate((32, 64, 2048, 2080, 4096, 4128, 6176, 14336)):
        fam = "D" if i % 2 else "P"
        add(f"K{K}", K, (37,), 1 + i % 4, fam=fam, strided=i % 4 == 2)
        add(f"K{K}-norm", K, (37,), 1 + (i + 2) % 4, fam="D", norm=True, epi="res" if i % 2 else "none")
    # rows: the clamp of N = 1, a ragged last group, idle waves, exactly 2048 groups, waves that own two groups (one and two steps)
    add("N1", 2080, (1,), 2)
    add("N5", 2080, (5,), 3, fam="D", norm=True, epi="res")
    add("N8192", 64, (8192,), 1, epi="res", strided=True)
    add("N8196", 2080, (8196,), 2, fam="D")
    add("N8196-2steps", 4128, (8196,), 1)
    # segments: two and three weights, inner sizes 4 and 8, the last one ragged
    add("seg-4-8-5", 2080, (4, 8, 5), 2, epi="res", strided=True)
    add("seg-8-3", 4128, (8, 3), 3, fam="D", norm=True)
    add("seg-8-8", 2080, (8, 8), 1)
    # epilogues: q|k|v as three weights, as one and as q + kv; SwiGLU with I = 5 (a group with one live unit) and I = 4098
    add("qkv-3w", 2080, (256, 256, 256), 4, epi="qkv", strided=True)
    add("qkv-1w", 4128, (768,), 1, epi="qkv", fam="D", norm=True)
    add("qkv-q-kv", 2080, (256, 512), 3, epi="qkv", fam="D", norm=True, ranks=(8, 16), strided=True)
    add("swiglu-I5", 2080, (5, 5), 3, epi="swiglu", strided=True)
    add("swiglu-I4098", 64, (4098, 4098), 2, epi="swiglu", fam="D", norm=True)
    add("swiglu-I5-lora", 4128, (5, 5), 4, epi="swiglu", ranks=(8, 24), lscale=0.5, strided=True)
    # LoRA: one lane, three lanes, eight lanes; one segment and three with unequal ranks; on the dense family the sum is not a bf16, so
    # where the adapter joins matters
    for r in (8, 24, 64):
        add(f"lora-r{r}", 2080, (37,), 1 + (r // 8) % 4, ranks=(r,), lscale=0.5 if r == 64 else 2.0, epi="res" if r == 24 else "none", strided=r == 8)
    add("lora-r8-24-16", 2080, (8, 12, 9), 2, ranks=(8, 24, 16), strided=True, epi="res")
    add("lora-dense-r8-24-64", 4128, (8, 12, 9), 4, fam="D", norm=True, ranks=(8, 24, 64), lscale=0.5)
    add("lora-dense-r24", 2048, (37,), 2, fam="D", ranks=(24,), lscale=0.5)
    # rows per pass: every class with residual and with q|k|v, LoRA on both
    for K, Ms in ((2080, (3, 4)), (14368, (2, 3, 4))):
        for M in Ms:
            tag = f"{pass_class(K, M)}-K{K}-M{M}"
            fam = "D" if M % 2 else "P"
            add(f"{tag}-res", K, (8, 5), M, epi="res", fam=fam, norm=fam == "D", ranks=(8, 16), strided=True)
            add(f"{tag}-qkv", K, (256, 256, 256), M, epi="qkv", fam="D", norm=M != 3, ranks=(16, 8, 24), lscale=0.5, strided=M == 4)
    return cs


CASES = {c.id: c for c in _table()}
assert len(CASES) == len(_table())
# (message, K, M, rank): LlxError before any launch
REJECTS = (("K too large for the LDS stage", 30752, 1, 0), ("multiple of 32", 2064, 1, 0), ("outside 1..4", 2080, 5, 0),
           ("ranks must be multiples of 8, at most 512", 2080, 1, 520))


# ------------------------------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=16)
def build(cid: str) -> dict:
    """The CPU operands of a case.  Strided operands are views; their ._base holds the gaps."""
    c = CASES[cid]
    M, K, N = c.M, c.K, c.N
    bcols = boundary_cols(K)
    d = {"case": c}
    if c.fam == "P":
        x = torch.zeros(M, K)
        for m in range(M):
            rest = [b for b in bcols if b != K - 1]
            cols = [K - 1] + [rest[(3 * m + j) % len(rest)] for j in range(min(3, len(rest)))]
            sign = (O.randint(f"mx_xs_{cid}_{m}", (4,), 0, 2) * 2 - 1).float()
            for col, v in zip(cols, sign):
                x[m, col] = v
    elif c.norm:
        x = (O.randint(f"mx_x_{cid}", (M, K), 0, 2) * 2 - 1).float()
    else:
        x = O.randint(f"mx_x_{cid}", (M, K), -2, 3).float()
    xv = _slice(M, K, 8, 16, float("nan")) if c.strided else torch.empty(M, K, dtype=BF16)
    xv.copy_(x)
    d["x"] = xv
    if c.norm:
        assert c.fam == "D"
        nw = (O.randint(f"mx_nw_{cid}", (K,), 0, 2) * 2 - 1) * (1 + O.randint(f"mx_nw2_{cid}", (K,), 0, 2))
        d["norm_w"] = nw.float().to(BF16)
    # ---- weights: random codes (all 16), scale bytes in {126, 127, 128}, neighbouring blocks and rows differing; row-strided views
    ws, scs = [], []
    for s, n in enumerate(c.ns):
        codes = O.randint(f"mx_w_{cid}_{s}", (n, K), 0, 16).to(torch.uint8)
        # (block kb, row r) -> 126 + (kb + 2 r + s) % 3: the next block and the next row always carry another scale
        sb = (126 + (torch.arange(K // BLOCK)[None, :] + 2 * torch.arange(n)[:, None] + s) % 3).to(torch.uint8)
        if c.strided:
            wb = torch.full((n, K // 2 + 16 * (s + 1)), 0x7F, dtype=torch.uint8)
            sv = torch.full((n, K // BLOCK + 3 + s), 0xFF, dtype=torch.uint8)
            w, sc = wb[:, :K // 2], sv[:, :K // BLOCK]
        else:
            w, sc = torch.empty(n, K // 2, dtype=torch.uint8), torch.empty(n, K // BLOCK, dtype=torch.uint8)
        w.copy_(_pack(codes))
        sc.copy_(sb)
        ws.append(w)
        scs.append(sc)
    d["ws"], d["scales"] = ws, scs
    if c.ranks:
        R = sum(c.ranks)
        t = torch.zeros(M, R)
        off = 0
        for s, r in enumerate(c.ranks):
            at = sorted({p for p in (0, 7, 8, 23, r - 1) if p < r})
            sg = O.randint(f"mx_t_{cid}_{s}", (M, len(at)), -1, 2)
            sg[:, -1] = sg[:, -1] + (sg[:, -1] == 0)  # rank r - 1 always carries something
            for j, p in enumerate(at):
                t[:, off + p] = sg[:, j].float()
            off += r
        tv = _slice(M, R, 8, 8, float("nan")) if c.strided else torch.empty(M, R, dtype=BF16)
        tv.copy_(t)
        d["t"] = tv
        d["bext"] = [O.randint(f"mx_b_{cid}_{s}", (n, r), -3, 4).float().to(BF16).contiguous() for s, (n, r) in enumerate(zip(c.ns, c.ranks))]
    if c.epi == "res":
        r = O.randint(f"mx_r_{cid}", (M, N), -128, 129).float() / 4
        rv = _slice(M, N, 1, 2, float("nan")) if c.strided else torch.empty(M, N, dtype=BF16)
        rv.copy_(r)
        d["res"] = rv
    if c.epi == "qkv":
        pick = O.randint(f"mx_rope_{cid}", (M, 64), 0, len(ROPE_PAIRS))
        d["rope"] = torch.tensor(ROPE_PAIRS)[pick].float().contiguous()  # [M, 64, 2]
        kvh, smax = (N - 256) // 256, 9
        for name in ("kc", "vc"):  # [1, KVH, Smax, 128] views of [1, Smax, KVH, 160]
            d[name] = torch.full((1, smax, kvh, 160), SENTINEL, dtype=BF16).permute(0, 2, 1, 3)[..., :128]
        d["pos"] = torch.tensor([5, 2, 7, 0][:M], dtype=torch.int64)
    off = (4 if c.epi == "qkv" else 3) if c.strided else 0
    d["out"] = _slice(M, c.n_out, off, 8 - off if c.strided else 0, SENTINEL)
    return d


# ------------------------------------------------------------------------------------------------------------------------ reference
FAULTS = ("nibbles_swapped", "neighbour_block_scale", "scale_row_plus1", "last_block_dropped", "sign_ignored", "adapter_after_round",
          "seg1_from_seg0")


def _weights64(d: dict, fault):
    """float64 images of the case's weights, as a kernel with `fault` would see them."""
    out = []
    for s, (w, sc) in enumerate(zip(d["ws"], d["scales"])):
        if fault == "seg1_from_seg0" and s == 1:
            w, sc = d["ws"][0], d["scales"][0]
        w, sc = w.contiguous(), sc.contiguous()
        if fault == "nibbles_swapped":
            w = (w >> 4) | ((w & 15) << 4)
        if fault == "neighbour_block_scale":
            sc = sc[:, torch.arange(1, sc.shape[1] + 1).clamp(max=sc.shape[1] - 1)]
        if fault == "scale_row_plus1":
            sc = sc[torch.arange(1, sc.shape[0] + 1).clamp(max=sc.shape[0] - 1)]
        img = dequantize64(w, sc)
        if fault == "last_block_dropped":
            img[:, -BLOCK:] = 0
        if fault == "sign_ignored":
            img = img.abs()
        out.append(img)
    return out


def reference(d: dict, fault: str = None) -> dict:
    """float64 evaluation with the kernel's rounding points: out [M, n_out] bf16 (SwiGLU: also h64, g, u) and for q|k|v the expected
    cache buffers kc, vc.  fault: what a kernel with that defect would return instead."""
    c = d["case"]
    assert fault is None or fault in FAULTS
    exact = fault is None
    M, K, N = c.M, c.K, c.N
    x = d["x"].double()
    if c.norm:
        w = d["norm_w"].double()
        rstd = 1.0 / torch.sqrt(x.pow(2).mean(1, keepdim=True) + EPS)
        xn = rbf(x * rstd * w)
        assert torch.equal(x.pow(2).mean(1), torch.ones(M, dtype=torch.float64)) and torch.equal(xn, x * w)
        assert torch.equal(rbf(x * (rstd * (1 + 2.0 ** -10)) * w), xn) and torch.equal(rbf(x * (rstd * (1 - 2.0 ** -10)) * w), xn)
    else:
        xn = x
    assert xn.abs().max() <= 2 and torch.equal(xn, xn.round())
    imgs = _weights64(d, fault)
    if exact:
        for img in imgs:
            assert img.abs().max() <= 12 and torch.equal(img * 4, (img * 4).round())
    S = torch.cat([(xn @ img.T)[:, :n] for img, n in zip(imgs, c.ns)], 1)
    S = _f32(S, exact, "linear sum")
    if exact and c.fam == "P":
        assert torch.equal(rbf(S), S), "family P: the sum must be a bf16"
    L = None
    if c.ranks:
        t = d["t"].double()
        offs = [sum(c.ranks[:s]) for s in range(len(c.ranks))]
        L = _f32(c.lscale * torch.cat([t[:, o:o + r] @ b.double().T for o, r, b in zip(offs, c.ranks, d["bext"])], 1), exact, "adapter sum")
    if L is None:
        pre = S
    elif fault == "adapter_after_round":
        pre = _f32(rbf(S) + L, False, "")
    else:
        pre = _f32(S + L, exact, "sum + adapter")
    v = rbf(pre)
    out = {}
    if c.epi == "none":
        o = v
    elif c.epi == "res":
        o = rbf(_f32(v + d["res"].double(), exact, "linear + residual"))
    elif c.epi == "swiglu":
        I = c.ns[0]
        g, u = v[:, :I], v[:, I:]
        out["g"], out["u"] = g.to(BF16), u.to(BF16)
        out["h64"] = rbf(g * torch.sigmoid(g)) * u
        o = rbf(out["h64"])
    else:
        rope = d["rope"].double()
        n_q, n_k = 256, (N - 256) // 2
        y = v.clone()
        pairs = v[:, :n_q + n_k].reshape(M, -1, 64, 2)
        cs, sn = rope[:, None, :, 0], rope[:, None, :, 1]
        y0 = _f32(pairs[..., 0] * cs - pairs[..., 1] * sn, exact and c.fam == "P", "rotation")
        y1 = _f32(pairs[..., 1] * cs + pairs[..., 0] * sn, exact and c.fam == "P", "rotation")
        y[:, :n_q + n_k] = rbf(torch.stack([y0, y1], -1)).reshape(M, n_q + n_k)
        o = y[:, :n_q]
        for name, lo in (("kc", n_q), ("vc", n_q + n_k)):
            base = d[name]._base.clone()
            view = base.permute(0, 2, 1, 3)[..., :128]
            for m in range(M):
                view[0, :, d["pos"][m]] = y[m, lo:lo + n_k].reshape(-1, 128).to(BF16)
            out[name] = base
    out["out"] = o.to(BF16)
    if fault is None:
        assert not (out["out"].float() == SENTINEL).any()
    return out


# fault -> the cases aimed at its class
FAULT_CASES = {
    "nibbles_swapped": ("K32", "K2080", "seg-8-8"),
    "neighbour_block_scale": ("K64", "K4128", "N1"),
    "scale_row_plus1": ("K2048", "N8192", "seg-4-8-5"),
    "last_block_dropped": ("K32", "K2080", "K4128", "K14336"),
    "sign_ignored": ("K2048", "K64-norm", "swiglu-I5"),
    "adapter_after_round": ("lora-dense-r24", "lora-dense-r8-24-64"),
    "seg1_from_seg0": ("seg-8-8", "seg-8-3", "qkv-3w"),
}
