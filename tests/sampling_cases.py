"""Cases, fp64 restatement and acceptance rule for the token sampler (csrc/sample.hip, llx.kernels.sample, llx/sampling.py).

The semantics (llx/sampling.py, rules 1-6) never mention an order among equal values, so the restatement groups equal values with
torch.unique and a parallel kernel can agree with it however it arranges ties.

Acceptance.  The kernel sums up to 2^17 fp32 weights; a pairwise fp32 sum of 2^17 terms is off by at most (17 + 3) 2^-24 ~ 1.2e-6
relative, expf by a few ulp more.  EPS = 1e-5 (relative to W) is about 8x the two together.  With S_>(t) / S_>=(t) the share of the
weight strictly above / at or above a value t (over the set top-k leaves):

  * a top-p threshold t is ACCEPTABLE iff it is a value present in the row, S_>(t) < top_p + EPS and S_>=(t) >= top_p - EPS;
    the top-k threshold is integer-exact and must match exactly;
  * given the reported threshold, a token i is ACCEPTABLE iff it is kept (z_i >= t, logit_i > -inf) and
    u lies in [C_{i-1} - EPS, C_i + EPS], C the fp64 running sum over the kept tokens in index order divided by its total.

So that the rule cannot hide a wrong kernel behind EPS, tests/test_sampling_cases.py checks on these very cases that at least 90 % of
the rows of each top-p case have exactly ONE acceptable threshold and that with top_k <= 50 the smallest kept probability is > 100 EPS.

Shapes.  The kernel walks a row as 16-byte chunks on the 16-byte grid of memory, 1024 chunks (8192 bf16 / 4096 fp32 elements) per
round of its draw scan, and peels the first and the last chunk.  The table therefore has: V below one chunk row (1000, 1001, 1024),
rows that start at every element offset of the grid (V 1001 with row stride 1003), one partial round (4100 bf16), a round boundary
crossed by an odd tail (4100 fp32 = 2 rounds, 8197 bf16 = 2 rounds, 20 011 fp32 = 5 rounds), and the 16 rounds of a Llama-3 row
(128 256).  There is no dispatch on R: 1, 3 and 64 rows (and 8192 in the statistical test) only vary the grid.
"""
import math
from dataclasses import dataclass

import torch

from oracle import ref as O

EPS = 1e-5
BF16 = torch.bfloat16


@dataclass(frozen=True)
class Shape:
    name: str
    V: int
    R: int
    scale: float
    dtype: torch.dtype = BF16
    stride: int = 0       # row stride in elements (0 = V)
    offset: int = 0       # elements in front of the first row (moves every row off the 16-byte grid)
    quantum: float = 0.0  # > 0: logits rounded to multiples of it (ties everywhere, also at the top)
    points: tuple = ()    # () = the whole grid PARAMS; otherwise exactly these (top_k, top_p, temperature) points


TOP_KS = (0, 1, 50, 1 << 20)      # off, greedy-like, a usual value, >= V (off)
TOP_PS = (1.0, 0.9, 1e-6)
TEMPS = (0.7, 1.0)
PARAMS = [(k, p, t) for k in TOP_KS for p in TOP_PS for t in TEMPS]

# Every shape class runs the WHOLE grid.  The scale of each case's logits is chosen so that CONDITION (below) holds on all 24 points:
# sharp enough that a top-p threshold is unique, flat enough that the 50th token still has a probability far above EPS.
SHAPES = [
    Shape("v1000", 1000, 64, 1.0),
    Shape("v1001_stride1003", 1001, 64, 1.25, stride=1003, offset=3),   # rows start at every element offset of the 16-byte grid
    Shape("v1024", 1024, 3, 2.0),
    Shape("v4100", 4100, 64, 1.0),
    Shape("v4100_f32", 4100, 3, 3.0, dtype=torch.float32, stride=4101, offset=1),  # fp32: two draw rounds, rows off the grid
    Shape("v8197", 8197, 3, 2.0),                                       # bf16: the round boundary crossed by a 5-element tail
    Shape("v1000_f32", 1000, 1, 2.0, dtype=torch.float32),
    Shape("v20011_f32", 20011, 3, 2.0, dtype=torch.float32, stride=20013, offset=2, quantum=0.0625),  # fp32: five draw rounds, odd tail
    Shape("v1000_ties", 1000, 64, 1.25, quantum=0.25),                  # ties at every threshold, the top-k one included
    Shape("v128256", 128_256, 3, 2.0),
    Shape("v128256_row", 128_256, 1, 2.0),
    # the two sharp rows of the issue's condition table, as top-p cases of their own: at these scales the 50th token's probability
    # falls to 2e-5 .. 6e-4, below the 100 EPS of CONDITION, so top_k = 50 runs on the flatter rows of the same V above instead
    Shape("v1000_sharp", 1000, 64, 2.0, points=tuple((k, p, t) for k, p, t in PARAMS if k != 50)),
    Shape("v4100_sharp", 4100, 64, 3.0, points=tuple((k, p, t) for k, p, t in PARAMS if k != 50) + ((0, 0.5, 1.0),)),
]
SHAPE = {s.name: s for s in SHAPES}


def params_for(s: Shape) -> list:
    """The (top_k, top_p, temperature) points of a case: the whole grid unless the case lists its own."""
    return list(s.points) if s.points else list(PARAMS)


# CONDITION (tests/test_sampling_cases.py): on every point of every case, >= 90 % of the rows have exactly one acceptable top-p threshold
# and with 0 < top_k <= 50 the smallest kept probability is > 100 EPS.  The issue's own rows, checked by name as well:
CONDITION_TOP_P = [("v128256", 1.0, 0, 0.9), ("v128256", 0.7, 0, 0.9), ("v1000_sharp", 1.0, 0, 0.9), ("v4100_sharp", 1.0, 0, 0.5)]
CONDITION_TOP_K = [("v128256", 1.0, 50)]


def make_logits(s: Shape) -> torch.Tensor:
    """The [R, V] view of the case (CPU): randn * scale in the case's dtype inside a buffer with the case's row stride and offset."""
    stride = s.stride or s.V
    x = O.randn("sampling_" + s.name, (s.R, s.V), s.scale)
    if s.quantum:
        x = torch.round(x / s.quantum) * s.quantum
    buf = torch.zeros(s.offset + s.R * stride, dtype=s.dtype)
    view = buf[s.offset:].view(s.R, stride)[:, : s.V]
    view.copy_(x.to(s.dtype))
    return view


def to_device(view: torch.Tensor, s: Shape, dev) -> torch.Tensor:
    """The same view (same stride and offset) on the device."""
    stride = s.stride or s.V
    buf = torch.zeros(s.offset + s.R * stride, dtype=s.dtype, device=dev)
    out = buf[s.offset:].view(s.R, stride)[:, : s.V]
    out.copy_(view)
    return out


def z_of(row: torch.Tensor, temperature: float) -> torch.Tensor:
    """z = logit / temperature in fp32 (a true division, as the kernel's), then exact in fp64; -0 folded onto +0."""
    x = row.float()
    z = x / torch.full_like(x, temperature)
    return z.double() + 0.0


class Row:
    """fp64 analysis of one row under (temperature, top_k): the distinct values in ascending order, how often each occurs, the
    weight of each group, and the set top-k leaves."""

    def __init__(self, row: torch.Tensor, temperature: float, top_k: int, *, mutant: str = ""):
        self.logits = row.float()
        self.V = row.numel()
        self.T = temperature
        self.z = z_of(row, temperature)
        self.values, self.inverse, self.counts = torch.unique(self.z, return_inverse=True, return_counts=True)
        self.zmax = self.values[-1]
        self.gw = torch.exp(self.values - self.zmax) * self.counts  # weight of each group of equal values (exp(-inf) = 0)
        self.mutant = mutant
        cnt_ge = torch.flip(torch.cumsum(torch.flip(self.counts, [0]), 0), [0])  # elements >= each value
        self.cnt_ge = cnt_ge
        self.g_k = 0  # lowest group top-k keeps
        if 0 < top_k < self.V:
            self.g_k = int((cnt_ge >= top_k).nonzero().max())
        self.top_k = top_k

    # ---- shares of the weight of the top-k set
    def shares(self):
        gw = self.gw.clone()
        gw[: self.g_k] = 0
        W = gw.sum()
        ge = torch.flip(torch.cumsum(torch.flip(gw, [0]), 0), [0])
        return (ge - gw) / W, ge / W  # S_>, S_>= per group

    def group_of_logit(self, thresh: float) -> int:
        """Group index of the value a raw logit maps to, or -1 if no element of the row has that value."""
        zt = z_of(torch.tensor([thresh], dtype=torch.float32), self.T)[0]
        g = int(torch.searchsorted(self.values, zt))
        return g if g < self.values.numel() and self.values[g] == zt else -1

    def exact_group(self, top_p: float) -> int:
        """The lowest group the rules keep."""
        g = self.g_k
        if top_p < 1:
            s_gt, s_ge = self.shares()
            keep = (s_ge < top_p) if self.mutant == "top_p_ge" else (s_gt < top_p)  # the mutant sums over z_j >= z_i
            keep[: self.g_k] = False
            keep[-1] = True
            g = int(keep.nonzero().min())
        return g

    def acceptable_groups(self, top_p: float) -> list[int]:
        if top_p >= 1:
            return [self.g_k]
        s_gt, s_ge = self.shares()
        ok = (s_gt < top_p + EPS) & (s_ge >= top_p - EPS)
        ok[: self.g_k] = False
        return ok.nonzero().flatten().tolist()

    def threshold_acceptable(self, top_p: float, thresh: float) -> bool:
        g = self.group_of_logit(thresh)
        if g < 0 or g not in self.acceptable_groups(top_p):
            return False
        return float(self.logits[self.inverse == g].min()) == float(thresh)  # the RAW logit of the smallest kept token

    def count_at(self, thresh: float) -> int:
        g = self.group_of_logit(thresh)
        return int(self.cnt_ge[g]) if g >= 0 else -1

    def kept_mask(self, g: int) -> torch.Tensor:
        keep = self.inverse >= g
        if self.mutant == "top_k_exact" and g == self.g_k and 0 < self.top_k < self.V:
            # keeps exactly k: of the ties at the threshold only the first ones by index
            above = int(self.cnt_ge[g] - self.counts[g])
            tie = (self.inverse == g).nonzero().flatten()
            keep[tie[self.top_k - above:]] = False
        return keep

    def running(self, g: int):
        w = torch.exp(self.z - self.zmax) * self.kept_mask(g)
        C = torch.cumsum(w, 0)
        return w, C, C[-1]

    def draw(self, g: int, u: float) -> int:
        w, C, W = self.running(g)
        hit = ((C - w) > u * W) if self.mutant == "scan_off_by_one" else (C > u * W)
        hit &= self.kept_mask(g)
        if bool(hit.any()):
            return int(hit.nonzero().min())
        return int(self.kept_mask(g).nonzero().max())

    def draw_many(self, g: int, us: torch.Tensor) -> torch.Tensor:
        """draw() for many uniforms on this one row."""
        w, C, W = self.running(g)
        kept = self.kept_mask(g).nonzero().flatten()
        j = torch.searchsorted(C[kept].contiguous(), us.double() * W, right=True)  # first kept index with C > u W
        return kept[j.clamp_max(kept.numel() - 1)]

    def token_acceptable(self, thresh: float, token: int, u: float) -> bool:
        g = self.group_of_logit(thresh)
        if g < 0 or not (0 <= token < self.V) or int(self.inverse[token]) < g or self.logits[token] == -math.inf:
            return False
        w, C, W = self.running(g)
        lo = float((C[token] - w[token]) / W) - EPS
        hi = float(C[token] / W) + EPS
        return lo <= u <= hi


def restate_row(r: Row, top_p: float, u: float):
    """(token, raw threshold logit, kept count) by rules 2-6 in fp64 on an analysed row."""
    g = r.exact_group(top_p)
    thresh = float(r.logits[r.inverse == g].min())
    kept = int(r.kept_mask(g).sum())
    return r.draw(g, u), thresh, kept


def restate(row: torch.Tensor, temperature: float, top_k: int, top_p: float, u: float, *, mutant: str = ""):
    """(token, raw threshold logit, kept count) by rules 1-6 in fp64."""
    if temperature == 0:
        x = row.float()
        m = x.max()
        tie = (x == m).nonzero().flatten()
        return int(tie[0]), float(m), int(tie.numel())
    return restate_row(Row(row, temperature, top_k, mutant=mutant), top_p, u)


def accepts_row(r: Row, top_p: float, u: float, token: int, thresh: float, kept: int) -> list[str]:
    """The acceptance rule on one row's result: the list of what is wrong with it (empty = accepted)."""
    bad = []
    if not r.threshold_acceptable(top_p, thresh):
        bad.append(f"threshold {thresh} not acceptable (acceptable groups {r.acceptable_groups(top_p)}, reported {r.group_of_logit(thresh)})")
        return bad
    if kept != r.count_at(thresh):
        bad.append(f"kept {kept} != count at the threshold {r.count_at(thresh)}")
    if not r.token_acceptable(thresh, token, u):
        bad.append(f"token {token} not acceptable for u={u}")
    return bad


def accepts(row: torch.Tensor, temperature: float, top_k: int, top_p: float, u: float, token: int, thresh: float, kept: int) -> list[str]:
    return accepts_row(Row(row, temperature, top_k), top_p, u, token, thresh, kept)


def stat_bound(R: int, p: float) -> float:
    """Allowed |count - R p| for a token of probability p over R independent draws: six binomial standard deviations + 1."""
    return 6.0 * math.sqrt(R * p * (1.0 - p)) + 1.0


# ---- the statistical case: R rows of the SAME logits, top_k = 8, counter = row index, one launch
STAT_R, STAT_V, STAT_TOP_K, STAT_SEED = 8192, 1000, 8, 7


def stat_logits() -> torch.Tensor:
    return O.randn("sampling_stat", (STAT_V,), 2.0).to(BF16)


def stat_uniforms() -> torch.Tensor:
    from llx.sampling import uniform

    return torch.tensor([uniform(STAT_SEED, r, r) for r in range(STAT_R)], dtype=torch.float64)


def stat_check(tokens: torch.Tensor) -> list[str]:
    """Every token in the top 8, every count within stat_bound of R p (p the renormalised fp64 probability)."""
    r = Row(stat_logits(), 1.0, STAT_TOP_K)
    w, _, W = r.running(r.g_k)
    bad = []
    tokens = tokens.cpu()
    kept = r.kept_mask(r.g_k)
    if not bool(kept[tokens].all()):
        bad.append("tokens outside the top-k set")
    counts = torch.bincount(tokens, minlength=STAT_V)
    for i in kept.nonzero().flatten().tolist():
        p = float(w[i] / W)
        if abs(int(counts[i]) - STAT_R * p) > stat_bound(STAT_R, p):
            bad.append(f"token {i}: count {int(counts[i])} vs {STAT_R * p:.1f} +- {stat_bound(STAT_R, p):.1f}")
    return bad
