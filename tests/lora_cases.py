"""LoRA / DoRA rank cases: one per execution plan the group planner (llx.ops.GroupPlan) and the skinny kernels distinguish, and the
CPU-side arithmetic that goes with them.

Rank is not a passive size here.  A group of linears that read the same input (q|k|v, gate|up) runs FUSED - one GEMM over the
concatenated weights with one 64-wide block-diagonal K-extension - only while the members' ranks sum to 64 or less, all members are
adapted and they share alpha / rank.  Otherwise every member runs its own LinearPlan into a column slice of the group's buffer, RoPE /
SwiGLU run stand-alone, and the data gradient is summed in place (the residual epilogue reading the buffer it writes).  Inside the
skinny kernels ceil(R / 16) picks the register tiling (NB = 1 | 2 | 4; 3 too for the TN product and the fused norm), rows past R are
clamped and zeroed, and whether the member boundaries are multiples of 64 / 256 decides between the ranged / segment forms and the
dense ones.  `CASES` names one configuration per class with the plan facts it is meant to reach (tests/test_lora_cases.py asserts
them against the planner, so a later change to the planner fails there instead of silently moving a case onto a tested path).

Everything is drawn through the oracle's named generators (oracle.ref.randn): a case is reproducible from its name alone.  alpha = 2 *
rank everywhere (scale 2.0: exact in bf16, never 1, so a forgotten scale shows), and B is drawn wide enough that the adapter carries
about as much of a linear's output as the base product does (`b_std`): a dropped rank column, exchanged members or a lost scale land
far outside the GEMM bar - which `group_math(rounded=True)` and its mutants check on the CPU for every case.
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch

from oracle import ref as O

# smallest config whose q|k|v member boundaries (1024, 1280, 1536) are multiples of 256 - the segment form of skinny_tn and the ranged
# form of skinny_nt are reachable - and whose width the fused norm + adapter projection takes (rmsnorm_skinny_ok(1024))
MID = O.TINY._replace(embed_dim=1024, num_heads=8, num_kv_heads=2, intermediate_dim=2048, num_layers=1)
M_TOK = 320      # B 1, S 320: two 256-row GEMM tiles, the second ragged; 20 skinny row blocks
SCALE = 2.0      # alpha / rank of every adapted linear (the unequal-scale case doubles one member's)
ATTN, MLP = ("attention.wq", "attention.wk", "attention.wv"), ("feed_forward.w1", "feed_forward.w3")
GEMM_RTOL = 2.0 ** -7  # the project's GEMM bar: |got - ref| <= 2^-7 max|ref| + 2^-7 |ref|


def b_std(rank: int) -> float:
    """std of B that puts the adapter's rms share of a linear's output at ~0.85 of the base product's for x ~ N(0, 1), W ~ N(0, 0.02),
    K = 1024 (A as O.init_lora draws it: std 0.577 / sqrt(K), so t = x A^T has std 0.577 and s t B^T std 2 * 0.577 * sqrt(r) * b_std = 0.55
    against the base's 0.02 * sqrt(1024) = 0.64).  At K = 512 .. 2048 the share stays inside [0.5, 2]."""
    return 0.55 / (2 * 0.577 * math.sqrt(rank))


@dataclass(frozen=True)
class Plan:
    """What the planner must make of one group: fused or not, R = sum of ranks, and - for fused groups - whether the ranged form of
    skinny_nt (`_kranges()`) and the segment form of skinny_tn (`_tn_segs()`) apply (None = does not: the dense forms run)."""
    fused: bool
    R: int
    kranges: Optional[bool] = None
    segs: Optional[bool] = None

    @property
    def nb(self) -> int:
        """16-row blocks the skinny kernels size their registers for (NT kernels round 3 up to 4)."""
        return -(-self.R // 16)


@dataclass(frozen=True)
class Case:
    name: str
    qkv: tuple                      # ranks of wq, wk, wv (0: left a plain frozen nn.Linear)
    rest: int                       # rank of wo, w1, w3, w2
    qkv_alpha_mult: tuple = (1, 1, 1)  # alpha = 2 * rank * mult
    mid: tuple = ()                 # (Plan of q|k|v, Plan of gate|up) at MID dims
    tiny: tuple = ()                # ... at O.TINY dims: member boundaries at multiples of 64 but not of 256 -> no segment form

    def rank(self, suffix: str) -> int:
        return self.qkv[ATTN.index(suffix)] if suffix in ATTN else self.rest

    def scale(self, suffix: str) -> float:
        return SCALE * (self.qkv_alpha_mult[ATTN.index(suffix)] if suffix in ATTN else 1)

    def group_ranks(self, which: str) -> tuple:
        return self.qkv if which == "qkv" else (self.rest, self.rest)

    def group_scales(self, which: str) -> tuple:
        return tuple(self.scale(s) for s in (ATTN if which == "qkv" else MLP))


def _uniform(r, qkv_mid, gu_mid, qkv_tiny, gu_tiny):
    return Case(f"r{r}", (r, r, r), r, mid=(qkv_mid, gu_mid), tiny=(qkv_tiny, gu_tiny))


def _per_member(R):
    return Plan(False, R)


F, U = Plan, _per_member  # short names for the table below
CASES = {c.name: c for c in (
    # uniform rank r: q|k|v carries 3r, gate|up 2r
    _uniform(1, F(True, 3, True, True), F(True, 2, True, True), F(True, 3, True, False), F(True, 2, True, True)),       # NB 1, rows 1..15 clamped
    _uniform(5, F(True, 15, True, True), F(True, 10, True, True), F(True, 15, True, False), F(True, 10, True, True)),   # odd ranks, element path of the pack
    _uniform(21, F(True, 63, True, True), F(True, 42, True, True), F(True, 63, True, False), F(True, 42, True, True)),  # NB 4 with ONE clamped row; NB 3 in TN
    _uniform(22, U(66), F(True, 44, True, True), U(66), F(True, 44, True, True)),                                       # q|k|v leaves the fused path
    _uniform(32, U(96), F(True, 64, True, True), U(96), F(True, 64, True, True)),                                       # gate|up at R = 64 exactly: no clamp, no zero column
    _uniform(33, U(99), U(66), U(99), U(66)),                                                                           # gate|up leaves it too; odd rank per member
    _uniform(64, U(192), U(128), U(192), U(128)),                                                                       # per-member R = 64
    # q|k|v members that differ (the other linears: rank 16)
    Case("r8-32-8", (8, 32, 8), 16, mid=(F(True, 48, True, True), F(True, 32, True, True)),
         tiny=(F(True, 48, True, False), F(True, 32, True, True))),                    # fused, unequal ranks, wk straddles 16-row blocks
    Case("r16-none-16", (16, 0, 16), 16, mid=(U(32), F(True, 32, True, True)), tiny=(U(32), F(True, 32, True, True))),   # lora_all_or_none
    Case("r16-scales", (16, 16, 16), 16, (1, 2, 1), mid=(U(48), F(True, 32, True, True)),
         tiny=(U(48), F(True, 32, True, True))),                                       # same_scale
)}


def group_dims(cfg, which: str) -> tuple:
    """(K, (N_0, N_1, ...)) of the q|k|v or gate|up group."""
    hq, hkv = cfg.num_heads * cfg.head_dim, cfg.num_kv_heads * cfg.head_dim
    return cfg.embed_dim, ((hq, hkv, hkv) if which == "qkv" else (cfg.intermediate_dim,) * 2)


# --------------------------------------------------------------------------------------------------------------------------------
# one group's data (bf16-exact values held in fp32) and its modules
# --------------------------------------------------------------------------------------------------------------------------------
def _bf(x):
    return x.to(torch.bfloat16).float()


def group_data(case: Case, cfg, which: str, M: int = M_TOK) -> dict:
    """x [M, K], dy [M, sum N], per member W [N, K], A [r, K] | None, B [N, r] | None and its scale - all rounded to bf16."""
    K, Ns = group_dims(cfg, which)
    tag = f"lc_{case.name}_{which}_{K}"
    d = dict(x=_bf(O.randn(tag + "x", (M, K))), dy=_bf(O.randn(tag + "dy", (M, sum(Ns)))), Ns=Ns, K=K, W=[], A=[], B=[],
             s=list(case.group_scales(which)))
    for i, (n, r) in enumerate(zip(Ns, case.group_ranks(which))):
        d["W"].append(_bf(O.randn(f"{tag}w{i}", (n, K), 0.02)))
        d["A"].append(_bf(O.randn(f"{tag}a{i}", (r, K), math.sqrt(2.0 / 6.0) / math.sqrt(K))) if r else None)  # as O.init_lora
        d["B"].append(_bf(O.randn(f"{tag}b{i}", (n, r), b_std(r))) if r else None)
    return d


def probe_B(d: dict, c_of) -> list:
    """B factors that are zero except ONE rank column per member (c_of(r) -> column), drawn at b_std(1): the whole adapter share sits
    in that column, so a clamp or offset error is localised to it."""
    out = []
    for i, b in enumerate(d["B"]):
        if b is None:
            out.append(None)
            continue
        nb = torch.zeros_like(b)
        nb[:, c_of(b.shape[1])] = _bf(O.randn(f"lc_probe_{i}_{b.shape[0]}", (b.shape[0],), b_std(1)))
        out.append(nb)
    return out


def group_modules(d: dict, kind: str = "lora", base: str = "bf16", B=None):
    """The group's nn.Linear modules (CPU, bf16), dressed as the training scripts do: quantise, then adapt (a member without factors
    stays a plain frozen nn.Linear).  DoRA: m = ||W||_row moved off it by a seeded +-10 %."""
    from torch import nn

    from modelling import apply_linear_adapter_
    from subclasses import quantize_linear_

    mods = []
    for i, (w, a, b, s) in enumerate(zip(d["W"], d["A"], B or d["B"], d["s"])):
        m = nn.Linear(d["K"], w.shape[0], bias=False).bfloat16()
        with torch.no_grad():
            m.weight.copy_(w)
        if base != "bf16":
            quantize_linear_(m, "int8", dynamic_int8_act=base == "int8-dynamic")
        if a is None:
            m.weight.requires_grad_(False)
        else:
            apply_linear_adapter_(m, kind, rank=a.shape[0], alpha=s * a.shape[0])
            with torch.no_grad():
                m.lora_a.copy_(a)
                m.lora_b.copy_(b)
                if kind == "dora":
                    m.m.copy_(dora_m(d, i))
        mods.append(m)
    return mods


def dora_m(d: dict, i: int):
    return _bf(d["W"][i].norm(dim=1) * (1 + 0.1 * O.randn(f"lc_m{i}_{d['K']}", (d["W"][i].shape[0],))))


# --------------------------------------------------------------------------------------------------------------------------------
# float64 statements of one group: ground truth, and the product's arithmetic with its rounding points (and mutants of it)
# --------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("drop_last_col", "swap_t", "no_scale", "dx_last_only")


def _r(x, on):
    return x.to(torch.bfloat16).double() if on else x


def group_math(d: dict, rounded: bool = False, fused: bool = True, mutant: Optional[str] = None, B=None) -> dict:
    """y [M, sum N], dx [M, K], dA_i [r, K], dB_i [N, r] of   y_i = x W_i^T + s_i (x A_i^T) B_i^T   in float64.
    rounded=False: exact (the ground truth).  rounded=True: with the product's rounding points - t = x A^T and u = dy B stored in bf16,
    s B and s A^T rounded to bf16 (the K-extension operands), outputs rounded to bf16; an unfused group sums dx member by member, each
    partial sum rounded (`fused=False`).  mutant (with rounded): a structurally wrong product -
      drop_last_col  the last rank of the first adapted member never enters (y, dx, its dA row and dB column)
      swap_t         the t blocks of the first and the last adapted member are exchanged (same rank in every case)
      no_scale       alpha / rank forgotten
      dx_last_only   the in-place accumulation of an unfused group's data gradient lost: dx is the last member's term alone"""
    assert mutant is None or (rounded and mutant in MUTANTS)
    x, dy = d["x"].double(), d["dy"].double()
    Bs = B or d["B"]
    idx = [i for i, a in enumerate(d["A"]) if a is not None]
    ts = {i: _r(x @ d["A"][i].double().T, rounded) for i in idx}
    if mutant == "swap_t":
        i0, i1 = idx[0], idx[-1]
        assert ts[i0].shape == ts[i1].shape
        ts[i0], ts[i1] = ts[i1], ts[i0]
    ys, dxs, dA, dB = [], [], [], []
    off = 0
    for i, (w, a, b, s) in enumerate(zip(d["W"], d["A"], Bs, d["s"])):
        w = w.double()
        n = w.shape[0]
        dyi = dy[:, off : off + n]
        off += n
        y, dxi = x @ w.T, dyi @ w
        if a is None:
            dA.append(None)
            dB.append(None)
        else:
            a, b = a.double(), b.double()
            if mutant == "no_scale":
                s = 1.0
            keep = torch.ones(a.shape[0], dtype=torch.float64)
            if mutant == "drop_last_col" and i == idx[0]:
                keep[-1] = 0
            t = ts[i] * keep
            u = _r(dyi @ b, rounded) * keep
            y = y + t @ _r(s * b, rounded).T
            dxi = dxi + u @ _r(s * a.T, rounded).T
            dA.append(_r(s * (u.T @ x), rounded))
            dB.append(_r(s * (dyi.T @ t), rounded))
        ys.append(_r(y, rounded))
        dxs.append(dxi)
    if mutant == "dx_last_only":
        dx = _r(dxs[-1], True)
    elif fused or not rounded:
        dx = _r(sum(dxs), rounded)
    else:
        dx = _r(dxs[0], True)
        for t_ in dxs[1:]:
            dx = _r(_r(t_, True) + dx, True)  # EPI_RESIDUAL: the bf16 product is added to the bf16 residual
    return dict(y=torch.cat(ys, 1), dx=dx, dA=dA, dB=dB)


def over_bar(got, ref, rtol: float = GEMM_RTOL) -> float:
    """Worst excess of |got - ref| over rtol |ref|, in units of atol = rtol max|ref|: <= 1 passes the bar, 10 is ten times outside."""
    got, ref = got.double(), ref.double()
    return (((got - ref).abs() - rtol * ref.abs()).max() / (rtol * ref.abs().max())).item()


# --------------------------------------------------------------------------------------------------------------------------------
# layer level: adapter factors of a whole TransformerLayer under the oracle's key names
# --------------------------------------------------------------------------------------------------------------------------------
def layer_lora(case: Case, cfg, layer: int = 0) -> dict:
    """lora_a / lora_b of every adapted linear of one layer, named and drawn as O.init_lora does (A) with B at b_std(rank)."""
    D, I = cfg.embed_dim, cfg.intermediate_dim
    hq, hkv = cfg.num_heads * cfg.head_dim, cfg.num_kv_heads * cfg.head_dim
    shapes = {"attention.wq": (hq, D), "attention.wk": (hkv, D), "attention.wv": (hkv, D), "attention.wo": (D, hq),
              "feed_forward.w1": (I, D), "feed_forward.w3": (I, D), "feed_forward.w2": (D, I)}
    p = {}
    for suf, (o, n) in shapes.items():
        r = case.rank(suf)
        if r:
            key = f"layers.{layer}.{suf}"
            p[key + ".lora_a"] = O.randn(key + ".lora_a", (r, n), math.sqrt(2.0 / 6.0) / math.sqrt(n))
            p[key + ".lora_b"] = O.randn(key + ".lora_b", (o, r), b_std(r))
    return p
