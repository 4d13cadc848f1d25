"""Cases and host restatements for the sampler's penalties and token log-probabilities (llx/sampling.py rule 0, csrc/sample.hip:
llx_sample_rows_ext).

penalize() is rule 0 in fp32, one torch op per IEEE operation and in the rule's order; the divisor and the factors are full tensors, as
in sampling_cases.z_of, so that no scalar-reciprocal shortcut enters.  Because the penalty is exact fp32 and everything the sampler does
after its per-element weight is integer arithmetic, the extended sampler on (logits, counts, penalties) must return the very bits the
plain sampler returns on the host-penalised fp32 row: no tolerance anywhere except on the log-probability (beam_cases.SCORE_TOL).

Counts.  One pattern for every case: per row 3 / 1 / 2 on its three largest logits, and 10 % of the other tokens at 1 .. 5 from a seeded
generator.  CONDITION (tests/test_sampling_penalty_cases.py): with the default penalties the penalised greedy pick differs from the plain
one in >= 90 % of the rows of every shape used on the GPU, so a kernel that ignores the counts cannot pass.
"""
import torch

from tests import sampling_cases as C

THETA, ALPHA_P, ALPHA_F = 1.3, 0.5, 0.25
PENALTIES = dict(repetition_penalty=THETA, presence_penalty=ALPHA_P, frequency_penalty=ALPHA_F)
# the shapes of the GPU test, by name from sampling_cases.SHAPE; v128256 only takes part in CONDITION
GPU_SHAPES = ("v1000", "v1001_stride1003", "v4100_f32", "v8197", "v1000_ties", "v128256_row")
CONDITION_SHAPES = GPU_SHAPES + ("v128256",)
POINTS = ((0, 1.0, 0.7), (50, 0.9, 1.0), (0, 1e-6, 1.0))  # (top_k, top_p, temperature); greedy is run beside them


def penalize(row: torch.Tensor, counts: torch.Tensor, theta: float, alpha_p: float, alpha_f: float) -> torch.Tensor:
    """Rule 0 on a row (or [R, V] rows) of logits with int32 counts of the same shape -> fp32.  Elements with count 0 keep their bits."""
    x = row.float()
    th = torch.full_like(x, theta)
    y = torch.where(x > 0, x / th, x * th)
    t = torch.full_like(x, alpha_f) * counts.float()
    t = torch.full_like(x, alpha_p) + t
    y = y - t
    return torch.where(counts > 0, y, x)


def logprob64(row: torch.Tensor, token: int) -> float:
    """(l_tok - l_max) - log sum exp(l - l_max) on the raw row in fp64."""
    x = row.double()
    m = x.max()
    return float((x[token] - m) - torch.log(torch.exp(x - m).sum()))


def make_counts(name: str, x: torch.Tensor) -> torch.Tensor:
    """int32 [R, V] for the case `name` with logits x: the pattern of the module docstring."""
    R, V = x.shape
    g = torch.Generator().manual_seed(20_000 + [s.name for s in C.SHAPES].index(name))
    some = torch.rand(R, V, generator=g) < 0.1
    counts = torch.where(some, torch.randint(1, 6, (R, V), generator=g), torch.zeros(R, V, dtype=torch.int64))
    top = torch.topk(x.float(), 3, dim=1).indices
    counts.scatter_(1, top, torch.tensor([3, 1, 2]).expand(R, 3))
    return counts.to(torch.int32)


def lowest_argmax(x: torch.Tensor) -> torch.Tensor:
    xf = x.float()
    return torch.stack([(row == row.max()).nonzero()[0, 0] for row in xf])


def strided_counts(counts: torch.Tensor, ldc: int, dev) -> torch.Tensor:
    """The table on `dev` as an [R, V] view with row stride ldc >= V (the padding holds -1: a kernel that reads it penalises nothing
    with it, one that writes it is caught)."""
    R, V = counts.shape
    buf = torch.full((R, ldc), -1, dtype=torch.int32, device=dev)
    buf[:, :V] = counts.to(dev)
    return buf
