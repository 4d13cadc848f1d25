"""Host side of the token sampler (csrc/sample.hip): the counter-based uniform and the checks on the sampling parameters.

Pure Python, no device needed.  The rules the kernel implements, all independent of any sort order and of how ties are arranged:

1. temperature == 0: the argmax of the fp32 logits, lowest index among ties.
2. otherwise z = logit / temperature in fp32; everything starts kept; a logit of -inf is never drawn.
3. top_k > 0: with t the k-th largest z (duplicates counted), keep z >= t - ties at t all stay; top_k >= V is off.
4. top_p < 1: with w = exp(z - z_max) over the kept set and W its sum, keep i iff the weight of {j: z_j > z_i} is < top_p * W.
5. draw: walk the kept tokens by ascending index; the first whose running weight exceeds u * W (W over the final kept set).
6. u = uniform(seed, pos, row) below: a multiple of 2^-24 in [0, 1), exact in fp32.
"""
from __future__ import annotations

from ._lib import LlxError

_M64 = (1 << 64) - 1


def _mix(x: int) -> int:
    """splitmix64 finaliser in uint64 arithmetic."""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def uniform(seed: int, pos: int, row: int) -> float:
    """The uniform the kernel draws for (seed, counter pos, row of the call): float(mix(mix(mix(seed) ^ pos) ^ row) >> 40) * 2^-24."""
    h = _mix(_mix(_mix(int(seed) & _M64) ^ (int(pos) & _M64)) ^ (int(row) & _M64))
    return (h >> 40) * 2.0 ** -24


def check_params(temperature: float, top_k: int, top_p: float, seed: int = 0) -> None:
    """Raise LlxError for sampling parameters the kernel would reject (before anything is launched)."""
    if not (isinstance(temperature, (int, float)) and temperature >= 0 and temperature == temperature and temperature != float("inf")):
        raise LlxError(f"temperature={temperature!r} must be a finite number >= 0 (0 = greedy)")
    if not (isinstance(top_k, int) and not isinstance(top_k, bool) and top_k >= 0):
        raise LlxError(f"top_k={top_k!r} must be an integer >= 0 (0 = off)")
    if not (isinstance(top_p, (int, float)) and 0 < top_p <= 1):
        raise LlxError(f"top_p={top_p!r} must lie in (0, 1] (1 = off)")
    if not (isinstance(seed, int) and 0 <= seed <= _M64):
        raise LlxError(f"seed={seed!r} must be an unsigned 64-bit integer")
