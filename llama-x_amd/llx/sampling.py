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


# ---- prompt-lookup drafting: the host reference of csrc/lookup.hip (generate(draft_tokens=k)); pure lists of ints
def lookup_draft(seq: list, g: int, k: int) -> list:
    """k draft tokens for the continuation of `seq`: for gg = g .. 1 (shorter than seq) the most recent earlier occurrence of the last gg
    tokens, seq[j : j + gg] == seq[-gg:] with j + gg <= len(seq) - 1; the first gg that has one wins, so a longer n-gram beats a more
    recent shorter one.  The draft is what followed it, read from seq extended by the draft so far: an occurrence that overlaps the tail
    continues periodically.  Without any match the last token is repeated."""
    L = len(seq)
    for gg in range(g, 0, -1):
        if gg >= L:
            continue
        for j in range(L - gg - 1, -1, -1):
            if seq[j : j + gg] == seq[L - gg :]:
                ext = list(seq)
                for i in range(k):
                    ext.append(ext[j + gg + i])
                return ext[L:]
    return [seq[-1]] * k


def lookup_accept(fed: list, picks: list, k: int, eos_id, room: int) -> tuple:
    """(emitted tokens, finished) of a step that fed `fed` = [last token, k draft tokens] and whose k + 1 logits rows have the greedy
    picks `picks`: with a the longest prefix of the draft that the picks confirm (fed[1 + i] == picks[i]), picks[0 .. a] are emitted,
    cut to `room` tokens (>= 1) and after the first `eos_id` (None or -1: none) among them, which sets finished."""
    a = 0
    while a < k and fed[1 + a] == picks[a]:
        a += 1
    out = list(picks[: min(a + 1, room)])
    if eos_id is not None and eos_id >= 0 and eos_id in out:
        return out[: out.index(eos_id) + 1], True
    return out, False
