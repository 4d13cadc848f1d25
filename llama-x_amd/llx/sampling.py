"""Host side of the token sampler (csrc/sample.hip): the counter-based uniform and the checks on the sampling parameters.

Pure Python, no device needed.  The rules the kernel implements, all independent of any sort order and of how ties are arranged:

0. penalties (llx_sample_rows_ext; off by default): with c_i the int32 count of how often token i has occurred in the row's sequence so
   far and x_i the logit as fp32, an element with c_i == 0 keeps its bits; one with c_i > 0 becomes, every step a single IEEE fp32
   operation in this order and none contracted into an FMA,
     repetition_penalty theta (finite, > 0, 1 = off):  x = x / theta if x > 0 else x * theta   (a true divide, the HF rule; 0 and -inf stay)
     presence_penalty a_p, frequency_penalty a_f (finite, 0 = off, negative allowed):  t = a_f * float(c);  t = a_p + t;  x = x - t.
   Rules 1-6 and the reported threshold treat x as "the logit".  The launch that draws a token adds one to its count.
1. temperature == 0: the argmax of the fp32 logits, lowest index among ties.
2. otherwise z = logit / temperature in fp32; everything starts kept; a logit of -inf is never drawn.
3. top_k > 0: with t the k-th largest z (duplicates counted), keep z >= t - ties at t all stay; top_k >= V is off.
4. top_p < 1: with w = exp(z - z_max) over the kept set and W its sum, keep i iff the weight of {j: z_j > z_i} is < top_p * W.
5. draw: walk the kept tokens by ascending index; the first whose running weight exceeds u * W (W over the final kept set).
6. u = uniform(seed, pos, row) below: a multiple of 2^-24 in [0, 1), exact in fp32.

The log-probability the sampler can report for the chosen token is defined on the RAW logits l - no penalties, temperature 1, nothing
filtered: logp = (l_tok - l_max) - log sum_i exp(l_i - l_max), the formula of beam_shortlist and of Llama.token_logprobs.  It is the
model's probability of the token, comparable across sampling settings; it equals the log-probability under the behaviour policy (the
distribution the token was drawn from) only when temperature == 1 and no filter and no penalty is on.
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


def _finite(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool) and v - v == 0


def check_penalties(repetition_penalty: float, presence_penalty: float, frequency_penalty: float) -> None:
    """Raise LlxError for penalties (rule 0) the kernel would reject (before anything is launched)."""
    if not (_finite(repetition_penalty) and repetition_penalty > 0):
        raise LlxError(f"repetition_penalty={repetition_penalty!r} must be a finite number > 0 (1 = off)")
    if not _finite(presence_penalty):
        raise LlxError(f"presence_penalty={presence_penalty!r} must be a finite number (0 = off)")
    if not _finite(frequency_penalty):
        raise LlxError(f"frequency_penalty={frequency_penalty!r} must be a finite number (0 = off)")


def penalties_on(repetition_penalty: float, presence_penalty: float, frequency_penalty: float) -> bool:
    """True if any of the three penalties would change a logit."""
    return repetition_penalty != 1 or presence_penalty != 0 or frequency_penalty != 0


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


# ---- beam search: the host reference of csrc/beam.hip (generate(num_beams=W)); pure lists of floats and ints
BEAM_DEAD = -1.0e30  # the score of a beam that does not exist yet (beams 1 .. W-1 before the first step): no sum of log-probabilities reaches it


def beam_shortlist(z, W: int) -> list:
    """The W + 1 best tokens of the logits row `z` as (log-probability, token), ordered by (logit descending, token index ascending);
    logp[t] = (z[t] - zmax) - log sum exp(z - zmax).  W + 1 are enough: the walk of beam_step stops at W live picks and a row holds
    one eos_id at most."""
    import heapq
    import math

    zmax = max(z)
    lse = math.log(math.fsum(math.exp(v - zmax) for v in z))
    best = heapq.nsmallest(W + 1, range(len(z)), key=lambda t: (-z[t], t))
    return [((z[t] - zmax) - lse, t) for t in best]


def beam_state(W: int) -> dict:
    """The state of one prompt before the first step: beam 0 alone is live."""
    return dict(s=[0.0] + [BEAM_DEAD] * (W - 1), hist=[[] for _ in range(W)], bank=[], done=False, steps=0)


def _beam_bank(st: dict, W: int, tokens: list, final: float, margins) -> None:
    """A hypothesis enters the bank (slots in order of arrival) if there is room, or in place of the worst one - the lowest final score,
    the lowest slot among equals - if it beats it."""
    bank = st["bank"]
    if len(bank) < W:
        bank.append((list(tokens), final))
        return
    worst = min(range(W), key=lambda i: (bank[i][1], i))
    if margins is not None:
        margins.append(abs(final - bank[worst][1]))
    if final > bank[worst][1]:
        if margins is not None:
            margins.extend(abs(bank[i][1] - bank[worst][1]) for i in range(W) if i != worst)
        bank[worst] = (list(tokens), final)


def beam_step(st: dict, rows, W: int, *, max_new_tokens: int, eos_id=None, length_penalty: float = 1.0, margins=None, used=None) -> list:
    """One step of beam search on the W logits rows `rows` (row r: the logits after beam r's last token; before the first step all rows
    are the prefill's): updates `st` (beam_state) and returns parent[0 .. W-1].

    Every row gives its shortlist (beam_shortlist); all candidates are ordered by (score s[r] + logp descending, row ascending, rank in
    the row's shortlist ascending) and walked: an eos_id becomes a finished hypothesis with the final score score / len ** length_penalty
    (len counts the eos) and is offered to the bank; any other token becomes the next live beam j (parent[j] = r); the walk stops at W
    live beams.  In the first step only row 0 takes part.  done is set when the bank holds W hypotheses or max_new_tokens tokens have
    been generated; the live beams are then offered to the bank as they are, with s / steps ** length_penalty.  A step on a done state
    returns the identity and changes nothing.

    margins (a list) receives the gaps that decide: between consecutive walked candidates up to the first one left out (pairs of equal
    logits of one row aside: their order is the index, exactly), and at the bank between a hypothesis and the worst entry, and between
    the worst and the others when it is replaced.  used (a list) receives the highest shortlist rank the walk touched."""
    if st["done"]:
        return list(range(W))
    n, init = st["steps"] + 1, st["steps"] == 0
    cands = []
    for r in range(1 if init else W):
        for k, (lp, t) in enumerate(beam_shortlist(rows[r], W)):
            cands.append((-(st["s"][r] + lp), r, k, t, rows[r][t]))
    cands.sort(key=lambda c: c[:3])
    parent, s, hist, top = [], [], [], 0
    for i, (neg, r, k, t, z) in enumerate(cands):
        if margins is not None and i > 0 and not (cands[i - 1][1] == r and cands[i - 1][4] == z):
            margins.append(neg - cands[i - 1][0])  # (the scores are stored negated: the gap to the candidate in front)
        if len(parent) == W:
            break
        top = max(top, k)
        if eos_id is not None and t == eos_id:
            _beam_bank(st, W, st["hist"][r] + [t], -neg / n ** length_penalty, margins)
        else:
            parent.append(r)
            s.append(-neg)
            hist.append(st["hist"][r] + [t])
    assert len(parent) == W, "a row holds one eos_id at most: W + 1 candidates per row always give W live beams"
    if used is not None:
        used.append(top)
    st.update(s=s, hist=hist, steps=n)
    if len(st["bank"]) == W or n == max_new_tokens:
        st["done"] = True
        for j in range(W):
            _beam_bank(st, W, hist[j], s[j] / n ** length_penalty, margins)
    return parent


def beam_ranked(st: dict, margins=None) -> list:
    """The bank as [(tokens, final score)], best first (the lower slot among equal scores)."""
    order = sorted(range(len(st["bank"])), key=lambda i: (-st["bank"][i][1], i))
    if margins is not None:
        margins.extend(st["bank"][a][1] - st["bank"][b][1] for a, b in zip(order, order[1:]))
    return [st["bank"][i] for i in order]
