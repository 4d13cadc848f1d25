"""Shared cases and the float64 restatement of the top-k log-probability kernel (csrc/topk.hip), used by the CPU checks of the
restatement itself (tests/test_topk_cases.py) and by the GPU parity tests (tests/test_topk_gpu.py, tests/test_topk_model_gpu.py).

The rule: the k largest logits of a row, descending by value, equal values by ascending index; -0.0 == +0.0; -inf entries rank last,
among themselves by index; a NaN ranks as -inf does (it never wins over a number, and ties with -inf by index).
logp[j] = x[ids[j]] - lse, lse = logsumexp(row) unless given.

The kernel's geometry, which the cases aim at: one 512-thread block per row, thread t takes the 16-byte chunks (8 elements) t, t + 512,
...; wave w is threads 64 w .. 64 w + 63; every thread keeps its 8 best, every wave merges its 64 lists, wave 0 merges the 8 waves.
"""
import torch

THREADS = 512
WAVE = 64
TOPK_MAX = 8
KS = (1, 5, 8)
# V: one chunk (k = 8 = V) | one thread takes two chunks, the rest one | the tiny model | the 8B vocabulary (one row)
VS = (8, 8 * THREADS + 8, 1024, 128256)
PAD_SENTINEL = 29952.0  # (on the bf16 grid) in the columns V..ld: larger than every logit, would win if read
NINF = float("-inf")


def _bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16)


def top_logprobs_ref(row: torch.Tensor, k: int, lse=None):
    """(ids int32 [k], logp float64 [k]) of one row (any float dtype) by the rule above, in float64."""
    x = row.double()
    key = torch.where(torch.isnan(x), torch.full_like(x, NINF), x)
    order = torch.sort(key, descending=True, stable=True).indices  # stable: equal keys keep their order = ascending index
    ids = order[:k]
    if lse is None:
        lse = torch.logsumexp(x, dim=0)
    return ids.to(torch.int32), x[ids] - torch.as_tensor(lse, dtype=torch.float64)


def top_logprobs_rows_ref(logits: torch.Tensor, k: int, lse=None):
    """top_logprobs_ref over the rows of [R, V] -> (ids int32 [R, k], logp float64 [R, k]); lse: None or [R]."""
    out = [top_logprobs_ref(logits[r], k, None if lse is None else lse[r]) for r in range(logits.shape[0])]
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
def _base(V: int, gen) -> torch.Tensor:
    return _bf(torch.randn(V, generator=gen) * 2.0).float()  # on the bf16 grid: at V = 128256 nearly every value occurs several times


def _plant(x: torch.Tensor, places, values) -> torch.Tensor:
    for p, v in zip(places, values):
        x[p % x.numel()] = v
    return x


def rows_of(V: int, gen):
    """[(kind, row fp32 on the bf16 grid)]: the row kinds of the case table at vocabulary V."""
    nchunk = V // 8
    desc = [40.0 - 2 * i for i in range(10)]
    rows = [("random", _base(V, gen))]
    # the best all inside ONE thread's chunks: thread 0's (chunk 0, and chunk 512 where it exists - the thread that takes two at 4104)
    c0 = 0
    c1 = THREADS if THREADS < nchunk else 0
    places = [c0 * 8 + 1, c1 * 8 + 6, c0 * 8 + 7, c1 * 8 + 0, c0 * 8 + 2, c1 * 8 + 5, c0 * 8 + 4, c1 * 8 + 3, c0 * 8 + 0, c0 * 8 + 6]
    places = list(dict.fromkeys(p for p in places))[: min(10, V)]
    rows.append(("one_thread", _plant(_base(V, gen).clamp(-6, 6), places, desc)))
    # the best spread ONE PER WAVE (lane 5 of wave w: chunk 64 w + 5), best in the last wave; a ninth in wave 0 again
    per_wave = [((WAVE * w + 5) % nchunk) * 8 + (w % 8) for w in range(THREADS // WAVE)]
    per_wave = list(dict.fromkeys(per_wave))
    rows.append(("per_wave", _plant(_base(V, gen).clamp(-6, 6), per_wave[::-1] + [(9 % nchunk) * 8 + 1], desc)))
    # EQUAL maxima straddling two threads (elements 7 | 8: chunks 0 | 1) and two waves (elements 511 | 512: chunks 63 | 64), twelve of them
    dup = [7, 8, 511, 512, V - 1, V // 2, 6, 9, 510, 513, V - 8, V // 2 + 1]
    rows.append(("dup_straddle", _plant(_base(V, gen).clamp(-6, 6), dup, [17.5] * len(dup))))
    # a wave's second best is the row's second best: both in wave 1 (chunks 64, 65), nothing else near
    rows.append(("wave_second", _plant(_base(V, gen).clamp(-6, 6), [(64 % nchunk) * 8, (65 % nchunk) * 8 + 3, 2], [30.0, 29.0, 28.0])))
    # the maximum is the row's LAST element, the runner-up the first of the last chunk
    rows.append(("max_last", _plant(_base(V, gen).clamp(-6, 6), [V - 1, V - 8], [25.0, 24.0])))
    rows.append(("all_equal", torch.full((V,), 1.5)))
    x = _base(V, gen)
    x[::3] = NINF
    rows.append(("some_ninf", x))
    # fewer than 8 finite entries: three numbers, the rest -inf -> the tail is -inf by ascending index
    x = torch.full((V,), NINF)
    rows.append(("few_finite", _plant(x, [V - 2, 1, V // 2], [0.5, -3.0, 0.5])))
    # NaN never wins: NaNs in front of and between the numbers; +0.0 and -0.0 tie by index
    x = _base(V, gen).clamp(-6, -1)
    _plant(x, [0, 5, V - 1], [float("nan")] * 3)
    _plant(x, [4, 2], [0.0, -0.0])
    rows.append(("nan_zero", x))
    x = torch.full((V,), NINF)
    rows.append(("nan_ninf", _plant(x, [0, 3], [float("nan"), 7.0])))
    return rows


def batch(V: int, ld=None):
    """(kinds, logits bf16 [R, ld]) with every row kind at V (the 8B vocabulary: ONE row, random with the maximum planted in the last
    chunk); the columns V..ld hold PAD_SENTINEL."""
    gen = torch.Generator().manual_seed(7000 + V)
    ld = V if ld is None else ld
    if V > 100000:
        x = _base(V, gen)
        x[V - 3] = x.max()  # equal to an earlier maximum: the tie goes to the lower index, the last chunk still places
        x[V - 5] = x.max() + 1.0
        rows = [("random_last", x)]
    else:
        rows = rows_of(V, gen)
    lg = torch.full((len(rows), ld), PAD_SENTINEL)
    for r, (_, x) in enumerate(rows):
        lg[r, :V] = x
    return [kind for kind, _ in rows], _bf(lg)


# (V, ld): every V of VS dense, and one with a row stride larger than V
SHAPES = [(V, V) for V in VS] + [(1024, 1024 + 64)]


def lse_of(logits: torch.Tensor) -> torch.Tensor:
    """A per-row fp32 lse to hand to the kernel (distinct per row, so that a wrong row shows; the all -inf / NaN rows get 0)."""
    lse = torch.logsumexp(logits.double(), dim=1)
    lse = torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse))
    return (lse + 0.125 * torch.arange(logits.shape[0])).float()


# ---- injected faults: wrong kernels restated on the host; each must be caught by at least one case ------------------------------------
def _fault_ties_highest(logits, k, lse):
    ids, lp = [], []
    for r in range(logits.shape[0]):
        x = logits[r].double()
        key = torch.where(torch.isnan(x), torch.full_like(x, NINF), x)
        order = (x.numel() - 1) - torch.sort(key.flip(0), descending=True, stable=True).indices
        ids.append(order[:k].to(torch.int32))
        lp.append(x[order[:k]] - (torch.logsumexp(x, 0) if lse is None else lse[r].double()))
    return torch.stack(ids), torch.stack(lp)


def _fault_wave_second(logits, k, lse):
    """The per-wave merge loses every wave's second best."""
    ids, lp = [], []
    V = logits.shape[1]
    wave_of = (torch.arange(V) // 8) % THREADS // WAVE
    for r in range(logits.shape[0]):
        x = logits[r].double()
        keep = torch.ones(V, dtype=torch.bool)
        for w in range(THREADS // WAVE):
            sel = (wave_of == w).nonzero()[:, 0]
            if sel.numel() >= 2:
                wi, _ = top_logprobs_ref(x[sel], 2, 0.0)
                keep[sel[wi[1]]] = False
        sel = keep.nonzero()[:, 0]
        i, _ = top_logprobs_ref(x[sel], min(k, sel.numel()), 0.0)
        i = sel[i.long()]
        i = torch.cat([i, i[-1:].expand(k - i.numel())])
        ids.append(i.to(torch.int32))
        lp.append(x[i] - (torch.logsumexp(x, 0) if lse is None else lse[r].double()))
    return torch.stack(ids), torch.stack(lp)


def _fault_last_chunk(logits, k, lse):
    """The last 16-byte chunk of the row is never looked at (V = 8: nothing is, the result is index 0 .. k-1)."""
    V = logits.shape[1]
    if V == 8:
        i = torch.arange(k, dtype=torch.int32)[None].expand(logits.shape[0], k)
        return i, torch.zeros(logits.shape[0], k, dtype=torch.float64)
    ids, _ = top_logprobs_rows_ref(logits[:, : V - 8], k)
    x = logits.double()
    l = torch.logsumexp(x, 1) if lse is None else lse.double()
    return ids, x.gather(1, ids.long()) - l[:, None]


def _fault_lse_row(logits, k, lse):
    """lse read from the row above."""
    if lse is None:
        lse = torch.logsumexp(logits.double(), 1)
    return top_logprobs_rows_ref(logits, k, torch.roll(lse, 1))


FAULTS = {"ties_highest_index": _fault_ties_highest, "wave_merge_drops_second": _fault_wave_second, "last_chunk_skipped": _fault_last_chunk,
          "lse_wrong_row": _fault_lse_row}


def same(got, want, atol=0.0) -> bool:
    """ids equal exactly and logp equal (NaN == NaN, inf == inf) within atol."""
    (gi, gl), (wi, wl) = got, want
    if not torch.equal(gi, wi):
        return False
    gl, wl = gl.double(), wl.double()
    fin = torch.isfinite(wl)
    if not torch.equal(torch.isnan(gl), torch.isnan(wl)) or not torch.equal(gl[~fin & ~torch.isnan(wl)], wl[~fin & ~torch.isnan(wl)]):
        return False
    return bool(((gl[fin] - wl[fin]).abs() <= atol).all())
