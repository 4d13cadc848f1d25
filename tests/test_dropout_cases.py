"""CPU: the restated attention-dropout mask has the statistics a mask needs, the emulation of the kernels' rounding points sits
well inside the bars the GPU test uses (tests/test_attn_dropout_gpu.py: the constants of tests/attn_cases.py), and every mutant
of tests/dropout_cases.py lands far outside them - so those bars tell a right kernel from a wrong one."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import attn_cases as C
from tests import dropout_cases as D

B, H, KVH = 2, 4, 2
SEED, COUNTER, STREAM = 20240607, 3, 1
SIZES = (64, 320, 577)
PS = (0.1, 0.5)
CASES = (("unit", "causal"), ("mixed", "docprefix"))


def test_threshold_and_scale_arithmetic():
    assert D.threshold(0.1) == 6554 and D.threshold(0.5) == 32768 and D.threshold(0.25) == 16384
    assert D.scale_c(32768) == 2.0 and D.scale_c(16384) == float(np.float32(65536.0) / np.float32(49152.0))
    for p in PS:
        t = D.threshold(p)
        assert abs(t / 65536 - p) <= 2.0 ** -17
        assert abs(D.scale_c(t) * (1.0 - t / 65536) - 1.0) < 1e-6  # the scale matches the realised probability
    from llx import kernels as K

    assert [K.attn_dropout_threshold(p) for p in (0.1, 0.25, 0.5)] == [D.threshold(p) for p in (0.1, 0.25, 0.5)]


@pytest.mark.parametrize("p", PS)
def test_keep_share_and_independence(p):
    """The kept share of every (b, h) lies within 5 binomial standard deviations of 1 - t / 65536; masks of another head, batch
    row, stream id, counter or seed agree with it on about (1 - p)^2 + p^2 of the elements (independent masks), not on all."""
    S = 577
    t = D.threshold(p)
    pr = t / 65536
    base = D.keep_mask(SEED, COUNTER, STREAM, B, H, S, S, t)
    n = S * S
    sd = math.sqrt(n * pr * (1 - pr))
    for b in range(B):
        for h in range(H):
            dev = (int(base[b, h].sum()) - n * (1 - pr)) / sd
            assert abs(dev) <= 5.0, (b, h, dev)
    agree = (1 - pr) ** 2 + pr ** 2
    sd_a = math.sqrt(agree * (1 - agree) / n)
    others = {"head": base[0, 1], "batch": base[1, 0],
              "stream": D.keep_mask(SEED, COUNTER, STREAM + 1, 1, 1, S, S, t)[0, 0],
              "counter": D.keep_mask(SEED, COUNTER + 1, STREAM, 1, 1, S, S, t)[0, 0],
              "seed": D.keep_mask(SEED + 1, COUNTER, STREAM, 1, 1, S, S, t)[0, 0],
              "transposed": base[0, 0].T, "next row": np.roll(base[0, 0], 1, axis=0), "next key": np.roll(base[0, 0], 1, axis=1)}
    for name, other in others.items():
        a = float((base[0, 0] == other).mean())
        assert abs(a - agree) <= 5.0 * sd_a, (name, a, agree)
    # rows and keys are not biased either: the per-row and per-key kept shares scatter as a binomial of S draws does
    for axis in (0, 1):
        share = base[0, 0].mean(axis=axis)
        z = (share - (1 - pr)) / math.sqrt(pr * (1 - pr) / S)
        assert abs(z).max() <= 5.0 and 0.8 <= z.std() <= 1.2, (axis, abs(z).max(), z.std())


@functools.lru_cache(maxsize=None)
def _case(family, kind, S, p):
    q, k, v, do = C.make_case(family, B, S, H, KVH, f"drop{kind}")
    mask, _, _ = C.dense_mask(kind, B, S)
    t = D.threshold(p)
    c = D.scale_c(t)
    keep = D.keep_tensor(SEED, COUNTER, STREAM, B, H, S, S, t)
    o_ref, lse_ref = D.fwd64(q, k, v, mask, keep, c)
    return q, k, v, do, mask, keep, c, t, o_ref, lse_ref


def _excess(family, kind, S, p, mutant=None):
    q, k, v, do, mask, keep, c, t, o_ref, lse_ref = _case(family, kind, S, p)
    nxt = D.keep_tensor(SEED, COUNTER + 1, STREAM, B, H, S, S, t) if mutant == "bwd_counter_plus_1" else None
    o, lse, grads = D.emulate(q, k, v, do, mask, keep, c, mutant=mutant, keep_next_counter=nxt)
    ref, rnd = D.bwd64(q, k, v, o, do, mask, keep, c)  # delta from the bf16 O the backward is given, as on the GPU
    return D.excess(o, lse, grads, o_ref, lse_ref, ref, rnd)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("family,kind", CASES)
def test_emulation_sits_inside_half_the_bars(family, kind, S, p):
    ex = _excess(family, kind, S, p)
    print(f"[{family} {kind} S={S} p={p}] " + "  ".join(f"{k} {v:.3f}" for k, v in ex.items()) + "  (multiples of the bar)")
    assert max(ex.values()) <= 0.5, ex


@pytest.mark.parametrize("mutant", D.MUTANTS)
@pytest.mark.parametrize("family,kind", CASES)
def test_mutants_land_ten_bars_out(family, kind, mutant):
    """At p = 0.5 and the smallest size of the list at which the mutant changes anything (all of them do at S = 64)."""
    ex = _excess(family, kind, 64, 0.5, mutant)
    worst = max(ex, key=ex.get)
    print(f"[{family} {kind} {mutant}] worst {worst}: {ex[worst]:.1f} x the bar")
    assert ex[worst] >= 10.0, (mutant, ex)
