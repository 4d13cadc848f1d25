"""CPU checks of the inference-attention cases (tests/infer_attn_cases.py): the restated dispatch of attn_decode, attn_dense_fwd and
attn_mask_fwd puts every threshold where the sources have it, and llx.kernels._decode_nsplit is the formula the wrapper always used;
the table holds every class of every axis; every case passes its float64 SDPA reference in both families (so torch.equal and integer
equality are fair bars for tests/test_infer_attn_exact_gpu.py); every fault planted in the emulated split walk changes an expected
value of each case aimed at its class (so those bars would fail).

Why the exact families exist: measured on Gaussian q, K, V at the same shapes and masks, the bar the decode kernel was held to - max
error within 0.02 of the largest reference magnitude - accepts 2 of the 9 planted faults: the two confined to a single split (its last
key dropped, its first key counted twice) pass at 8197 keys with errors of 0.0071 and 0.0056 of max|ref|, and sit on either side
of the bar, within a hundredth of it, at the other caches of 4101 keys and more (0.013 .. 0.031).  The seven faults that hit every split, row or
batch element are rejected in every case aimed at them, the closest at 0.024 (the clamp row off by one under a per-batch mask with 16
tokens) and 0.031 (the span rounded down at 8197 keys).  test_old_bar_accepts_the_single_split_faults asserts the number."""
import functools

import pytest
import torch

from oracle import ref as O
from tests import infer_attn_cases as C

DECODE = C.cases_of("decode")
WRAPPER = [c for c in DECODE if not c.nsplit]


# ------------------------------------------------------------------------------------------------------------------ thresholds
def test_decode_instance_thresholds():
    inst = C.decode_instance
    assert [inst(r, 1) for r in (4, 5, 8, 9, 16, 17)] == [(4, 4, 16), (8, 2, 4), (8, 2, 4), (16, 1, 4), (16, 1, 4), None]
    assert inst(2, 2) == (4, 4, 16) and inst(1, 5) == (8, 2, 4) and inst(3, 3) == (16, 1, 4) and inst(2, 9) is None
    # the LDS the partials take: NPART x ROWS x (128 + 2) floats, 32.5 KiB for the 4- and 16-row instances
    assert {n * r * 130 * 4 for r, _, n in (inst(4, 1), inst(16, 1))} == {33280} and inst(8, 1)[0] * 4 * 130 * 4 == 16640


def test_nsplit_thresholds_and_helper():
    """Both sides of every term of the wrapper's nsplit, and the helper in llx.kernels against the expression attn_decode had inline."""
    from llx import kernels as K

    ns, term = C.decode_nsplit, C.nsplit_term
    assert [ns(1, 1, s) for s in (1, 32, 33, 64, 65)] == [1, 1, 2, 2, 3]                      # ceil(Skv / 32); 32 | 33 keys: one split | two
    assert [ns(1, 1, s) for s in (4064, 4065, 4096, 4097, 8197)] == [127, 128, 128, 128, 128]  # the cap, from 4065 keys on
    assert (term(1, 1, 4064), term(1, 1, 4096), term(1, 1, 4097)) == ("keys", "keys+cap", "cap")
    assert [ns(b, 1, 8197) for b in (3, 4, 5, 8, 128, 512, 513)] == [128, 128, 103, 64, 4, 1, 1]  # ceil(512 / (B KVH)), from B KVH = 5 on
    assert (term(4, 1, 8197), term(5, 1, 8197), term(16, 8, 520), term(16, 8, 100)) == ("wgs+cap", "wgs", "wgs", "keys+wgs")
    assert ns(2, 2, 1000) == 32 and term(2, 2, 1000) == "keys"
    for B in (1, 2, 3, 4, 5, 7, 16, 64, 600):
        for KVH in (1, 2, 8, 32):
            for Skv in (1, 2, 31, 32, 33, 63, 64, 65, 200, 1000, 4064, 4065, 4096, 4097, 8197, 16384, 131072):
                old = max(1, min(-(-Skv // 32), -(-512 // (B * KVH)), 128))  # the line that stood in kernels.attn_decode
                assert K._decode_nsplit(B, KVH, Skv) == old == ns(B, KVH, Skv)


def test_split_walk_geometry():
    """span, k_lo / k_hi, empty splits, steps per wave and the owner of a key at hand-computed shapes."""
    p = C.decode_plan(4, 1, 200, 200, 7)
    assert (p.span, p.splits[0], p.splits[6], p.empty, p.ragged) == (32, (0, 32), (192, 200), 0, True)
    assert [p.steps(0, w) for w in range(4)] == [1, 1, 0, 0] and [p.steps(6, w) for w in range(4)] == [1, 0, 0, 0]
    assert p.owner(0) == (0, 0, 0, 0, 0) and p.owner(31) == (0, 0, 1, 3, 3) and p.owner(199) == (6, 0, 0, 1, 3)
    p = C.decode_plan(16, 1, 200, 200, 7)  # one key per lane group and step: 16 keys per workgroup step
    assert [p.steps(0, w) for w in range(4)] == [2, 2, 2, 2] and p.owner(21) == (0, 1, 1, 0, 1)
    p = C.decode_plan(2, 2, 1000, 65, 32)
    assert (p.span, len(p.live), p.empty, p.splits[4], p.splits[5]) == (16, 5, 27, (64, 65), (80, 80))
    p = C.decode_plan(2, 2, 8197, 8197, 128)
    assert (p.span, len(p.live), p.splits[102]) == (80, 103, (8160, 8197)) and [p.steps(0, w) for w in range(4)] == [2, 1, 1, 1]
    p = C.decode_plan(2, 2, 520, 520, 4)
    assert (p.span, p.splits[3]) == (144, (432, 520)) and [p.steps(0, w) for w in range(4)] == [3, 2, 2, 2]
    p = C.decode_plan(2, 2, 200, 200, 3)
    assert p.span == 80 and p.splits == ((0, 80), (80, 160), (160, 200))
    assert C.decode_plan(2, 2, 200, 200, 1024).span == 16 and C.decode_plan(2, 2, 200, 200, 1024).empty == 1011
    assert C.decode_plan(1, 1, 33, 33, 2).splits == ((0, 32), (32, 33)) and C.decode_plan(1, 1, 32, 32, 1).splits == ((0, 32),)
    # every key below ext has exactly one owner, and the owner's coordinates are in range
    for p in (C.decode_plan(4, 1, 200, 200, 7), C.decode_plan(3, 2, 1000, 65, 32), C.decode_plan(16, 1, 200, 123, 40)):
        seen = {p.owner(k) for k in range(p.ext)}
        assert len(seen) == p.ext and all(s in p.live and w < 4 and j < p.kpg and g < 4 and st < p.steps(s, w) for s, st, w, j, g in seen)


def test_tile_classes_rule():
    m = torch.zeros(1, 130, 130, dtype=torch.bool)
    m[0, :128, :64] = True   # full tile, all 128 rows: 2
    m[0, 128:, 64:128] = True  # the two rows that exist of the second block: rows past Sq do not count: 2
    m[0, :128, 128:] = True  # ragged tile: never 2
    m[0, 5, 70] = True
    assert C.tile_classes(m).tolist() == [[[2, 1, 1], [0, 2, 0]]]
    assert [C.dense_chunks(s) for s in (1, 63, 64, 65, 130)] == [1, 1, 1, 2, 3]


# ------------------------------------------------------------------------------------------------------------------ coverage
def test_decode_table_holds_every_class():
    plans = {(c.id, e): c.plan(e) for c in WRAPPER for e in (True, False)}
    # row classes x mask forms, both kv-head counts, every instance whole and partly filled
    assert {(c.G, c.M, c.form) for c in WRAPPER} >= {(g, m, f) for g, m in C.ROW_CLASSES for f in C.FORMS}
    assert {c.KVH for c in WRAPPER if (c.G, c.M) in C.ROW_CLASSES and c.Skv == 200} == {1, 2}
    assert {c.G * c.M for c in WRAPPER} >= {1, 3, 4, 5, 6, 8, 9, 10, 15, 16}
    assert any(c.G not in (1, 2, 4, 8, 16) and C.decode_instance(c.G, c.M)[0] == r for r in (4, 8, 16) for c in WRAPPER)
    for rows in (4, 8, 16):
        of = [c for c in WRAPPER if C.decode_instance(c.G, c.M)[0] == rows]
        assert {c.form for c in of} == set(C.FORMS) and any(c.G * c.M == rows for c in of) and any(c.G * c.M < rows for c in of)
        assert any(c.M > 1 and c.G * c.M < rows and c.form != "head" for c in of)  # min(r, M - 1) clamps
        assert any(c.G > 1 and c.G * c.M < rows for c in of)                       # min(g, G - 1) clamps / dead rows r / M >= G
        # the plan's classes under this instance
        ps = [plans[c.id, e] for c in of for e in (True, False)]
        assert set().union(*(p.step_classes for p in ps)) == {0, 1, 2, 3} if rows == 4 else {1, 2, 3} <= set().union(*(p.step_classes for p in ps))
        assert any(p.empty and p.live for p in ps) and any(not p.empty for p in ps) and any(p.ragged for p in ps)
    # cache lengths and batches; the terms of nsplit
    assert {c.Skv for c in WRAPPER} == {1, 17, 32, 33, 200, 520, 1000, 4101, 8197}
    assert {(c.Skv, c.live) for c in WRAPPER if c.live} == {(1000, 65)} and all(plans[c.id, True].empty >= 27 for c in WRAPPER if c.live)
    assert {plans[c.id, True].nsplit for c in WRAPPER} == {1, 2, 4, 7, 32, 128}
    terms = {C.nsplit_term(c.B, c.KVH, c.Skv) for c in WRAPPER}
    assert {"keys", "wgs", "cap", "wgs+cap"} <= terms
    assert all(c.B * c.KVH <= 4 for c in WRAPPER if c.Skv > 4096) and {c.B for c in WRAPPER} >= {1, 2, 3, 16}
    many = [c for c in WRAPPER if (c.B, c.KVH) == (16, 8)]
    assert many and all(C.nsplit_term(c.B, c.KVH, c.Skv) == "wgs" and 3 in plans[c.id, True].step_classes and plans[c.id, True].nsplit == 4 for c in many)
    assert {c.form for c in many} >= {"batch", "head"} and {C.decode_instance(c.G, c.M)[0] for c in many} == {4, 8, 16}
    # rows without keys next to exact ones, in every form
    assert {c.form for c in WRAPPER if c.nan} == set(C.FORMS)
    # the C entry: nsplit 3 | above ceil(ext / 16) | 1024, at a 4-row and a 16-row shape
    abi = [c for c in DECODE if c.nsplit]
    assert {(C.decode_instance(c.G, c.M)[0], c.nsplit) for c in abi} == {(r, n) for r in (4, 16) for n in (3, 40, 1024)}
    assert all(c.nsplit > -(-c.ext // 16) for c in abi if c.nsplit >= 40) and all(c.nsplit not in {plans[k].nsplit for k in plans} for c in abi)


def test_decode_targets_sit_on_the_plans_edges():
    """Over the table, the selection targets cover key 0, first and last keys of splits, the last live key, a partly filled last group,
    every (wave, lane group) and every load j of every instance; and a per-batch mask gives every sequence its own live range."""
    hit = set()
    for c in DECODE:
        d = C.build(c.id, "sel")
        for e in (True, False):
            p = c.plan(e)
            for t in d["tgt"].flatten().tolist():
                if t < 0:
                    hit.add("nan")
                    continue
                s, st, w, j, g = p.owner(t)
                lo, hi = p.splits[s]
                hit |= {("wave", p.kpg, w, g), ("load", p.kpg, j), ("step", min(st, 2))}
                hit |= {n for n, ok in (("key0", t == 0), ("split_first", t == lo and s > 0), ("split_last", t == hi - 1 and s < len(p.live) - 1),
                                        ("last_live", t == p.ext - 1), ("ragged_group", p.ragged and t >= p.ext - p.ext % 16)) if ok}
        if c.form == "batch" and c.B > 1 and c.ext > 7 * c.B:
            m = d["mask4"]
            rng = [(int(m[b, 0].any(0).nonzero().min()), int(m[b, 0].any(0).nonzero().max())) for b in range(c.B) if m[b, 0].any()]
            assert len(set(rng)) == len(rng) and (len(rng) > 1 or c.nan)
    assert {"nan", "key0", "split_first", "split_last", "last_live", "ragged_group", ("step", 0), ("step", 1), ("step", 2)} <= hit
    for kpg in (4, 2, 1):
        assert {("wave", kpg, w, g) for w in range(4) for g in range(4)} <= hit and {("load", kpg, j) for j in range(kpg)} <= hit


def test_dense_table_holds_every_class():
    cs = C.cases_of("dense")
    assert {c.Skv for c in cs} == {1, 63, 64, 65, 130} and {c.G for c in cs} == {1, 3} and {c.M for c in cs} == {1, 17} and {c.B for c in cs} == {2}
    for form in C.FORMS:
        of = [c for c in cs if c.form == form]
        assert {c.Skv for c in of} == {1, 63, 64, 65, 130} and {c.G for c in of} == {1, 3} and {c.M for c in of} == {1, 17}
    # a first, a middle and a last chunk masked whole for rows that attend elsewhere
    seen = set()
    for c in cs:
        m = C.build(c.id, "cen0")["mask4"]
        n = C.dense_chunks(c.Skv)
        per = torch.stack([m[..., i * 64:(i + 1) * 64].any(-1) for i in range(n)], -1)  # [B, H, M, chunks]
        rows = per.any(-1)
        for i in range(n):
            if n >= 3 and bool((rows & ~per[..., i]).any()):
                seen.add("first" if i == 0 else ("last" if i == n - 1 else "middle"))
        if c.chunk:
            i = {"first": 0, "middle": 1, "last": n - 1}[c.chunk]
            assert n == 3 and not bool(per[..., i].any()) and bool(rows.any())
    assert seen == {"first", "middle", "last"} and {c.chunk for c in cs} == {"", "first", "middle", "last"}
    assert any(c.nan and bool((C.build(c.id, "cen0")["count"] == 0).any()) for c in cs)


def test_prefill_table_holds_every_class():
    cs = C.cases_of("prefill")
    assert {c.M for c in cs} == {1, 17, 128, 129, 300} and {c.Skv for c in cs} == {4, 63, 64, 65, 700, 4300}
    assert max(-(-c.Skv // 64) for c in cs) > 64 and {c.B for c in cs} == {1, 2} and {c.G for c in cs} == {1, 2}
    assert any(c.B == 2 and (c.Skv + c.pad) % 2 == 1 for c in cs) and {(c.Skv + c.pad) % 2 for c in cs} == {0, 1}
    first, last, tgt_cls, tgt_pos = set(), set(), set(), set()
    for c in cs:
        d = C.build(c.id, "sel")
        cls = C.tile_classes(d["mask4"][:, 0])
        first |= set(cls[:, :, 0].flatten().tolist())
        last |= set(cls[:, :, -1].flatten().tolist())
        if c.B == 2:  # per-batch masks
            assert not torch.equal(d["mask4"][0], d["mask4"][1])
        for b in range(c.B):
            for m in range(c.M):
                t = int(d["tgt"][b, 0, m])
                if t >= 0:
                    tgt_cls.add(int(cls[b, m // 128, t // 64]))
                    tgt_pos |= {n for n, ok in (("tile_first", t % 64 == 0), ("tile_last", t % 64 == 63), ("row_last", t == c.Skv - 1)) if ok}
    assert first == {0, 1, 2} and last == {0, 1, 2}
    assert tgt_cls == {1, 2} and tgt_pos == {"tile_first", "tile_last", "row_last"}


# ------------------------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("cid", list(C.CASES))
def test_case_passes_its_float64_reference(cid):
    """float64 SDPA on the case's operands, rounded to bf16: selection is the gathered V rows bit for bit (and the target leads every
    other allowed key by 181 nats), census decodes to the integer counts with count_d <= 128; rows without keys are NaN."""
    c = C.CASES[cid]
    for fam in C.FAMILIES:
        d = C.build(cid, fam)
        o = C.rbf(C.sdpa64(d))
        assert o.shape == (c.B, c.H, c.M, C.HD) and C.family_ok(o, d), (cid, fam)
        nan_rows = torch.isnan(o.float()).all(-1)
        assert torch.equal(nan_rows, ~d["mask4"].any(-1)) and bool(c.nan) <= bool(nan_rows.any()) and not bool(nan_rows.all())
        if fam == "sel":
            kk = d["k"].double().repeat_interleave(c.G, 1)
            s = torch.einsum("bhmd,bhkd->bhmk", d["q"].double(), kk) / C.HD ** 0.5
            top = s.gather(3, d["tgt"].clamp_min(0)[..., None])
            others = s.masked_fill(~d["mask4"], float("-inf")).scatter(3, d["tgt"].clamp_min(0)[..., None], float("-inf")).max(-1, keepdim=True).values
            gap = (top - others)[d["tgt"] >= 0]
            assert float(gap.min()) > 181.0
            assert len({C.salt(c, b, kv) for b in range(c.B) for kv in range(c.KVH)}) == c.B * c.KVH
        else:
            assert int(d["count_d"].max()) <= 128 and bool(torch.isfinite(d["k"].float()).all()) and float(d["k"].float().abs().max()) > 9000
            if fam == "cen0":  # the bar is not vacuous: one key less, or one key twice, in one row changes what plane 0 decodes to
                b, h, m = (d["count"] == d["count"].max()).nonzero()[0].tolist()
                for w in (0, 2) if int(d["count"].max()) > 2 else (0,):
                    W = d["mask4"].long().clone()
                    W[b, h, m, int(d["mask4"][b, h, m].nonzero()[-1])] = w
                    assert not C.census_ok(C.rbf(C.weighted_sdpa64(d["q"], d["k"], d["v"], W)), d)


# ------------------------------------------------------------------------------------------------------------------ planted faults
def _aimed(fault):
    """Every third case of each instance that is aimed at the fault's class."""
    by_rows = {r: [c.id for c in DECODE if C.fault_applies(c, fault) and C.decode_instance(c.G, c.M)[0] == r] for r in (4, 8, 16)}
    ids = [cid for ids in by_rows.values() for cid in ids[::3]]
    if fault.endswith("_one"):  # and every long cache, where one key weighs least
        ids += [c.id for c in DECODE if c.Skv >= 4101 and c.id not in ids]
    return ids


AIMED = {f: _aimed(f) for f in C.FAULTS}


@functools.lru_cache(maxsize=None)
def _fault_outcomes(cid: str) -> dict:
    """fault -> (families whose expectation the fault changes, whether the old bar accepts it on Gaussian operands) for the faults aimed
    at this case; also checks that the walk without a fault counts every allowed key exactly once, with and without an extent."""
    c = C.CASES[cid]
    faults = [f for f in C.FAULTS if cid in AIMED[f]]
    out = {f: [set(), None] for f in faults}
    m4 = C.expand_mask(c, C.build_mask(c))
    for e in (True, False):
        W, extra = C.emulate(c, m4, e)
        assert torch.equal(W, m4.long()) and not bool(extra.any()), (cid, e)
    assert torch.equal(C.walk_counts(c, True, "span_ceil_only"), C.walk_counts(c, True))  # the walk does not need span % 16 == 0
    for fam in C.FAMILIES:
        d = C.build(cid, fam)
        for f in faults:
            W, extra = C.emulate(c, d["mask4"], True, f)
            if not C.family_ok(C.rbf(C.weighted_sdpa64(d["q"], d["k"], d["v"], W, extra)), d):
                out[f][0].add(fam)
    d = C.build(cid, "cen0")
    q, k, v = (O.randn(f"ia_old_{n}_{cid}", d[n].shape, 1.0).to(C.BF16) for n in ("q", "k", "v"))
    want = C.rbf(C.weighted_sdpa64(q, k, v, d["mask4"].long())).double()
    for f in faults:
        W, extra = C.emulate(c, d["mask4"], True, f)
        got = C.rbf(C.weighted_sdpa64(q, k, v, W, extra)).double()
        assert not torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(want, nan=-7.0)), (cid, f)
        out[f][1] = C.old_bar_accepts(got, want)
    return out


@pytest.mark.parametrize("fault", C.FAULTS)
def test_fault_changes_its_cases(fault):
    """Every case aimed at the fault's class sees it: the emulated kernel's output misses the bar of at least one family."""
    assert len(AIMED[fault]) >= 3
    for cid in AIMED[fault]:
        assert _fault_outcomes(cid)[fault][0], (fault, cid)
    if fault != "empty_factor1":  # census sees every one of these
        assert all({"cen0", "cen1"} & _fault_outcomes(cid)[fault][0] for cid in AIMED[fault])


def test_faults_are_aimed_at_every_instance():
    for fault in C.FAULTS:
        rows = {C.decode_instance(C.CASES[cid].G, C.CASES[cid].M)[0] for cid in AIMED[fault]}
        assert rows == {4, 8, 16}, (fault, rows)


def test_old_bar_accepts_the_single_split_faults():
    """Gaussian q, K, V (the distributions of test_attn_decode_against_oracle_sdpa) at the shapes and masks of the aimed cases, the
    faulty and the right output both from float64 and rounded to bf16.  Every fault changes output bits in every aimed case
    (_fault_outcomes asserts it); the 0.02 max|ref| bar accepts two of the nine faults - the ones confined to one split, at the longest
    cache - and rejects the other seven everywhere."""
    accepted = {}
    for f in C.FAULTS:
        acc = [cid for cid in AIMED[f] if _fault_outcomes(cid)[f][1]]
        print(f"old bar, {f}: accepted in {len(acc)} of {len(AIMED[f])} aimed cases {acc}")
        accepted[f] = acc
    assert sorted(f for f, acc in accepted.items() if acc) == ["double_first_one", "drop_last_one"]
    assert sum(1 for acc in accepted.values() if acc) == 2
    assert all("dec_s8197_g1m3" in accepted[f] for f in ("drop_last_one", "double_first_one"))
