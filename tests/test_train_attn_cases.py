"""CPU checks of the training-attention cases (tests/train_attn_cases.py): the restated walks put every threshold where
csrc/attn_bwd.hip and csrc/attn_fwd.hip have it; the table holds every class the restatement distinguishes; every case's expected
gradients agree with a plain float64 evaluation of the backward after the documented roundings and pass the exactness bounds (so
torch.equal is a fair bar for tests/test_train_attn_exact_gpu.py); the forward families pass the float64 SDPA reference; the emulated walks
without a fault count every allowed pair exactly once; every planted fault changes an expected bit of every case aimed at it.

Why the exact families exist: with Gaussian operands at the same shapes and masks, and the faulty and the right gradients both from the
emulation, the bar the older tests hold dQ, dK and dV to (atol = rtol = 4e-2) accepts OLD_BAR_ACCEPTS of the 14 planted faults in at
least one case aimed at them; test_old_bars_on_gaussian_operands prints the cases and asserts the number."""
import functools

import pytest
import torch

from oracle import ref as O
from tests import attn_cases as A
from tests import infer_attn_cases as I
from tests import train_attn_cases as C

SHORT = [c.id for c in C.CASES.values() if not c.long]
LONG = [c.id for c in C.CASES.values() if c.long]
OLD_BAR_ACCEPTS = 2  # measured; the faults are named in test_old_bars_on_gaussian_operands


def _keep(c):
    return C.keep_host(c) if c.dropout else None


# ------------------------------------------------------------------------------------------------------------------ thresholds
def test_restated_thresholds():
    # dQ, causal: the last tile of row block qb is the one that holds row 128 qb + 127; class 2 iff the tile ends at or before the block's first row
    assert [C.causal_dq_kt_end(705, qb) for qb in range(6)] == [2, 4, 6, 8, 10, 12] and C.causal_dq_kt_end(129, 1) == 3 and C.causal_dq_kt_end(64, 0) == 1
    assert [C.causal_dq_class(2, t) for t in range(6)] == [2, 2, 2, 2, 1, 1] and C.causal_dq_class(0, 0) == 1
    # dK/dV, causal: 64 x 64 index arithmetic; query tiles start at 2 kblk
    assert [C.causal_dkv_class(qt, 2) for qt in range(5)] == [0, 0, 1, 2, 2] and C.causal_dkv_class(3, 3) == 1
    # the route: the dS buffer is used for causal and rule masks up to 128 key tiles
    mk = lambda S, mask: C.Case("x", S, 1, 1, 1, mask, "ss" if mask in C.DENSE else "")
    assert C.bwd_route(mk(8192, "doc"), True) == "a" and C.bwd_route(mk(8193, "doc"), True) == "b" and C.bwd_route(mk(8256, "causal"), True) == "a"
    assert C.bwd_route(mk(320, "window"), True) == "b" and C.bwd_route(mk(320, "causal"), False) == "b"
    # the flags of the rule masks are the classes of the dense rule: ragged tiles are never 2, rows past S do not count
    m = C.rule_allow(130, None, torch.tensor([70], dtype=torch.int32), 1)
    assert C.tile_classes(m).tolist() == [[[2, 1, 0], [2, 2, 1]]]


def test_the_table_holds_every_class():
    have = set().union(*(C.classes_of(c) for c in C.CASES.values()))
    missing = sorted(C.required_classes() - have)
    assert not missing, f"classes without a case: {missing}"
    assert {c.S for c in C.CASES.values()} == set(C.SIZES)
    # the dense forms: each of the five masks, and each form with a per-batch pattern where it has a batch dim
    assert {c.mask for c in C.CASES.values() if c.mode == "mask"} == set(C.DENSE)
    for c in C.CASES.values():
        if c.mode == "mask" and c.form != "ss" and c.B > 1 and c.mask not in ("eqcausal", "deadblock") and c.S > 5:
            a = C.allow_of(c.id)
            assert not torch.equal(a[0], a[1]), c.id
        if c.mode == "mask":
            t = C.mask_tensor(c, C.allow_of(c.id))
            assert (t.stride(-2) > c.S) == (c.form == "strided") and t.dim() == (2 if c.form == "ss" else 4)
    # left padding: keyless rows, listed, next to rows that have keys, in every batch element
    for c in C.CASES.values():
        kl = C.keyless_rows(c.id)
        assert bool(kl.any()) == (c.mask == "leftpad") and not bool(kl.all(-1).any()), c.id


def test_rope_tables_are_signed_permutations():
    c = C.CASES["causal_s129"]
    t = C.rope_table(c)
    assert set(map(tuple, t.reshape(-1, 2).tolist())) == {(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)}
    x = O.randn("ta_rope_x", (2, 129, 1, 128), 1.0).to(C.BF16)
    y = C.rope_transpose(x, t)
    assert torch.equal(y.float().abs().view(2, 129, 64, 2).sort(-1).values, x.float().abs().view(2, 129, 64, 2).sort(-1).values)
    # it is the transpose (here: the inverse) of the oracle's rope_apply, and a shifted position gives another result
    assert torch.equal(C.rope_transpose(O.rope_apply(x, t), t), x) and not torch.equal(C.rope_transpose(x, t, 1), y)


# ------------------------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("cid", SHORT)
def test_backward_case_agrees_with_float64(cid):
    """expected() (fp32, chunked, on the mask as weights; it asserts the exactness bounds) against ref64 (float64, whole tensors); for
    the selection family also against attn_cases.bwd64, whose own softmax is one-hot here, and its lse against the float64 forward."""
    c = C.CASES[cid]
    keep = _keep(c)
    for fam in C.families_of(c):
        d = C.build(cid, fam)
        want = C.expected(cid, fam, keep)
        got = C.ref64(d, keep)
        assert not C.same(got, want, d["keyless"]), (cid, fam, C.explain(got, want, d["keyless"]))
        assert all(bool(torch.isfinite(t.float()).all()) and float(t.float().abs().max()) > 0 for t in want[1:]), (cid, fam)
        if fam == "sel" and keep is None and "rope" not in d and not bool(d["keyless"].any()):  # (bwd64's softmax is NaN on a keyless row)
            (dq, dk, dv), _ = A.bwd64(d["q"], d["k"], d["v"], d["o"], d["do"], d["allow"][:, None])
            assert torch.equal(dv.to(C.BF16), want[2])
            for g, w in ((dq, want[0]), (dk, want[1])):
                assert float((g - w.double()).abs().max()) <= 2.0 ** -8 * float(w.double().abs().max())
        if fam == "sel":
            _, lse = A.sdpa64(d["q"], d["k"], d["v"], d["allow"][:, None])
            ok = ~d["keyless"][:, None, :].expand_as(lse)
            assert float((d["lse"].double()[ok] - lse[ok] * A.LOG2E).abs().max()) < 1e-3  # bf16(P) = 1 needs 2.8e-3
            assert {float(x) for x in d["mag"].unique()} <= {24.0, 32.0}


@pytest.mark.parametrize("cid", LONG)
def test_long_case_expectation_is_exact(cid):
    """The two long shapes: the fp32 evaluation against the same evaluation in float64 (chunked: no S x S float64 tensor)."""
    c = C.CASES[cid]
    keep = _keep(c)
    for fam in (("cenA1", "sel") if c.S < 8000 else ("cenB1",)):
        d = C.build(cid, fam)
        want = C.expected(cid, fam, keep)
        got = C.evaluate(d, keep=keep, dtype=torch.float64)
        assert not C.same(got, want, d["keyless"]), (cid, fam)


@pytest.mark.parametrize("cid", [c.id for c in C.CASES.values() if c.mode != "mask" and not c.long])
def test_forward_case_passes_its_float64_reference(cid):
    for fam in C.FWD_FAMILIES:
        d = C.build_fwd(cid, fam)
        assert I.family_ok(I.rbf(I.sdpa64(d)), d), (cid, fam)
        if fam != "sel":  # a key less in the fullest row changes what the plane decodes to
            b, h, m = (d["count"] == d["count"].max()).nonzero()[0].tolist()
            if int(d["count"].max()) > 2 and fam == "cen0":
                W = d["mask4"].long().clone()
                W[b, h, m, int(d["mask4"][b, h, m].nonzero()[-1])] = 0
                assert not I.census_ok(I.rbf(I.weighted_sdpa64(d["q"], d["k"], d["v"], W)), d)


# ------------------------------------------------------------------------------------------------------------------ the walks
@pytest.mark.parametrize("cid", list(C.CASES))
def test_walks_without_a_fault_count_every_pair_once(cid):
    allow = C.allow_of(cid).to(torch.uint8)
    assert torch.equal(C.walk_dq(cid), allow) and torch.equal(C.walk_dkv(cid), allow)


def _routes(c):
    return ("b", "a") if c.route_a and C.bwd_route(c, True) == "a" else ("b",)


AIMED = {f: [(c.id, r) for c in C.CASES.values() for r in _routes(c) if C.fault_applies(c, f, r)] for f in C.FAULTS}


def _weights(cid, route, fault):
    if fault not in C.WALK_FAULTS:
        return None, None
    wkv = C.walk_dkv(cid, fault)
    return (wkv if route == "a" else C.walk_dq(cid, fault)), wkv  # (route (a): dQ sums the dS^T the dK/dV walk stored)


def _faulty(d, cid, route, fault, keep):
    wq, wkv = _weights(cid, route, fault)
    return C.evaluate(d, wq, wkv, fault="" if fault in C.WALK_FAULTS else fault, keep=keep)


@pytest.mark.parametrize("fault", C.FAULTS)
def test_fault_changes_every_case_aimed_at_it(fault):
    assert AIMED[fault], fault
    for cid, route in AIMED[fault]:
        c = C.CASES[cid]
        keep = _keep(c) if route == "b" else None
        seen = []
        for fam in C.families_of(c):
            d = C.build(cid, fam)
            seen = C.same(_faulty(d, cid, route, fault, keep), C.expected(cid, fam, keep), d["keyless"])
            if seen:
                break
        assert seen, (fault, cid, route)


def test_faults_are_aimed_widely():
    """Every fault has a case in each mode it can occur in; the chunk-boundary fault has its dQ and its dK/dV form."""
    modes = {f: {C.CASES[cid].mode for cid, _ in AIMED[f]} for f in C.FAULTS}
    for f in ("class1_as_2", "ragged_keys", "ragged_rows", "partial_missing", "delta_neighbour", "lse_neighbour", "rope_position"):
        assert modes[f] == {"causal", "rule", "mask"}, (f, modes[f])
    assert modes["chunk_skip"] == {"rule", "mask"} and {C.CASES[cid].S for cid, _ in AIMED["chunk_skip"]} == {4160, 8256}
    assert modes["keep_transposed"] == modes["drop_on_ds"] == {"causal", "rule"} and modes["other_prefix"] == {"rule"}
    assert modes["mask_word_shift"] == {"mask"} and {r for _, r in AIMED["ds_pad_rows"]} == {"a"} and modes["head_mod"] >= {"causal", "rule"}


# ------------------------------------------------------------------------------------------------------------------ the old bars
@functools.lru_cache(maxsize=None)
def _gaussian(cid: str) -> dict:
    """Gaussian q, k, v, dO of std 1 (what test_attention_fwd_bwd draws) at the case's shape and mask, o and lse from their forward."""
    c = C.CASES[cid]
    d = dict(C.build(cid, "cenA0"))
    q, do = (O.randn(f"ta_g{n}_{cid}", (c.B, c.S, c.H, 128), 1.0).to(C.BF16) for n in ("q", "do"))
    k, v = (O.randn(f"ta_g{n}_{cid}", (c.B, c.S, c.KVH, 128), 1.0).to(C.BF16) for n in ("k", "v"))
    o = torch.zeros(c.B, c.S, c.H, 128)
    lse = torch.full((c.B, c.H, c.S), float("-inf"))
    for b in range(c.B):
        for h in range(c.H):
            for r0 in range(0, c.S, 1024):
                r = slice(r0, min(c.S, r0 + 1024))
                s = (q[b, r, h].float() @ k[b, :, h // c.G].float().T * C.SCALE).masked_fill(~d["allow"][b, r], float("-inf"))
                l = torch.logsumexp(s, -1)
                lse[b, h, r] = l * A.LOG2E
                o[b, r, h] = torch.nan_to_num(torch.exp(s - l[:, None])) @ v[b, :, h // c.G].float()
    d.update(q=q, k=k, v=v, do=do, o=o.to(C.BF16), lse=lse)
    return d


def _old_bar_accepts(got, want, keyless) -> bool:
    live = ~keyless[:, :, None, None]
    pairs = ((got[0] * live, want[0] * live), (got[1], want[1]), (got[2], want[2]))
    return all(torch.allclose(g.float(), w.float(), atol=4e-2, rtol=4e-2) for g, w in pairs)


def test_old_bars_on_gaussian_operands():
    accepted = {}
    for f in C.FAULTS:
        acc = []
        for cid, route in AIMED[f]:
            c = C.CASES[cid]
            keep = _keep(c) if route == "b" else None
            d = _gaussian(cid)
            good = C.evaluate(d, keep=keep)
            bad = _faulty(d, cid, route, f, keep)
            if _old_bar_accepts(bad, good, d["keyless"]):
                acc.append(f"{cid}/{route}")
        print(f"old bar, {f}: accepted in {len(acc)} of {len(AIMED[f])} aimed cases {acc}")
        accepted[f] = acc
    names = sorted(f for f, acc in accepted.items() if acc)
    print("accepted somewhere:", names)
    assert len(names) == OLD_BAR_ACCEPTS, names
