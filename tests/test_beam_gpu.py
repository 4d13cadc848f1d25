"""GPU: the beam-search kernels (csrc/beam.hip) against their host reference (llx.sampling.beam_shortlist / beam_step) on the case table
of tests/beam_cases.py - decisions identical, scores within SCORE_TOL per accumulated step, two launches bit-identical, a done state
frozen - and llx_kv_reorder_rows on guard-filled caches against index_select."""
import pytest
import torch

from tests import beam_cases as BC

pytestmark = pytest.mark.gpu
_REF: dict = {}


def _ref(case):
    """(rows of every step, the reference's trace): computed once per case and shared."""
    if case.name not in _REF:
        _REF[case.name] = (BC.rows_of(case), BC.run_reference(case))
    return _REF[case.name]


def _on_device(case, z, cuda):
    """The rows of one step as the case lays them out: dtype, row stride and elements in front of the first row."""
    dt = torch.bfloat16 if case.dtype == "bf16" else torch.float32
    ld = case.ld or case.V
    buf = torch.full((case.offset + case.W * ld + 8,), float("nan"), device=cuda, dtype=dt)  # what lies between the rows is never read
    rows = buf[case.offset :].as_strided((case.W, case.V), (ld, 1))
    rows.copy_(z.to(cuda))
    return rows


def _state(W, n, cuda):
    z = lambda *shape, dt: torch.zeros(*shape, device=cuda, dtype=dt)  # noqa: E731
    return dict(cand_score=z(W, W + 1, dt=torch.float32), cand_token=z(W, W + 1, dt=torch.int32), s=z(W, dt=torch.float32),
                parent=z(W, dt=torch.int32), tok=z(W, 1, dt=torch.int64), hist=z(W, n, dt=torch.int64), bank_tok=z(W, n, dt=torch.int64),
                bank_len=z(W, dt=torch.int32), bank_score=z(W, dt=torch.float32), meta=z(3, dt=torch.int32))


def _same(a, b, skip=()):
    return all(torch.equal(a[k], b[k]) for k in a if k not in skip)


@pytest.mark.parametrize("case", BC.CASES, ids=lambda c: c.name)
def test_kernels_equal_the_reference(cuda, case):
    from llx import kernels as K
    from llx import sampling as S

    W, n = case.W, case.n
    rows, trace = _ref(case)
    st = _state(W, n, cuda)
    kw = dict(n=n, eos_id=case.eos_id, length_penalty=case.length_penalty)
    was_done = False
    for k, (z, want) in enumerate(zip(rows, trace)):
        logits = _on_device(case, z, cuda)
        K.beam_rows(logits, st["cand_score"], st["cand_token"])
        # the shortlists: tokens exactly (the order of equal logits is the index), log-probabilities within the bar
        short = [S.beam_shortlist(r, W) for r in z.double().tolist()]
        assert st["cand_token"].tolist() == [[t for _, t in row] for row in short], k
        got_lp = st["cand_score"].double().cpu()
        assert (got_lp - torch.tensor([[lp for lp, _ in row] for row in short], dtype=torch.float64)).abs().max() <= BC.SCORE_TOL, k
        again = (torch.empty_like(st["cand_score"]), torch.empty_like(st["cand_token"]))
        K.beam_rows(logits, *again)
        assert torch.equal(again[0], st["cand_score"]) and torch.equal(again[1], st["cand_token"]), k  # bit-identical

        before = {name: t.clone() for name, t in st.items()}
        K.beam_merge(*st.values(), init=k == 0, **kw)
        twice = {name: t.clone() for name, t in before.items()}
        K.beam_merge(*twice.values(), init=k == 0, **kw)
        assert _same(st, twice), k  # bit-identical

        steps = want["steps"]
        tol = BC.SCORE_TOL * steps
        assert st["parent"].tolist() == want["parent"], k
        if was_done:  # frozen: identity parents, nothing else changed
            assert want["parent"] == list(range(W)) and _same(st, before, skip=("parent",)), k
            continue
        count, done, got_steps = st["meta"].tolist()
        assert (count, bool(done), got_steps) == (len(want["bank"]), want["done"], steps), k
        assert st["hist"][:, :steps].tolist() == want["hist"] and st["tok"].view(-1).tolist() == [h[-1] for h in want["hist"]], k
        assert (st["s"].double().cpu() - torch.tensor(want["s"], dtype=torch.float64)).abs().max() <= tol, k
        lens = st["bank_len"].tolist()[:count]
        assert [st["bank_tok"][i, : lens[i]].tolist() for i in range(count)] == [t for t, _ in want["bank"]], k
        if count:
            finals = torch.tensor([f for _, f in want["bank"]], dtype=torch.float64)
            assert (st["bank_score"][:count].double().cpu() - finals).abs().max() <= tol, k
        was_done = want["done"]
    assert case.name not in ("w16_fp32", "bank_full", "replace") or was_done


def test_wrappers_refuse_bad_arguments(cuda):
    from llx import kernels as K
    from llx._lib import LlxError

    st = _state(3, 4, cuda)
    with pytest.raises(LlxError, match="cand_score"):
        K.beam_rows(torch.zeros(3, 100, device=cuda), st["cand_score"][:2], st["cand_token"])
    with pytest.raises(LlxError, match="V=3"):
        K.beam_rows(torch.zeros(3, 3, device=cuda), st["cand_score"], st["cand_token"])
    with pytest.raises(LlxError, match="hist"):
        K.beam_merge(*{**st, "hist": st["hist"][:, :3]}.values(), n=4)
    with pytest.raises(LlxError, match="HIP device only"):
        K.beam_merge(*{**st, "meta": st["meta"].cpu()}.values(), n=4)


# ---- llx_kv_reorder_rows
KVH, SMAX, HD, LAYERS, GUARD = 1, 64, 128, 2, 512


def _caches(B, cuda):
    """2 * LAYERS caches [B, KVH, SMAX, HD] inside guard-filled buffers of distinct 16-bit patterns."""
    flats, caches = [], []
    for i in range(2 * LAYERS):
        bits = torch.randint(-(2 ** 15), 2 ** 15, (2 * GUARD + B * KVH * SMAX * HD,), device=cuda, dtype=torch.int16,
                             generator=torch.Generator(device=cuda).manual_seed(100 + i))
        flats.append(bits)
        caches.append(bits[GUARD:-GUARD].view(torch.bfloat16).view(B, KVH, SMAX, HD))
    return flats, caches


@pytest.mark.parametrize("W", [3, 16])
@pytest.mark.parametrize("length", [1, 37, 64])
def test_kv_reorder_rows_equals_index_select(cuda, W, length):
    from llx import kernels as K

    B = W + 1  # a slot past the beams: never written
    flats, caches = _caches(B, cuda)
    table = K.kv_cache_table(caches)
    swap = list(range(W))
    swap[0], swap[W - 1] = W - 1, 0
    for parents in (list(range(W)), swap, [2] * W, [(5 * b + 1) % W for b in range(W)]):
        want = [f.clone() for f in flats]
        idx = torch.tensor(parents, device=cuda)
        for f, c in zip(want, caches):
            f[GUARD:-GUARD].view(B, KVH, SMAX, HD)[:W, :, :length] = c.view(torch.int16)[:, :, :length].index_select(0, idx)
        K.kv_reorder_rows(table, torch.tensor(parents, device=cuda, dtype=torch.int32), length)
        # the slots that move, and nothing else: positions >= length, the slot past W and the guards are bit-unchanged
        assert all(torch.equal(f, w) for f, w in zip(flats, want)), parents


def test_kv_reorder_rows_wrapper_checks(cuda):
    from llx import kernels as K
    from llx._lib import LlxError

    _, caches = _caches(4, cuda)
    table = K.kv_cache_table(caches)
    parent = torch.zeros(4, device=cuda, dtype=torch.int32)
    for length in (0, SMAX + 1):
        with pytest.raises(LlxError, match=f"len={length}"):
            K.kv_reorder_rows(table, parent, length)
    with pytest.raises(LlxError, match="parent must be"):
        K.kv_reorder_rows(table, parent.to(torch.int64), 4)
    with pytest.raises(LlxError, match="parent must be"):
        K.kv_reorder_rows(table, torch.zeros(5, device=cuda, dtype=torch.int32), 4)
    with pytest.raises(LlxError, match="W=1"):
        K.kv_reorder_rows(table, parent[:1], 4)
    with pytest.raises(LlxError, match="kv_cache_table"):
        K.kv_cache_table([caches[0], caches[1][:, :, :32]])
