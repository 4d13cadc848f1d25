"""GPU: llx.kernels.sample (csrc/sample.hip) against the fp64 restatement and acceptance rule of tests/sampling_cases.py."""
import math

import pytest
import torch

from tests import sampling_cases as C

pytestmark = pytest.mark.gpu
SEED = 11


@pytest.fixture(scope="module")
def K():
    from llx import kernels

    return kernels


_CASES: dict = {}


def _case(name, cuda):
    """(CPU view, device view with the same stride and offset) of a case, built once."""
    if name not in _CASES:
        s = C.SHAPE[name]
        x = C.make_logits(s)
        _CASES[name] = (x, C.to_device(x, s, cuda))
    return _CASES[name]


def _pos(R, cuda):
    return torch.arange(R, dtype=torch.int64) * 7 + 1000, (torch.arange(R, dtype=torch.int64, device=cuda) * 7 + 1000)


def _lowest_argmax(x):
    xf = x.float()
    return torch.stack([(row == row.max()).nonzero()[0, 0] for row in xf])


@pytest.mark.parametrize("name", [s.name for s in C.SHAPES])
def test_greedy_is_argmax(K, cuda, name):
    x, xd = _case(name, cuda)
    assert xd.stride() == x.stride() and (xd.data_ptr() % 16 == 0) == (C.SHAPE[name].offset == 0)
    _, pos = _pos(x.shape[0], cuda)
    tok, _, th, kept = K.sample(xd, temperature=0.0, pos=pos, aux=True)
    assert torch.equal(tok.cpu(), _lowest_argmax(x))
    assert torch.equal(th.cpu(), x.float().max(dim=1).values)
    assert torch.equal(kept.cpu().long(), (x.float() == x.float().max(dim=1, keepdim=True).values).sum(1))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_greedy_ties_and_minus_inf(K, cuda, dtype):
    V = 4100
    x = C.O.randn("sampling_greedy_special", (4, V), 2.0).to(dtype)
    x[1, [4000, 17, 2050]] = 9.0                     # the maximum three times: the lowest index wins
    x[2, :13] = -math.inf                            # -inf over the first chunks and scattered
    x[2, 100::7] = -math.inf
    x[3] = -math.inf                                 # -inf everywhere: index 0
    pos = torch.zeros(4, dtype=torch.int64, device=cuda)
    tok, _, th, kept = K.sample(x.to(cuda), temperature=0.0, pos=pos, aux=True)
    assert tok.tolist() == [int(_lowest_argmax(x[:1])[0]), 17, int(_lowest_argmax(x[2:3])[0]), 0]
    assert kept.tolist()[1] == 3 and kept.tolist()[3] == V and th.tolist()[1] == 9.0
    # sampled with -inf entries: they are never drawn, and they do not count against top_k
    for k, p in ((0, 1.0), (0, 0.9), (50, 1.0)):
        tok, u, th, kept = K.sample(x[2:3].repeat(64, 1).to(cuda), temperature=1.0, top_k=k, top_p=p, seed=SEED,
                                    pos=torch.arange(64, dtype=torch.int64, device=cuda), aux=True)
        assert bool(torch.isfinite(x[2][tok.cpu()]).all())
        for r in range(0, 64, 9):
            assert C.accepts(x[2], 1.0, k, p, float(u[r]), int(tok[r]), float(th[r]), int(kept[r])) == []


def test_uniform_is_bit_equal_to_the_host_hash(K, cuda):
    from llx.sampling import uniform

    x, xd = _case("v1000", cuda)
    pos = torch.tensor([0, 1, 2, 4095, 2 ** 31, 2 ** 40 + 5, 2 ** 62] + list(range(100, 157)), dtype=torch.int64)
    for seed in (0, 1234, 2 ** 64 - 1):
        _, u, _, _ = K.sample(xd, temperature=1.0, seed=seed, pos=pos.to(cuda), aux=True)
        want = torch.tensor([uniform(seed, int(pos[r]), r) for r in range(64)], dtype=torch.float32)
        assert torch.equal(u.cpu(), want)


@pytest.mark.parametrize("name", [s.name for s in C.SHAPES])
def test_grid_against_the_acceptance_rule(K, cuda, name):
    """Every (top_k, top_p, temperature) point of the case: threshold acceptable, kept = the count at it, token acceptable; with
    0 < top_k <= 50 the token equals the fp64 restatement's on all but <= 1 % of the rows."""
    s = C.SHAPE[name]
    x, xd = _case(name, cuda)
    pos_c, pos = _pos(s.R, cuda)
    rows: dict = {}
    for k, p, T in C.params_for(s):
        tok, u, th, kept = (t.cpu() for t in K.sample(xd, temperature=T, top_k=k, top_p=p, seed=SEED, pos=pos, aux=True))
        differ = 0
        for r in range(s.R):
            key = (r, T, k if 0 < k < s.V else 0)
            if key not in rows:
                rows[key] = C.Row(x[r], T, k)
            bad = C.accepts_row(rows[key], p, float(u[r]), int(tok[r]), float(th[r]), int(kept[r]))
            assert bad == [], (name, k, p, T, r, bad)
            if 0 < k <= 50:
                differ += C.restate_row(rows[key], p, float(u[r])) != (int(tok[r]), float(th[r]), int(kept[r]))
        assert differ <= 0.01 * s.R, (name, k, p, T, differ)


def test_strided_row_view_and_3d_input(K, cuda):
    """The last position of a [S, V] logits block per row ([R, V] view with row stride S * V), and a [1, R, V] tensor."""
    x, _ = _case("v1001_stride1003", cuda)
    R, V = 8, x.shape[1]
    big = torch.zeros(R, 3, V, dtype=torch.bfloat16, device=cuda)
    big[:, -1] = x[:R].to(cuda)
    pos_c, pos = _pos(R, cuda)
    want = K.sample(x[:R].contiguous().to(cuda), temperature=0.8, top_p=0.9, seed=SEED, pos=pos, aux=True)
    got = K.sample(big[:, -1], temperature=0.8, top_p=0.9, seed=SEED, pos=pos, aux=True)
    got3 = K.sample(x[:R].contiguous().to(cuda)[None], temperature=0.8, top_p=0.9, seed=SEED, pos=pos, aux=True)
    for a, b, c in zip(want, got, got3):
        assert torch.equal(a, b) and torch.equal(a, c)
    for r in range(R):
        assert C.accepts(x[r], 0.8, 0, 0.9, float(got[1][r]), int(got[0][r]), float(got[2][r]), int(got[3][r])) == []


def test_all_equal_logits_follow_the_uniform(K, cuda):
    V, R = 1000, 64
    x = torch.full((R, V), 1.5, dtype=torch.bfloat16)
    _, pos = _pos(R, cuda)
    tok, u, th, kept = (t.cpu() for t in K.sample(x.to(cuda), temperature=0.7, seed=SEED, pos=pos, aux=True))
    assert kept.tolist() == [V] * R and th.tolist() == [1.5] * R
    for r in range(R):
        assert abs(int(tok[r]) - math.floor(float(u[r]) * V)) <= 1
        assert C.accepts(x[r], 0.7, 0, 1.0, float(u[r]), int(tok[r]), 1.5, V) == []


def test_frequencies_over_8192_rows(K, cuda):
    x = C.stat_logits()
    xd = x.to(cuda)[None].expand(C.STAT_R, C.STAT_V)  # the same row 8192 times: row stride 0 is not a row stride >= V, so materialise
    pos = torch.arange(C.STAT_R, dtype=torch.int64, device=cuda)
    tok, u, _, kept = K.sample(xd.contiguous(), temperature=1.0, top_k=C.STAT_TOP_K, seed=C.STAT_SEED, pos=pos, aux=True)
    assert torch.equal(u.cpu().double(), C.stat_uniforms())
    assert kept.tolist() == [C.STAT_TOP_K] * C.STAT_R
    assert C.stat_check(tok) == []
    r = C.Row(x, 1.0, C.STAT_TOP_K)
    assert (r.draw_many(r.g_k, C.stat_uniforms()) != tok.cpu()).sum() <= 0.01 * C.STAT_R


def test_side_effects(K, cuda):
    x, xd = _case("v1000", cuda)
    R, cap, base = 64, 5, 1010
    pos = torch.arange(R, dtype=torch.int64, device=cuda) + 1000       # pos - base in [-10, 54): rows 10..14 land inside the history
    hist_full = torch.full((R, 8), -7, dtype=torch.int64, device=cuda)
    hist = hist_full[:, :cap]  # row stride 8 > cap
    out = torch.full((R,), -1, dtype=torch.int64, device=cuda)
    plain = K.sample(xd, temperature=1.0, top_k=4, seed=SEED, pos=pos.clone())
    eos = int(plain[20])
    fin = torch.zeros(R, dtype=torch.int32, device=cuda)
    fin[12] = 1
    fin[40] = 1
    pos2 = pos.clone()
    tok = K.sample(xd, temperature=1.0, top_k=4, seed=SEED, pos=pos2, out=out, history=hist, hist_base=base, advance=True, eos_id=eos, finished=fin)
    assert tok.data_ptr() == out.data_ptr()
    was_finished = torch.zeros(R, dtype=torch.bool)
    was_finished[[12, 40]] = True
    want = torch.where(was_finished, torch.tensor(eos), plain.cpu())
    assert torch.equal(tok.cpu(), want)
    # advance adds exactly one, except on rows that were finished
    assert torch.equal(pos2.cpu(), pos.cpu() + (~was_finished).long())
    # history: written at pos - base only inside [0, cap), never by a finished row; the padding past cap is untouched
    h = hist.cpu()
    for r in range(R):
        want_row = torch.full((cap,), -7, dtype=torch.int64)
        j = 1000 + r - base
        if 0 <= j < cap and not was_finished[r]:
            want_row[j] = want[r]
        assert torch.equal(h[r], want_row), r
    assert bool((hist_full[:, cap:] == -7).all())
    # a sampled eos sets the flag; nothing else does
    assert torch.equal(fin.cpu().bool(), was_finished | (plain.cpu() == eos))
    assert bool(fin[20] == 1)


def test_two_calls_are_bit_identical(K, cuda):
    x, xd = _case("v128256", cuda)
    _, pos = _pos(3, cuda)
    for kw in (dict(top_k=50, top_p=0.9), dict(top_p=0.9), dict()):
        a = K.sample(xd, temperature=0.7, seed=SEED, pos=pos, aux=True, **kw)
        b = K.sample(xd, temperature=0.7, seed=SEED, pos=pos, aux=True, **kw)
        assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_wrapper_rejects(K, cuda):
    from llx._lib import LlxError

    x, xd = _case("v1024", cuda)
    pos = torch.zeros(3, dtype=torch.int64, device=cuda)
    for kw in (dict(temperature=-1.0), dict(temperature=1.0, top_p=0.0), dict(temperature=1.0, top_k=-2), dict(temperature=1.0, eos_id=3)):
        with pytest.raises(LlxError):
            K.sample(xd, pos=pos, **kw)
    with pytest.raises(LlxError):
        K.sample(xd, temperature=1.0, pos=pos.cpu())
    with pytest.raises(LlxError):
        K.sample(xd.half(), temperature=1.0, pos=pos)
