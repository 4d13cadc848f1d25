"""GPU: the mask-driven attention backward (llx_attn_mask_bwd: the default backward route with its schedule from the mask's tile
flags and its class-1 predicate from the mask bytes) against the float64 reference `bwd64` of tests/attn_cases.py, given the
mask-driven forward's own bf16 O and lse - the protocol and the bars of tests/test_attn_range_gpu.py.  Each shape is the smallest
that reaches its path: per-sample masks with ragged tiles, masks with live tiles above the diagonal, all three tile classes, key
blocks nobody attends to, more than 64 key tiles / query blocks (the kernels' flag registers), and the causal mask given densely.
No mask here has a row without an allowed key (asserted): such a row is NaN in the forward, as in SDPA."""
import pytest
import torch

from tests import attn_cases as C

pytestmark = pytest.mark.gpu

FAMILIES = ("unit", "diag", "sink")


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


def _flags(K, mask, B, S):
    return K.attn_mask_flags(mask, B).view(B, -(-S // 128), -(-S // 64))


def _fwd(K, q, k, v, mask):
    """The mask-driven forward on the training layout: (o [B,S,H,128], lse [B,H,S])."""
    B, S, H, hd = q.shape
    o, lse = K.attn_mask_fwd(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), mask, lse=True)
    return o.view(B, S, H, hd), lse


def _lse64(q, k, mask, rows=1024):
    """logsumexp of the float64 scores (nats), in row blocks."""
    out = []
    for r0 in range(0, q.shape[1], rows):
        out.append(torch.logsumexp(C.scores64(q[:, r0 : r0 + rows], k, mask[..., r0 : r0 + rows, :]), dim=-1))
    return torch.cat(out, dim=-1)


def _bwd64_blocked(q, k, v, o, do, mask, rows=2048):
    """`bwd64` over blocks of query rows: dq and its rounding scale are per row, dk / dv and theirs are sums over the rows."""
    acc = None
    dq, rq = [], []
    for r0 in range(0, q.shape[1], rows):
        sl = slice(r0, r0 + rows)
        (a, b, c), (ra, rb, rc) = C.bwd64(q[:, sl], k, v, o[:, sl], do[:, sl], mask[..., sl, :])
        dq.append(a)
        rq.append(ra)
        acc = [b, c, rb, rc] if acc is None else [x + y for x, y in zip(acc, (b, c, rb, rc))]
    return (torch.cat(dq, 1), acc[0], acc[1]), (torch.cat(rq, 1), acc[2], acc[3])


def _check(label, grads, ref, rnd, lse, lse_ref):
    out = [(n, *C.bwd_err(a, b, r)) for n, a, b, r in zip(("dq", "dk", "dv"), grads, ref, rnd)]
    le = C.lse_rel(lse, lse_ref)
    print(f"[{label}] " + "  ".join(f"{n} {r:.3f} of bar, cos {c:.6f}" for n, r, c in out) + f"  (cos bar {C.BWD_COS})  lse {le:.1e} (bar {C.LSE_REL:.0e})")
    assert le <= C.LSE_REL, f"{label}: lse error {le:.3e}"
    for n, ratio, cos in out:
        assert ratio <= 1.0, f"{label} {n}: error {ratio:.3f} x the bar"
        assert cos >= C.BWD_COS, f"{label} {n}: worst row cosine {cos:.6f}"


def _run(K, cuda, family, B, S, H, KVH, mask, tag, blocked=False):
    """Forward + backward through the mask kernels on one case; returns everything a test may want to look at."""
    assert bool(mask.any(-1).all()), "every row attends to some key"
    q, k, v, do = (t.to(cuda) for t in C.make_case(family, B, S, H, KVH, tag))
    md = mask.to(cuda)
    o, lse = _fwd(K, q, k, v, md)
    g = [torch.full_like(t, float("nan")) for t in (q, k, v)]
    K.attn_mask_bwd(q, k, v, o, do, lse, *g, md)
    ref, rnd = (_bwd64_blocked if blocked else C.bwd64)(q, k, v, o, do, md)
    _check(f"attn_mask_bwd {tag} {family} B,S,H,KVH={(B, S, H, KVH)}", g, ref, rnd, lse, _lse64(q, k, md))
    return q, k, v, do, o, lse, g, md


def _left_padded(S, pad):
    """Causal with the first `pad` keys masked for every row (left padding), plus the diagonal so that the padded rows stay alive."""
    i = torch.arange(S)
    return ((i[:, None] >= i[None, :]) & (i[None, :] >= pad)) | torch.eye(S, dtype=torch.bool)


def _band(S, w, sink=0):
    i = torch.arange(S)
    m = (i[:, None] - i[None, :]).abs() <= w
    if sink:
        m[:, :sink] = True
    return m


@pytest.mark.parametrize("family", FAMILIES)
def test_per_sample_masks(K, cuda, family):
    """[2,1,333,333]: sample 0 prefix-LM (prefix 150), sample 1 causal with 70 left-padding keys masked: per-sample masks, mask rows of
    odd length, a ragged last query tile and key tile, a class-0 tile in front of a class-1 tile."""
    B, S = 2, 333
    i = torch.arange(S)
    m0 = (i[:, None] >= i[None, :]) | (i[None, :] < 150)
    mask = torch.stack([m0, _left_padded(S, 70)])[:, None]
    fl = _flags(K, mask.to(cuda), B, S)
    assert fl[1, 1, 0] == 0 and fl[1, 1, 1] == 1, "sample 1: key tile 0 is dead for rows 128.., tile 1 partly masked"
    _run(K, cuda, family, B, S, 8, 2, mask, "persample")


@pytest.mark.parametrize("family", FAMILIES)
def test_random_holes_above_and_below_the_diagonal(K, cuda, family):
    """A 50 % random mask plus the diagonal, broadcast over the batch: every tile is class 1 and half the allowed keys lie above the
    diagonal - a causal assumption left in the schedule or the predicate shows here."""
    B, S = 2, 200
    g = torch.Generator().manual_seed(11)
    mask = (torch.rand(S, S, generator=g) < 0.5) | torch.eye(S, dtype=torch.bool)
    assert bool((_flags(K, mask.to(cuda), B, S) == 1).all())
    assert int(mask.triu(1).sum()) > S * S // 5
    _run(K, cuda, family, B, S, 8, 2, mask, "holes")


@pytest.mark.parametrize("family", FAMILIES)
def test_band_mask_has_every_tile_class_on_both_sides(K, cuda, family):
    B, S = 1, 1000
    mask = _band(S, 300)[None, None]
    fl = _flags(K, mask.to(cuda), B, S)[0]
    assert set(fl.unique().tolist()) == {0, 1, 2}
    qb, kt = torch.arange(fl.shape[0])[:, None] * 128, torch.arange(fl.shape[1])[None, :] * 64
    assert bool((fl != 0)[kt > qb + 127].any()) and bool((fl != 0)[kt + 63 < qb].any()), "live tiles on both sides of the diagonal"
    _run(K, cuda, family, B, S, 4, 1, mask, "band")


@pytest.mark.parametrize("family", FAMILIES)
def test_keys_nobody_attends_get_exact_zeros(K, cuda, family):
    """Keys 0..129 masked for every row (rows 0..129 see key 130 only): the first dK/dV key block has no live tile at all.  Outputs are
    views of a fused [B,S,(H+2KVH)*128] buffer pre-filled with 12345 inside a poisoned allocation: dk / dv of the dead keys are exact
    zeros, nothing outside the buffer is written, and a run on a cloned mask tensor is bit-identical."""
    B, S, H, KVH, hd = 1, 400, 8, 2, 128
    i = torch.arange(S)
    mask = (i[:, None] >= i[None, :]) & (i[None, :] >= 130)
    mask[:130, 130] = True
    mask = mask[None, None]
    assert bool(mask.any(-1).all()) and not bool(mask[..., :130].any())
    q, k, v, do = (t.to(cuda) for t in C.make_case(family, B, S, H, KVH, "deadkeys"))
    md = mask.to(cuda)
    assert bool((_flags(K, md, B, S)[0, :, :2] == 0).all()), "the key block 0..127 has no live tile"
    o, lse = _fwd(K, q, k, v, md)
    W, guard = (H + 2 * KVH) * hd, 4096
    runs = []
    for m_ in (md, md.clone()):
        alloc = torch.full((guard + B * S * W + guard,), 12345.0, device=cuda, dtype=torch.bfloat16)
        buf = alloc[guard : guard + B * S * W].view(B, S, W)
        dq = buf[..., : H * hd].unflatten(-1, (H, hd))
        dk = buf[..., H * hd : (H + KVH) * hd].unflatten(-1, (KVH, hd))
        dv = buf[..., (H + KVH) * hd :].unflatten(-1, (KVH, hd))
        K.attn_mask_bwd(q, k, v, o, do, lse, dq, dk, dv, m_)
        assert bool((alloc[:guard] == 12345.0).all()) and bool((alloc[guard + B * S * W :] == 12345.0).all()), "bytes outside the buffer"
        assert not bool((buf == 12345.0).all(-1).any()), "every row of the buffer is written"
        assert bool((dk[:, :130] == 0).all()) and bool((dv[:, :130] == 0).all()), "dead keys: exact zeros"
        runs.append(buf.clone())
    assert torch.equal(runs[0], runs[1]), "bit-identical on a cloned mask tensor"
    ref, rnd = C.bwd64(q, k, v, o, do, md)
    _check(f"attn_mask_bwd deadkeys {family}", (dq, dk, dv), ref, rnd, lse, _lse64(q, k, md))


def test_more_than_64_key_tiles(K, cuda):
    """S = 4300: 68 key tiles - the dQ kernel reloads its flag register; band 300 plus the first 4 keys as a sink column."""
    S = 4300
    _run(K, cuda, "sink", 1, S, 4, 1, _band(S, 300, sink=4)[None, None], "kt68", blocked=True)


def test_more_than_64_query_blocks(K, cuda):
    """S = 8320: 65 query blocks - the dK/dV kernel reloads its flag register; the same band."""
    S = 8320
    _run(K, cuda, "sink", 1, S, 2, 1, _band(S, 300, sink=4)[None, None], "qb65", blocked=True)


@pytest.mark.parametrize("family", FAMILIES)
def test_causal_mask_given_densely(K, cuda, family):
    """The causal mask as bytes against the causal kernels on the same inputs: both inside the bars (bit-identity is printed only: the
    two forwards are different kernels)."""
    B, S, H, KVH = 1, 512, 8, 2
    mask = torch.ones(S, S, dtype=torch.bool).tril()[None, None]
    q, k, v, do, o, lse, g, md = _run(K, cuda, family, B, S, H, KVH, mask, "causal")
    o0, lse0 = K.attn_fwd(q, k, v)
    g0 = [torch.full_like(t, float("nan")) for t in (q, k, v)]
    K.attn_bwd(q, k, v, o0, do, lse0, *g0)
    ref, rnd = C.bwd64(q, k, v, o0, do, md)
    _check(f"attn_bwd causal kernels {family}", g0, ref, rnd, lse0, _lse64(q, k, md))
    same = [bool(torch.equal(a, b)) for a, b in zip((o, lse, *g), (o0, lse0, *g0))]
    print(f"[causal dense vs rule {family}] bit-identical o, lse, dq, dk, dv: {same}")
