"""GPU: llx_attn_mask_fwd, the MFMA tile loop of the training forward driven by a dense bool mask (KV-cache prefill and explicit
masks broadcast over heads, modelling/llama.py:_run_dense), against a float64 SDPA computed on the device.

Inputs come from tests/attn_cases.py (families unit, diag, sink); the bars are the project's forward bars C.FWD_O_BAR / C.FWD_O_COS,
which the training kernel meets with the same arithmetic (bf16 P, bf16 O).  The only rows left out of a comparison are the rows a
case masks completely on purpose: they must be NaN (SDPA's softmax over -inf) in every head, their neighbours finite.  The shapes
are the smallest at which each path of the kernel runs: under one wave's rows, a ragged second workgroup, a 128-row flag block
partly past the end, a key count off the 64-key tile with whole skipped tiles behind the live range, more than 64 key tiles (one
flag register), a mask whose every tile is partly masked, mask rows of odd length (unaligned 4-byte mask reads)."""
import pytest
import torch

from tests import attn_cases as C

pytestmark = pytest.mark.gpu

FAMILIES = ("unit", "diag", "sink")
HD = 128


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


def _sdpa64_rows(q, k, v, mask):
    """float64 SDPA of q [B,H,Sq,128] against k / v [B,KVH,Skv,128] (GQA by head grouping) -> rows [B, Sq, H*128]."""
    g = q.shape[1] // k.shape[1]
    s = (q.double() @ k.double().repeat_interleave(g, dim=1).transpose(-1, -2)) * C.SCALE
    o = torch.softmax(s.masked_fill(~mask, float("-inf")), dim=-1) @ v.double().repeat_interleave(g, dim=1)
    return o.transpose(1, 2).reshape(q.shape[0], q.shape[2], -1)


def _row_buffer(q_rows, k_rows=None, v_rows=None):
    """The fused q|k|v row buffer of _run_dense, [B, S, (H + 2 KVH) * 128], and its strided q (k, v) views [B, heads, S, 128]."""
    B, S, H, _ = q_rows.shape
    KVH = k_rows.shape[2] if k_rows is not None else 2
    buf = torch.zeros(B, S, (H + 2 * KVH) * HD, dtype=torch.bfloat16, device=q_rows.device)
    buf[..., : H * HD] = q_rows.reshape(B, S, H * HD)
    if k_rows is not None:
        buf[..., H * HD : (H + KVH) * HD] = k_rows.reshape(B, S, KVH * HD)
        buf[..., (H + KVH) * HD :] = v_rows.reshape(B, S, KVH * HD)
    q = buf[..., : H * HD].unflatten(-1, (H, HD)).transpose(1, 2)
    k = buf[..., H * HD : (H + KVH) * HD].unflatten(-1, (KVH, HD)).transpose(1, 2)
    v = buf[..., (H + KVH) * HD :].unflatten(-1, (KVH, HD)).transpose(1, 2)
    return q, k, v


def _check(label, got, want, dead_rows=None):
    """got / want [B, Sq, H*128]; dead_rows: bool [B, Sq] of the rows masked completely on purpose."""
    B, Sq, _ = got.shape
    live = torch.ones(B, Sq, dtype=torch.bool, device=got.device)
    if dead_rows is not None:
        assert torch.isnan(got[dead_rows]).all(), f"{label}: a fully masked row is NaN in every head"
        live = ~dead_rows
    assert not torch.isnan(got[live]).any(), f"{label}: NaN in a row that has allowed keys"
    g, w = got[live].reshape(-1, HD), want[live].reshape(-1, HD)
    err, cos = C.max_rel(g, w), C.worst_row_cos(g, w)
    print(f"[attn_mask_fwd {label}] O {err:.2e} (bar {C.FWD_O_BAR:.0e})  cos {cos:.6f} (bar {C.FWD_O_COS})")
    assert err <= C.FWD_O_BAR, f"{label}: O max-norm error {err:.3e}"
    assert cos >= C.FWD_O_COS, f"{label}: worst row cosine {cos:.6f}"


def _cache_case(cuda, family, Sq, live=620, Smax=700, H=8, KVH=2, tag="cache"):
    """A chunk of Sq tokens continuing a cache: contiguous caches [1, KVH, Smax, 128] with `live` keys written (the rest zeros, as
    KVCache leaves them), q the strided view of a row buffer, mask = tril[pos] over the whole cache."""
    q_all, k_all, v_all, _ = (t.to(cuda) for t in C.make_case(family, 1, live, H, KVH, tag))
    kc = torch.zeros(1, KVH, Smax, HD, dtype=torch.bfloat16, device=cuda)
    vc = torch.zeros_like(kc)
    kc[:, :, :live] = k_all.transpose(1, 2)
    vc[:, :, :live] = v_all.transpose(1, 2)
    q, _, _ = _row_buffer(q_all[:, live - Sq :])
    pos = torch.arange(live - Sq, live, device=cuda)
    mask = torch.ones(Smax, Smax, dtype=torch.bool, device=cuda).tril()[None, None, pos]  # as Llama.forward builds it
    return q, kc, vc, mask


@pytest.mark.parametrize("Sq", [17, 300, 620])
@pytest.mark.parametrize("family", FAMILIES)
def test_cache_layout_chunk_continuing_a_cache(K, cuda, family, Sq):
    """Case 1: B 1, H 8, KVH 2, 620 live keys of a 700-position cache (not a multiple of 64; whole class-0 tiles behind them)."""
    q, kc, vc, mask = _cache_case(cuda, family, Sq)
    got = K.attn_mask_fwd(q, kc, vc, mask)
    assert got.shape == (1, Sq, 8 * HD)
    _check(f"cache {family} Sq={Sq}", got, _sdpa64_rows(q, kc, vc, mask))


@pytest.mark.parametrize("family", FAMILIES)
def test_row_buffer_layout_prefix_lm_and_left_padding(K, cuda, family):
    """Case 2: k / v as views of the q|k|v row buffer, B 2, Sq = Skv = 333 (mask rows of odd length), mask [2, 1, 333, 333]: sample 0
    prefix-LM (prefix 150), sample 1 causal with 70 left-padding keys masked (a class-0 tile first, then a partial one) and one row
    fully masked: NaN in every head, its neighbours finite."""
    B, S, H, KVH = 2, 333, 8, 2
    q_r, k_r, v_r, _ = (t.to(cuda) for t in C.make_case(family, B, S, H, KVH, "rows"))
    q, k, v = _row_buffer(q_r, k_r, v_r)
    idx = torch.arange(S, device=cuda)
    causal = idx[:, None] >= idx[None, :]
    eye = idx[:, None] == idx[None, :]  # a padding row keeps its own key, as padded batches are built (no NaN rows by accident)
    mask = torch.stack([causal | (idx[None, :] < 150), (causal & (idx[None, :] >= 70)) | eye])[:, None].contiguous()  # [2, 1, S, S]
    mask[1, 0, 200] = False  # the one row masked completely on purpose
    dead = torch.zeros(B, S, dtype=torch.bool, device=cuda)
    dead[1, 200] = True
    assert bool((~mask[:, 0].any(-1) == dead).all())
    fl = K.attn_mask_flags(mask, B).view(B, 3, 6)
    assert fl[1, 1].tolist()[:2] == [0, 1], "sample 1, rows 128..255: the padding tile is skipped, the next one partly masked"
    got = K.attn_mask_fwd(q, k, v, mask)
    _check(f"rows {family}", got, _sdpa64_rows(q, k, v, mask), dead)
    assert not torch.isnan(got[1, 199]).any() and not torch.isnan(got[1, 201]).any()


@pytest.mark.parametrize("family", FAMILIES)
def test_more_key_tiles_than_one_flag_register(K, cuda, family):
    """Case 3: Skv 4300 = 68 key tiles (a flag register holds 64), Sq 70 at positions 4230..4299, H 4, KVH 1."""
    q, kc, vc, mask = _cache_case(cuda, family, 70, live=4300, Smax=4300, H=4, KVH=1, tag="chunk")
    got = K.attn_mask_fwd(q, kc, vc, mask)
    _check(f"68 tiles {family}", got, _sdpa64_rows(q, kc, vc, mask))


@pytest.mark.parametrize("family", FAMILIES)
def test_mask_with_holes(K, cuda, family):
    """Case 4: 50 % random keys, broadcast over heads, each row's own key kept: every tile is class 1.  Sq 100, Skv 200."""
    Sq, Skv, H, KVH = 100, 200, 8, 2
    q_all, k_all, v_all, _ = (t.to(cuda) for t in C.make_case(family, 1, Skv, H, KVH, "holes"))
    q, _, _ = _row_buffer(q_all[:, Skv - Sq :])
    k, v = k_all.transpose(1, 2).contiguous(), v_all.transpose(1, 2).contiguous()
    g = torch.Generator().manual_seed(11)
    mask = torch.rand(Sq, Skv, generator=g) < 0.5
    mask[torch.arange(Sq), torch.arange(Skv - Sq, Skv)] = True
    mask = mask.to(cuda)
    fl = K.attn_mask_flags(mask, 1)
    assert fl.tolist() == [1, 1, 1, 1], "every 128 x 64 tile of this mask is partly masked"
    got = K.attn_mask_fwd(q, k, v, mask)
    _check(f"holes {family}", got, _sdpa64_rows(q, k, v, mask))


@pytest.mark.parametrize("family", FAMILIES)
def test_rows_of_tril_in_shuffled_order(K, cuda, family):
    """Case 5: a non-monotone input_pos: rows of tril gathered in shuffled order.  Sq 96, Skv 256."""
    Sq, Skv, H, KVH = 96, 256, 8, 2
    q_all, k_all, v_all, _ = (t.to(cuda) for t in C.make_case(family, 1, Skv, H, KVH, "shuffle"))
    pos = torch.randperm(Skv, generator=torch.Generator().manual_seed(5))[:Sq].to(cuda)
    q, _, _ = _row_buffer(q_all[:, pos])
    k, v = k_all.transpose(1, 2).contiguous(), v_all.transpose(1, 2).contiguous()
    mask = torch.ones(Skv, Skv, dtype=torch.bool, device=cuda).tril()[None, None, pos]
    got = K.attn_mask_fwd(q, k, v, mask)
    _check(f"shuffled {family}", got, _sdpa64_rows(q, k, v, mask))


def test_tile_flags_of_a_chunk_mask(K, cuda):
    """The tile classes of case 1 at Sq 300: 3 row blocks x 11 key tiles; keys >= 620 are class 0, the ragged last tile is never 2."""
    _, _, _, mask = _cache_case(cuda, "unit", 300)
    fl = K.attn_mask_flags(mask, 1).view(3, 11).cpu()
    m = torch.nn.functional.pad(mask[0, 0].cpu(), (0, 11 * 64 - 700, 0, 3 * 128 - 300), value=False)
    rows_in = torch.nn.functional.pad(torch.ones(300, dtype=torch.bool), (0, 84))
    for qb in range(3):
        for kt in range(11):
            tile = m[qb * 128 : qb * 128 + 128, kt * 64 : kt * 64 + 64][rows_in[qb * 128 : qb * 128 + 128]]
            want = 0 if not tile.any() else (2 if tile.all() else 1)
            assert int(fl[qb, kt]) == want, (qb, kt, int(fl[qb, kt]), want)
    assert fl[:, 10].tolist() == [0, 0, 0] and fl[2, 9] == 1


@pytest.mark.parametrize("Sq", [17, 300, 620])
def test_repeatable_and_writes_only_its_rows(K, cuda, Sq):
    """Case 6: a second run of case 1 is bit-identical, and the output buffer, allocated inside a larger poisoned one, is untouched
    outside [B, Sq, H*128]."""
    q, kc, vc, mask = _cache_case(cuda, "diag", Sq)
    n = Sq * 8 * HD
    big = torch.full((n + 2 * 4096,), 12345.0, dtype=torch.bfloat16, device=cuda)
    out = big[4096 : 4096 + n].view(1, Sq, 8 * HD)
    got = K.attn_mask_fwd(q, kc, vc, mask, out=out)
    assert got.data_ptr() == out.data_ptr()
    first = got.clone()
    assert bool((big[:4096] == 12345.0).all()) and bool((big[4096 + n :] == 12345.0).all()), "bytes outside the output were written"
    again = K.attn_mask_fwd(q, kc, vc, mask.clone())  # a fresh mask tensor: the flags are rebuilt as well
    assert torch.equal(first, again)
    _check(f"poisoned buffer Sq={Sq}", first, _sdpa64_rows(q, kc, vc, mask))
