"""GPU: the inference attention kernels - llx_attn_decode (split walk + combine), llx_attn_dense_fwd, llx_attn_mask_fwd - on the two exact
operand families of tests/infer_attn_cases.py, over its table: every row class, mask form, split count, extent form and tile class the
launchers distinguish.  Selection must return V[target] bit for bit (torch.equal), census must name every attended key as an integer;
rows without any allowed key are NaN and their neighbours exact.  No tolerance anywhere: a miss here is a wrong key set or a wrong
address, not rounding.  Every decode call goes through strided operands: q as the view of a fused q|k|v row buffer, the caches as
slices of longer allocations poisoned beyond the slice, out= inside a larger buffer whose other bytes keep a sentinel."""
import math

import pytest
import torch

from tests import infer_attn_cases as C

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TAIL = 19  # cache positions allocated beyond Skv


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


def _explain(o, d):
    """The first rows that miss, for the assertion message."""
    c = d["case"]
    lines = []
    for b in range(c.B):
        for h in range(c.H):
            for m in range(c.M):
                if d["fam"] == "sel":
                    w, g = d["want"][b, h, m].float(), o[b, h, m].float()
                    if not torch.equal(torch.nan_to_num(w, nan=-7.0), torch.nan_to_num(g, nan=-7.0)):
                        lines.append(f"row (b {b}, h {h}, m {m}) target {int(d['tgt'][b, h, m])}: got {g[:4].tolist()} want {w[:4].tolist()}")
                else:
                    want = d["count_d"][b, h, m] if int(d["count"][b, h, m]) else torch.full((C.HD,), -1)
                    got = C.census_decode(o, d)[b, h, m]
                    bad = (got != want).nonzero().flatten().tolist()
                    if bad:
                        lines.append(f"row (b {b}, h {h}, m {m}) count {int(d['count'][b, h, m])}: dims {bad[:6]} got {got[bad[:6]].tolist()} want {want[bad[:6]].tolist()}")
                if len(lines) >= 6:
                    return "\n".join(lines)
    return "\n".join(lines)


def _check(o, d, what):
    assert o.shape == d["q"].shape and o.dtype is BF
    assert C.family_ok(o, d), f"{d['case'].id} {d['fam']} {what}:\n{_explain(o, d)}"


def _fused_q(d, cuda):
    """q [B, H, M, 128] as the strided view of rows [B, M, (H + 2 KVH) 128] whose k | v part is NaN."""
    c = d["case"]
    rows = torch.full((c.B, c.M, (c.H + 2 * c.KVH) * C.HD), float("nan"), dtype=BF, device=cuda)
    rows[..., :c.H * C.HD] = d["q"].to(cuda).transpose(1, 2).reshape(c.B, c.M, c.H * C.HD)
    return rows[..., :c.H * C.HD].view(c.B, c.M, c.H, C.HD).transpose(1, 2)


def _cache(t, cuda):
    """[B, KVH, Skv, 128] as the slice of an allocation TAIL positions longer, 1e4 beyond the slice."""
    B, KVH, S, hd = t.shape
    full = torch.full((B, KVH, S + TAIL, hd), 1e4, dtype=BF, device=cuda)
    full[:, :, :S] = t.to(cuda)
    return full[:, :, :S]


class _Out:
    """out= of attn_decode inside a larger buffer: rows 1 .. M of M + 2, columns 128 .. 128 + H 128 of H 128 + 256."""

    def __init__(self, c, cuda):
        self.c = c
        self.big = torch.full((c.B, c.M + 2, c.H * C.HD + 256), C.SENTINEL, dtype=BF, device=cuda)
        self.out = self.big[:, 1:c.M + 1, C.HD:C.HD + c.H * C.HD]

    def result(self):
        """[B, H, M, 128] on the host, after checking that nothing outside the window was written."""
        c = self.c
        rest = self.big.clone()
        rest[:, 1:c.M + 1, C.HD:C.HD + c.H * C.HD] = C.SENTINEL
        assert bool((rest == C.SENTINEL).all()), f"{c.id}: bytes outside out= were written"
        return self.out.reshape(c.B, c.M, c.H, C.HD).transpose(1, 2).contiguous().cpu()


def _extent(d, cuda, use_ext):
    return torch.tensor([d["ext"]], dtype=torch.int32, device=cuda) if use_ext else None


def _decode_wrapper(K, d, cuda, use_ext):
    c = d["case"]
    q, kc, vc, mask = _fused_q(d, cuda), _cache(d["k"], cuda), _cache(d["v"], cuda), d["mask"].to(cuda)
    assert kc.stride(1) != c.Skv * C.HD and q._base.shape[-1] == (c.H + 2 * c.KVH) * C.HD
    o = _Out(c, cuda)
    ret = K.attn_decode(q, kc, vc, mask, extent=_extent(d, cuda, use_ext), out=o.out)
    assert ret.data_ptr() == o.out.data_ptr()
    first = o.result()
    K.attn_decode(q, kc, vc, mask, extent=_extent(d, cuda, use_ext), out=o.out)
    assert torch.equal(first.view(torch.int16), o.result().view(torch.int16)), f"{c.id}: a second identical call differs"
    return first


def _decode_entry(K, d, cuda, use_ext):
    """llx_attn_decode itself, with the nsplit of the case and a workspace of its own."""
    from llx import _lib as L

    c = d["case"]
    q, kc, vc = _fused_q(d, cuda), _cache(d["k"], cuda), _cache(d["v"], cuda)
    m, m_sb, m_sh = K._mask_norm(d["mask"].to(cuda), c.B, c.M, c.Skv, c.H)
    lib = L.load()
    ws = torch.full((lib.llx_attn_decode_workspace_bytes(c.B, c.H, c.M, c.nsplit) // 4,), float("nan"), device=cuda)
    o = _Out(c, cuda)
    o4 = o.out.view(c.B, c.M, c.H, C.HD)
    L.check(lib.llx_attn_decode(L.ptr(q), q.stride(0), q.stride(1), q.stride(2), L.ptr(kc), L.ptr(vc), kc.stride(0), kc.stride(1), kc.stride(2), L.ptr(o.out),
                                o4.stride(0), o4.stride(2), o4.stride(1), L.ptr(m), m_sb, m_sh, m.stride(2), L.ptr(_extent(d, cuda, use_ext)), L.ptr(ws),
                                c.B, c.H, c.KVH, c.M, c.Skv, c.nsplit, C.HD, 1.0 / math.sqrt(C.HD), L.stream()), "llx_attn_decode")
    return o.result()


DECODE = [c.id for c in C.cases_of("decode")]


@pytest.mark.parametrize("cid", DECODE)
def test_attn_decode_exact(K, cuda, cid):
    c = C.CASES[cid]
    run = _decode_entry if c.nsplit else _decode_wrapper
    if not c.nsplit:
        assert K._decode_nsplit(c.B, c.KVH, c.Skv) == c.plan().nsplit
    for fam in C.FAMILIES:
        d = C.build(cid, fam)
        for use_ext in (True, False):
            _check(run(K, d, cuda, use_ext), d, f"extent {'on the device' if use_ext else 'None'}")


def test_attn_decode_workspace_reuse(K, cuda):
    """The cached workspace grows with the largest call; a larger call (more rows, 128 splits) between two equal smaller ones must not
    change the second one's result, in either family."""
    small, large = "dec_g2m3_head", "dec_s4101_g2m3"
    for fam in ("sel", "cen0"):
        ds, dl = C.build(small, fam), C.build(large, fam)
        a = _decode_wrapper(K, ds, cuda, True)
        _check(_decode_wrapper(K, dl, cuda, False), dl, "between")
        b = _decode_wrapper(K, ds, cuda, True)
        _check(a, ds, "before")
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("cid", [c.id for c in C.cases_of("dense")])
def test_attn_dense_fwd_exact(K, cuda, cid):
    """q, k and v as strided views: q of fused rows, k / v of longer allocations."""
    for fam in C.FAMILIES:
        d = C.build(cid, fam)
        o = K.attn_dense_fwd(_fused_q(d, cuda), _cache(d["k"], cuda), _cache(d["v"], cuda), d["mask"].to(cuda))
        _check(o.cpu(), d, "")


@pytest.mark.parametrize("cid", [c.id for c in C.cases_of("prefill")])
def test_attn_mask_fwd_exact(K, cuda, cid):
    """The prefill route: q as the transposed view of fused rows (head stride 128), k / v cache slices, the mask rows c.pad bytes apart
    beyond Skv (odd row strides), [1 | B, 1, Sq, Skv]."""
    c = C.CASES[cid]
    for fam in C.FAMILIES:
        d = C.build(cid, fam)
        rows = torch.zeros(c.B, 1, c.M, c.Skv + c.pad, dtype=torch.bool, device=cuda)
        rows[..., :c.Skv] = d["mask"].to(cuda)
        mask = rows[..., :c.Skv]
        assert mask.stride(2) == c.Skv + c.pad
        o = K.attn_mask_fwd(_fused_q(d, cuda), _cache(d["k"], cuda), _cache(d["v"], cuda), mask)
        assert o.shape == (c.B, c.M, c.H * C.HD)
        _check(o.view(c.B, c.M, c.H, C.HD).transpose(1, 2).cpu(), d, "")
        if fam == "sel":  # the tile classes the kernel ran with are the restated ones
            fl = K.attn_mask_flags(mask, c.B).cpu().view(c.B, -(-c.M // 128), -(-c.Skv // 64))
            assert torch.equal(fl, C.tile_classes(d["mask4"][:, 0]))
