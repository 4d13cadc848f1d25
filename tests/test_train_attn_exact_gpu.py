"""GPU: the training attention kernels - llx_attn_fwd / llx_attn_fwd_dropout and the backward routes of csrc/attn_bwd.hip (route (b) from
the causal mask, the doc_ids / prefix_len rule and a dense mask; route (a) through the dS^T scratch; the dropout builds; the rope
epilogues) - on the exact operand families of tests/train_attn_cases.py, over its table.  torch.equal on dQ, dK and dV and on the
selection forward, integer equality on the census forward, are the only bars; lse alone has a tolerance (attn_cases.LSE_REL against
float64, beside the integer check round(exp2(lse)) == count).  The only rows left out are the dq rows of the listed keyless rows.
Every call goes through strided operands: q | k | v as views of one fused row buffer whose gaps hold NaN, o and dO inside NaN-filled
buffers, dq / dk / dv inside larger buffers whose other elements keep a sentinel bit for bit, dq (and the forward's o) once at an
8-byte, not 16-byte, aligned address; every call is made twice and must repeat itself bit for bit, with the workspace memory poisoned
in between."""
import functools
import math

import pytest
import torch

from tests import attn_cases as A
from tests import infer_attn_cases as I
from tests import train_attn_cases as C

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
RNG = (20240607, 3)  # (seed, counter) of the dropout ticket
STREAM_ID = 5


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


class _Window:
    """A [B, S, heads, 128] tensor inside a larger flat buffer filled with the sentinel: rows 12 or 16 elements apart, one spare row
    before and after every batch element; narrow: rows 8 bytes off the 16-byte grid, every other one by its stride of 24 bytes mod 16."""

    def __init__(self, B, S, heads, cuda, narrow=False, fill=C.SENTINEL):
        ss = heads * C.HD + (12 if narrow else 16)
        sb, off = (S + 3) * ss, (2 * ss + 4) if narrow else (ss + 8)
        self.flat = torch.full((B * sb + 16,), fill, dtype=BF, device=cuda)
        self.geom = ((B, S, heads, C.HD), (sb, ss, C.HD, 1), off)
        self.t = self.flat.as_strided(*self.geom)
        assert (self.t.data_ptr() % 16 == 8) == narrow and self.t.data_ptr() % 8 == 0

    def put(self, x):
        self.t.copy_(x)
        return self.t

    def result(self, name):
        """The window on the host, after checking that every element outside it still holds the sentinel's bits."""
        inside = torch.zeros(self.flat.shape, dtype=torch.bool, device=self.flat.device)
        inside.as_strided(*self.geom).fill_(True)
        rest = self.flat.view(torch.int16)[~inside]
        want = torch.tensor([C.SENTINEL], dtype=BF).view(torch.int16).item()
        assert bool((rest == want).all()), f"{name}: elements outside the window were written"
        return self.t.contiguous().cpu()


def _operands(d, cuda):
    """q | k | v as views of fused rows [B, S, (H + 2 KVH) 128 + 8] and o, dO as windows, every gap NaN."""
    c = d["case"]
    w = (c.H + 2 * c.KVH) * C.HD
    rows = torch.full((c.B, c.S, w + 8), float("nan"), dtype=BF, device=cuda)
    rows[..., :c.H * C.HD] = d["q"].reshape(c.B, c.S, -1).to(cuda)
    rows[..., c.H * C.HD:(c.H + c.KVH) * C.HD] = d["k"].reshape(c.B, c.S, -1).to(cuda)
    rows[..., (c.H + c.KVH) * C.HD:w] = d["v"].reshape(c.B, c.S, -1).to(cuda)
    q = rows[..., :c.H * C.HD].view(c.B, c.S, c.H, C.HD)
    k = rows[..., c.H * C.HD:(c.H + c.KVH) * C.HD].view(c.B, c.S, c.KVH, C.HD)
    v = rows[..., (c.H + c.KVH) * C.HD:w].view(c.B, c.S, c.KVH, C.HD)
    assert c.S == 1 or (q.stride(1) == w + 8 and not q.is_contiguous())
    return q, k, v


def _poison(cuda, nbytes):
    """Fill memory of the size the next call's workspace takes with NaN and hand it back to the allocator."""
    junk = torch.full((max(1, nbytes // 4),), float("nan"), dtype=torch.float32, device=cuda)
    del junk


def _spec(K, c, cuda):
    if c.mode == "causal":
        return None
    doc, prefix = C.rule_operands(c)
    return K.MaskSpec(None if doc is None else doc.to(cuda), None if prefix is None else prefix.to(cuda))


def _dropout(cuda):
    return (C.DROP_T, torch.tensor(RNG, dtype=torch.int64, device=cuda), STREAM_ID)


@functools.lru_cache(maxsize=8)
def _expected_plain(cid, fam):
    return C.expected(cid, fam)


def _run_bwd(K, d, cuda, *, ds=False, dropout=None, narrow=False):
    """One backward through the wrapper (attn_bwd, or attn_mask_bwd with the case's mask form), twice; (dq, dk, dv) on the host."""
    from llx import _lib as L

    c = d["case"]
    q, k, v = _operands(d, cuda)
    o = _Window(c.B, c.S, c.H, cuda, fill=float("nan")).put(d["o"].to(cuda))
    do = _Window(c.B, c.S, c.H, cuda, fill=float("nan")).put(d["do"].to(cuda))
    lse = d["lse"].to(cuda)
    rope = d["rope"].to(cuda) if "rope" in d else None
    lib = L.load()
    ws = lib.llx_attn_bwd_workspace_bytes(c.B, c.S, c.H, c.KVH) + (lib.llx_attn_bwd_ds_bytes(c.B, c.S, c.H) if ds else 0)
    mask = C.mask_tensor(c, d["allow"], cuda) if c.mode == "mask" else None
    if mask is not None:
        assert (mask.stride(-2) > c.S) == (c.form == "strided")
    spec = _spec(K, c, cuda)
    outs = []
    old = K._ATTN_BWD_DS
    K._ATTN_BWD_DS = ds
    try:
        for _ in range(2):
            dq, dk, dv = _Window(c.B, c.S, c.H, cuda, narrow), _Window(c.B, c.S, c.KVH, cuda), _Window(c.B, c.S, c.KVH, cuda)
            _poison(cuda, ws)
            if mask is not None:
                K.attn_mask_bwd(q, k, v, o, do, lse, dq.t, dk.t, dv.t, mask, rope=rope)
            else:
                K.attn_bwd(q, k, v, o, do, lse, dq.t, dk.t, dv.t, spec, rope=rope, dropout=dropout)
            outs.append((dq.result(f"{c.id} dq"), dk.result(f"{c.id} dk"), dv.result(f"{c.id} dv")))
    finally:
        K._ATTN_BWD_DS = old
    for a, b, n in zip(outs[0], outs[1], ("dq", "dk", "dv")):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{c.id} {d['fam']}: a second identical call differs in {n}"
    return outs[0]


def _check_bwd(got, want, d, what):
    bad = C.same(got, want, d["keyless"])
    assert not bad, f"{d['case'].id} {d['fam']} {what}: {bad} differ\n{C.explain(got, want, d['keyless'])}"


@pytest.mark.parametrize("cid", list(C.CASES))
def test_attn_bwd_exact(K, cuda, cid):
    """Route (b) for every case (the dense masks through attn_mask_bwd in the case's mask form), route (a) where the case asks for it
    (the flagged case beyond 128 key tiles falls back to (b) inside llx_attn_bwd), rope and the narrow dq store as the case says."""
    c = C.CASES[cid]
    for fam in C.families_of(c):
        d = C.build(cid, fam)
        want = _expected_plain(cid, fam)
        _check_bwd(_run_bwd(K, d, cuda, narrow=c.narrow), want, d, "route (b)")
        if c.route_a:
            _check_bwd(_run_bwd(K, d, cuda, ds=True, narrow=c.narrow), want, d, f"route ({C.bwd_route(c, True)}) with the dS buffer")


@pytest.mark.parametrize("cid", [c.id for c in C.CASES.values() if c.dropout])
def test_attn_bwd_dropout_exact(K, cuda, cid):
    """p = 1/2: dV takes 2 keep P, dP takes 2 keep dP, the P in front of dS stays undropped; keep from kernels.attn_dropout_keep."""
    c = C.CASES[cid]
    drop = _dropout(cuda)
    keep = K.attn_dropout_keep(c.B, c.H, c.S, c.S, drop).cpu()
    assert 0.4 < float(keep.float().mean()) < 0.6 or c.S < 8
    for fam in C.families_of(c):
        d = C.build(cid, fam)
        want = C.expected(cid, fam, keep)
        _check_bwd(_run_bwd(K, d, cuda, dropout=drop, narrow=c.narrow), want, d, "dropout")


# ------------------------------------------------------------------------------------------------------------------ forward
def _run_fwd(K, d, cuda, *, dropout=None, narrow=False):
    """llx_attn_fwd on the fused-row views; with `narrow` through the C entry, o at an 8-byte aligned address.  (o [B, H, S, 128], lse)
    on the host, in the layout of tests/infer_attn_cases.py."""
    from llx import _lib as L

    c = d["case"]
    dd = {"case": c, "q": d["q"].transpose(1, 2), "k": d["k"].transpose(1, 2), "v": d["v"].transpose(1, 2)}
    q, k, v = _operands(dd, cuda)
    spec = _spec(K, c, cuda)
    outs = []
    for _ in range(2):
        if not narrow:
            o, lse = K.attn_fwd(q, k, v, spec, dropout=dropout)
            outs.append((o.cpu(), lse.cpu()))
            continue
        ow = _Window(c.B, c.S, c.H, cuda, narrow=True)
        lse = torch.full((c.B, c.H, c.S), float("nan"), device=cuda)
        dp = pp = fl = None
        if spec is not None:
            spec = spec.prepared(c.B, c.S, cuda)
            dp, pp, fl = spec.doc_ids, spec.prefix_len, spec._flags
        args = (L.ptr(q), q.stride(0), q.stride(1), L.ptr(k), k.stride(0), k.stride(1), L.ptr(v), v.stride(0), v.stride(1), L.ptr(ow.t), ow.t.stride(0),
                ow.t.stride(1), L.ptr(lse), L.ptr(dp), L.ptr(pp), L.ptr(fl), c.B, c.S, c.H, c.KVH, C.HD, 1.0 / math.sqrt(C.HD))
        if dropout is not None:
            L.check(L.load().llx_attn_fwd_dropout(*args, *K._dropout_operands(dropout, cuda, "attn_fwd"), L.stream()), "llx_attn_fwd_dropout")
        else:
            L.check(L.load().llx_attn_fwd(*args, L.stream()), "llx_attn_fwd")
        outs.append((ow.result(f"{c.id} o"), lse.cpu()))
    assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16)) and torch.equal(outs[0][1], outs[1][1]), f"{c.id}: a second identical call differs"
    return outs[0][0].transpose(1, 2).contiguous(), outs[0][1]


def _explain_fwd(o, d):
    lines = []
    B, H, S, _ = o.shape
    for b in range(B):
        for h in range(H):
            for m in range(S):
                if d["fam"] == "sel":
                    if not torch.equal(o[b, h, m], d["want"][b, h, m]):
                        lines.append(f"row (b {b}, h {h}, q {m}) target {int(d['tgt'][b, h, m])}: got {o[b, h, m, :4].tolist()} want {d['want'][b, h, m, :4].tolist()}")
                else:
                    got, want = I.census_decode(o, d)[b, h, m], d["count_d"][b, h, m]
                    bad = (got != want).nonzero().flatten().tolist()
                    if bad:
                        lines.append(f"row (b {b}, h {h}, q {m}) count {int(d['count'][b, h, m])}: dims {bad[:6]} got {got[bad[:6]].tolist()} want {want[bad[:6]].tolist()}")
                if len(lines) >= 6:
                    return "\n".join(lines)
    return "\n".join(lines)


@pytest.mark.parametrize("cid", [c.id for c in C.CASES.values() if c.mode != "mask"])
def test_attn_fwd_exact(K, cuda, cid):
    """Causal and rule mode on the sel / cen0 / cen1 families; lse against float64 and, on census rows up to 4096 keys, as an integer."""
    c = C.CASES[cid]
    for fam in C.FWD_FAMILIES:
        d = C.build_fwd(cid, fam)
        for narrow in ((False, True) if c.narrow else (False,)):
            o, lse = _run_fwd(K, d, cuda, narrow=narrow)
            assert I.family_ok(o, d), f"{cid} {fam} narrow={narrow}:\n{_explain_fwd(o, d)}"
            if fam == "sel":
                score = d["q"].double().mul(d["k"].double().repeat_interleave(c.G, 1).gather(2, d["tgt"][..., None].expand(-1, -1, -1, C.HD))).sum(-1) * C.SCALE
                assert A.lse_rel(lse, score) <= A.LSE_REL, (cid, A.lse_rel(lse, score))  # (every other key is 181 nats below: logsumexp = the target's score)
            else:
                small = d["count"] <= 4096
                assert torch.equal(torch.round(torch.exp2(lse.double()))[small].long(), d["count"][small]), f"{cid} {fam}: exp2(lse) is not the row's key count"
                assert A.lse_rel(lse, torch.log(d["count"].double())) <= A.LSE_REL


@pytest.mark.parametrize("cid", [c.id for c in C.CASES.values() if c.dropout])
def test_attn_fwd_dropout_exact(K, cuda, cid):
    """Census under p = 1/2: o count is twice the kept count per dim (decoded as round(o count / 2), the integer that bf16 cannot
    move), lse stays that of the undropped row."""
    c = C.CASES[cid]
    drop = _dropout(cuda)
    keep = K.attn_dropout_keep(c.B, c.H, c.S, c.S, drop).cpu()
    for fam in ("cen0", "cen1"):
        d = C.build_fwd(cid, fam)
        for narrow in ((False, True) if c.narrow else (False,)):
            o, lse = _run_fwd(K, d, cuda, dropout=drop, narrow=narrow)
            assert C.fwd_dropout_ok(o, d, keep), f"{cid} {fam} narrow={narrow}"
            small = d["count"] <= 4096
            assert torch.equal(torch.round(torch.exp2(lse.double()))[small].long(), d["count"][small])


def test_rule_flags_are_the_restated_classes(K, cuda):
    """The tile flags the rule kernels ran with are the classes the restated walks use."""
    for cid in ("docprefix_s449", "doc_s705", "prefix_s320"):
        c = C.CASES[cid]
        spec = _spec(K, c, cuda).prepared(c.B, c.S, cuda)
        fl = spec._flags.cpu().view(c.B, C.cdiv(c.S, C.BQ), C.cdiv(c.S, C.BKV))
        assert torch.equal(fl, C.flags_of(cid)), cid
