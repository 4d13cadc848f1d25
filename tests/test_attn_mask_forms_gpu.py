"""GPU: one bool mask handed to the four mask-taking attention wrappers in every form their shared normaliser (llx.kernels._mask_norm)
accepts - [Sq, Skv], [1, 1, Sq, Skv], an expanded-then-contiguous [B, 1, Sq, Skv], and a view with a strided last dim (a transposed
buffer, which the normaliser copies).  The kernels see the same bytes whatever the form, so outputs (and dq, dk, dv) must be
bit-identical across the forms: no tolerance.  One form per wrapper is also held against the float64 reference of
tests/attn_cases.py at the bars tests/test_attn_mask_gpu.py, tests/test_attn_mask_bwd_gpu.py and tests/test_attn_range_gpu.py use.
Shapes: B 2, H 4, KVH 2; Sq 5 x Skv 70 for attn_decode / attn_dense_fwd (a ragged second 64-key tile; Sq * H / KVH = 10 <= 16 decode
rows), S 130 for attn_mask_fwd / attn_mask_bwd (a full 128-row block plus a ragged one, three key tiles).  Every row keeps key 0:
no row is masked completely, no NaN."""
import pytest
import torch

from tests import attn_cases as C

pytestmark = pytest.mark.gpu

B, H, KVH, HD = 2, 4, 2, 128
FORMS = ("SqSkv", "11SqSkv", "B1SqSkv", "strided")


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


def _mask(Sq, Skv, seed):
    m = torch.rand(Sq, Skv, generator=torch.Generator().manual_seed(seed)) < 0.5
    m[:, 0] = True
    return m


def _forms(mask, cuda):
    """form -> a fresh device tensor holding `mask` [Sq, Skv] in that form."""
    md = mask.to(cuda)
    out = {"SqSkv": md.clone(), "11SqSkv": md.clone()[None, None], "B1SqSkv": md[None, None].expand(B, 1, *mask.shape).contiguous(),
           "strided": md.t().contiguous().t()}
    assert out["strided"].stride(-1) != 1 and all(torch.equal(f.expand(B, 1, *mask.shape), md.expand(B, 1, *mask.shape)) for f in out.values())
    return out


def _fwd_bars(label, got, want):
    err, cos = C.max_rel(got, want), C.worst_row_cos(got, want)
    print(f"[{label}] O {err:.2e} (bar {C.FWD_O_BAR:.0e})  cos {cos:.6f} (bar {C.FWD_O_COS})")
    assert not torch.isnan(got).any()
    assert err <= C.FWD_O_BAR and cos >= C.FWD_O_COS, (label, err, cos)


@pytest.fixture(scope="module")
def small(cuda):
    """Sq 5 queries continuing a 70-key cache: q [B,H,Sq,128], k / v [B,KVH,Skv,128], the mask forms, the float64 SDPA [B,H,Sq,128]."""
    Sq, Skv = 5, 70
    q_all, k_all, v_all, _ = (t.to(cuda) for t in C.make_case("unit", B, Skv, H, KVH, "forms"))
    q = q_all[:, Skv - Sq:].transpose(1, 2)
    k, v = k_all.transpose(1, 2).contiguous(), v_all.transpose(1, 2).contiguous()
    mask = _mask(Sq, Skv, 21)
    want, _ = C.sdpa64(q.transpose(1, 2), k_all, v_all, mask.to(cuda))  # [B,Sq,H,128]
    return q, k, v, _forms(mask, cuda), want.transpose(1, 2)


def test_attn_decode_takes_every_mask_form(K, small):
    q, k, v, forms, want = small
    Sq = q.shape[2]
    got = {f: K.attn_decode(q, k, v, m, K.mask_extent(m)).view(B, Sq, H, HD).transpose(1, 2) for f, m in forms.items()}
    _fwd_bars("attn_decode [Sq,Skv]", got["SqSkv"], want)
    for f in FORMS[1:]:
        assert torch.equal(got[f], got["SqSkv"]), f


def test_attn_dense_fwd_takes_every_mask_form(K, small):
    q, k, v, forms, want = small
    got = {f: K.attn_dense_fwd(q, k, v, m) for f, m in forms.items()}
    _fwd_bars("attn_dense_fwd [Sq,Skv]", got["SqSkv"], want)
    for f in FORMS[1:]:
        assert torch.equal(got[f], got["SqSkv"]), f


@pytest.fixture(scope="module")
def square(cuda):
    """S 130 training layout: q / do [B,S,H,128], k / v [B,S,KVH,128], the mask forms [.., S, S]."""
    S = 130
    q, k, v, do = (t.to(cuda) for t in C.make_case("unit", B, S, H, KVH, "forms"))
    mask = _mask(S, S, 22)
    return q, k, v, do, mask.to(cuda), _forms(mask, cuda)


def _mask_fwd(K, q, k, v, m):
    o, lse = K.attn_mask_fwd(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), m, lse=True)
    return o.view(q.shape), lse


def test_attn_mask_fwd_takes_every_mask_form(K, square):
    q, k, v, _, md, forms = square
    got = {f: _mask_fwd(K, q, k, v, m) for f, m in forms.items()}
    want, lse_ref = C.sdpa64(q, k, v, md)
    _fwd_bars("attn_mask_fwd [S,S]", got["SqSkv"][0], want)
    assert C.lse_rel(got["SqSkv"][1], lse_ref) <= C.LSE_REL
    for f in FORMS[1:]:
        assert torch.equal(got[f][0], got["SqSkv"][0]) and torch.equal(got[f][1], got["SqSkv"][1]), f
        assert torch.equal(K.attn_mask_flags(forms[f], B), K.attn_mask_flags(forms["SqSkv"], B)), f


def test_attn_mask_bwd_takes_every_mask_form(K, square):
    q, k, v, do, md, forms = square
    o, lse = _mask_fwd(K, q, k, v, forms["SqSkv"])
    got = {}
    for f, m in forms.items():
        g = [torch.full_like(t, float("nan")) for t in (q, k, v)]
        K.attn_mask_bwd(q, k, v, o, do, lse, *g, m)
        got[f] = g
    ref, rnd = C.bwd64(q, k, v, o, do, md)
    for n, a, b, r in zip(("dq", "dk", "dv"), got["SqSkv"], ref, rnd):
        ratio, cos = C.bwd_err(a, b, r)
        print(f"[attn_mask_bwd [S,S]] {n} {ratio:.3f} of bar, cos {cos:.6f} (bar {C.BWD_COS})")
        assert ratio <= 1.0 and cos >= C.BWD_COS, (n, ratio, cos)
    for f in FORMS[1:]:
        for n, a, b in zip(("dq", "dk", "dv"), got[f], got["SqSkv"]):
            assert torch.equal(a, b), (f, n)
