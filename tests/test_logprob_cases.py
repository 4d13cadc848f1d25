"""CPU: the float64 restatement of the token log-probability kernels (tests/logprob_cases.py) against torch - forward values against
-F.cross_entropy(..., reduction="none", ignore_index=-100) in float64, the top1 tie rule, and the backward formula against autograd of
that expression with a random upstream gradient.  The GPU tests compare the kernels with this restatement."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import logprob_cases as C


def _all_batches():
    for T, V, ld, rows in C.SHAPES:
        if rows is None:
            for lg, lb in C.batches(T, V, ld):
                yield V, lg[:, :V], lb


def test_case_table_holds_every_row_kind():
    for T, V, ld, rows in C.SHAPES:
        bs = C.batches(T, V, ld)
        assert T * len(bs) >= C.N_KINDS
        for lg, lb in bs:
            assert lg.dtype is torch.bfloat16 and lg.shape == (T, ld) and lb.shape == (T,)
            assert ld == V or (lg[:, V:].float() == C.PAD_SENTINEL).all()
            assert (lg[:, :V].float() < C.PAD_SENTINEL).all()
    labels = torch.cat([lb for lg, lb in C.batches(1, 8, 8)])
    assert labels.tolist() == [0, 7, 7, 7, -100, 4, 6, 5, 1, 4]
    assert {float(g) for r in range(4) for g in C.grads(1, r)} == {float(torch.tensor(g, dtype=torch.float32)) for g in C.GRADS}


def test_restatement_forward_matches_cross_entropy():
    for V, x, lb in _all_batches():
        logp, lse, top1 = C.ref_fwd(x, lb)
        want = -F.cross_entropy(x.double(), lb, reduction="none", ignore_index=-100)
        torch.testing.assert_close(logp, want, atol=1e-12, rtol=1e-12)
        assert (logp[lb == -100] == 0).all() and (lse[lb == -100] == 0).all() and (top1[lb == -100] == -1).all()
        keep = lb != -100
        torch.testing.assert_close(lse[keep], torch.logsumexp(x.double(), 1)[keep], atol=0, rtol=0)


def test_restatement_top1_and_special_rows():
    T, V, ld, _ = C.SHAPES[3]
    (lg, lb), = C.batches(T, V, ld)
    logp, lse, top1 = C.ref_fwd(lg, lb)
    for t in range(T):
        kind = t % C.N_KINDS
        row = lg[t].double()
        if kind != 4:
            assert row[top1[t]] == row.max() and (row[: top1[t]] < row.max()).all()  # the lowest index among ties
        if kind == 5:
            assert top1[t] == 0 and abs(logp[t].item() + math.log(V)) < 1e-12
        if kind == 6:
            assert top1[t] == V // 3 and row[V - 2] == row[V // 3]
        if kind == 7:
            assert top1[t] == lb[t] and -1e-30 < logp[t].item() <= 0.0
        if kind == 8:
            assert -83.0 < logp[t].item() < -79.0
        if kind == 9:
            assert lse[t].item() < -2.8e4 and -3000.0 < logp[t].item() < 0.0
    # a label outside [0, V) other than -100: its logit counts as 0 (the loss kernel's rule), logp = -lse
    x = lg[:2].clone()
    logp2, lse2, _ = C.ref_fwd(x, torch.tensor([V, -5]))
    torch.testing.assert_close(logp2, -lse2, atol=0, rtol=0)
    # the compacted-row limit: zeros from the end of the 256-row tile that holds the last labelled row
    logp3, lse3, top13 = C.ref_fwd(lg, lb, rows=3)
    assert torch.equal(logp3[:256], logp[:256]) and (logp3[256:] == 0).all() and (lse3[256:] == 0).all() and (top13[256:] == 0).all()


@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_restatement_backward_matches_autograd(rot):
    gen = torch.Generator().manual_seed(7 + rot)
    for V, x, lb in _all_batches():
        T = x.shape[0]
        for g in (C.grads(T, rot), torch.randn(T, generator=gen)):
            xr = x.double().requires_grad_()
            (-F.cross_entropy(xr, lb, reduction="none", ignore_index=-100)).backward(g.double())
            got = C.ref_bwd(x, lb, g)
            torch.testing.assert_close(got, xr.grad, atol=1e-12 * max(1.0, g.abs().max().item()), rtol=1e-9)
            assert (got[lb == -100] == 0).all() and (got[g == 0] == 0).all()
