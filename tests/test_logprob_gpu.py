"""GPU: the token log-probability row kernels (csrc/logprob.hip) against their float64 restatement (tests/logprob_cases.py) on the same
bf16 logits, at the shapes where a 512-thread row kernel over 16-byte chunks can go wrong and over the row kinds of the case table.
Bars as test_cross_entropy (tests/test_kernels_gpu.py) holds the same quantities to: logp / lse atol 1e-4, rtol 1e-5; d logits (stored
in bf16) rtol 2^-7, atol 1e-6 * max(1, |g[t]|)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import logprob_cases as C  # noqa: E402


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


def _rows_arg(rows, cuda):
    return None if rows is None else torch.tensor([rows], dtype=torch.int32, device=cuda)


@pytest.mark.parametrize("T,V,ld,rows", C.SHAPES)
def test_logprob_rows_fwd(K, cuda, T, V, ld, rows):
    for lg, lb in C.batches(T, V, ld):
        want_logp, want_lse, want_top1 = C.ref_fwd(lg[:, :V], lb, rows)
        buf = lg.to(cuda)
        logp, lse, top1 = K.logprob_rows_fwd(buf[:, :V], lb.to(cuda), rows=_rows_arg(rows, cuda), want_top1=True)
        assert logp.dtype is torch.float32 and lse.dtype is torch.float32 and top1.dtype is torch.int32
        torch.testing.assert_close(logp.cpu().double(), want_logp, atol=1e-4, rtol=1e-5)
        torch.testing.assert_close(lse.cpu().double(), want_lse, atol=1e-4, rtol=1e-5)
        assert torch.equal(top1.cpu(), want_top1)
        ign = lb == -100
        if rows is not None:
            ign[256:] = False  # past the row limit everything is zero, top1 included (checked below)
        assert (logp.cpu()[ign] == 0).all() and (lse.cpu()[ign] == 0).all() and (top1.cpu()[ign] == -1).all()  # exact zeros
        if rows is not None:
            assert (logp.cpu()[256:] == 0).all() and (lse.cpu()[256:] == 0).all() and (top1.cpu()[256:] == 0).all()
        assert torch.equal(buf.cpu(), lg)  # the logits are only read
        # without top1, and a repeat launch: bit-identical
        logp2, lse2, none = K.logprob_rows_fwd(buf[:, :V], lb.to(cuda), rows=_rows_arg(rows, cuda))
        assert none is None and torch.equal(logp2, logp) and torch.equal(lse2, lse)
        logp3, lse3, top13 = K.logprob_rows_fwd(buf[:, :V], lb.to(cuda), rows=_rows_arg(rows, cuda), want_top1=True)
        assert torch.equal(logp3, logp) and torch.equal(lse3, lse) and torch.equal(top13, top1)


@pytest.mark.parametrize("T,V,ld,rows", C.SHAPES)
def test_logprob_rows_bwd(K, cuda, T, V, ld, rows):
    lim = T if rows is None else min(T, (rows + 255) // 256 * 256)
    for lg, lb in C.batches(T, V, ld):
        _, lse, _ = K.logprob_rows_fwd(lg.to(cuda)[:, :V], lb.to(cuda), rows=_rows_arg(rows, cuda))
        for rot in range(4):
            g = C.grads(T, rot)
            want = C.ref_bwd(lg[:, :V], lb, g)
            # out of place, into a sentinel-filled buffer: the pad columns and the rows past the limit stay untouched
            out = torch.full((T, ld), C.OUT_SENTINEL, dtype=torch.bfloat16, device=cuda)
            src = lg.to(cuda)
            got = K.logprob_rows_bwd(src[:, :V], lb.to(cuda), lse, g.to(cuda), rows=_rows_arg(rows, cuda), out=out[:, :V])
            assert got.data_ptr() == out.data_ptr() and torch.equal(src.cpu(), lg)
            o = out.cpu().float()
            assert (o[:, V:] == C.OUT_SENTINEL).all() and (o[lim:] == C.OUT_SENTINEL).all()
            err = (o[:lim, :V].double() - want[:lim]).abs()
            bound = 1e-6 * g[:lim].abs().clamp_min(1.0).double()[:, None] + 2 ** -7 * want[:lim].abs()
            bad = (err > bound).nonzero()
            assert bad.numel() == 0, f"rot {rot}: {bad.shape[0]} elements off, first (row, col) {bad[0].tolist()}: err {err[tuple(bad[0])]:.3e}"
            zero = ((lb == -100) | (g == 0))[:lim]
            assert (o[:lim, :V][zero] == 0).all()  # ignored rows and rows with g == 0: exact zero rows
            # in place: bit-identical to out of place; the pad columns keep the logits' sentinel
            inpl = lg.to(cuda)
            got2 = K.logprob_rows_bwd(inpl[:, :V], lb.to(cuda), lse, g.to(cuda), rows=_rows_arg(rows, cuda))
            assert got2.data_ptr() == inpl.data_ptr()
            assert torch.equal(inpl[:lim, :V], out[:lim, :V]) and torch.equal(inpl[:, V:].cpu(), lg[:, V:]) and torch.equal(inpl[lim:].cpu(), lg[lim:])
            # a repeat launch: bit-identical
            out2 = torch.full((T, ld), C.OUT_SENTINEL, dtype=torch.bfloat16, device=cuda)
            K.logprob_rows_bwd(src[:, :V], lb.to(cuda), lse, g.to(cuda), rows=_rows_arg(rows, cuda), out=out2[:, :V])
            assert torch.equal(out2, out)


def test_logprob_rows_out_of_range_label(K, cuda):
    """A label outside [0, V) other than -100 is treated as the loss kernel treats it: its logit counts as 0, no one-hot term."""
    T, V, ld, _ = C.SHAPES[1]
    lg, _ = C.batches(T, V, ld)[0]
    lb = torch.tensor([V, -5, V + 7])
    logp, lse, _ = K.logprob_rows_fwd(lg.to(cuda), lb.to(cuda))
    want_logp, want_lse, _ = C.ref_fwd(lg, lb)
    torch.testing.assert_close(logp.cpu().double(), want_logp, atol=1e-4, rtol=1e-5)
    torch.testing.assert_close(lse.cpu().double(), want_lse, atol=1e-4, rtol=1e-5)
    g = torch.tensor([1.0, -1.0 / 7.0, 1.0])
    d = K.logprob_rows_bwd(lg.to(cuda), lb.to(cuda), lse, g.to(cuda), out=torch.empty(T, V, dtype=torch.bfloat16, device=cuda))
    torch.testing.assert_close(d.cpu().double(), C.ref_bwd(lg, lb, g), rtol=2 ** -7, atol=1e-6)


@pytest.mark.parametrize("T", [1, 300, 1025])
def test_logprob_map_rows(K, cuda, T):
    """The [T] vectors between positions and compacted rows: through inv (scatter, fills at the ignored positions) and through idx (gather)."""
    gen = torch.Generator().manual_seed(T)
    lb = torch.randint(0, 50, (T,), generator=gen)
    lb[torch.rand(T, generator=gen) < 0.4] = -100
    idx, inv, _, cnt = K.head_compact_index(lb.to(cuda))
    n = int((lb != -100).sum())
    assert int(cnt) == n
    src = torch.randn(T, generator=gen)
    src_i = torch.randint(0, 1000, (T,), generator=gen).to(torch.int32)
    keep = lb != -100
    want, want_i = torch.full((T,), 7.5), torch.full((T,), -1, dtype=torch.int32)
    want[keep], want_i[keep] = src[:n], src_i[:n]
    got, got_i = K.logprob_map_rows(inv, src.to(cuda), 7.5, src_i.to(cuda), -1)
    assert torch.equal(got.cpu(), want) and torch.equal(got_i.cpu(), want_i)
    back, none = K.logprob_map_rows(idx, want.to(cuda))  # positions -> compacted rows, 0 past the count
    assert none is None and torch.equal(back.cpu()[:n], src[:n]) and (back.cpu()[n:] == 0).all()
