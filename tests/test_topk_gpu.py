"""GPU: llx_topk_logprobs_rows (csrc/topk.hip) against its float64 restatement (tests/topk_cases.py) on the same bf16 logits, over the
case table: ids exact; with lse given logp is the fp32 difference bit for bit; with lse null logp is within 1e-5 of float64 (two fp32
summation orders over <= 128256 positive terms differ by about log2(V) * 2^-24 ~ 1e-6 relative in the sum, so by that much absolutely
in its logarithm; ten times that)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import topk_cases as C  # noqa: E402

NAN = float("nan")


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


@pytest.fixture(scope="module")
def batches():
    """(V, ld) -> (kinds, logits bf16 [R, ld] on the host): built once, never changed."""
    return {s: C.batch(*s) for s in C.SHAPES}


@pytest.mark.parametrize("k", C.KS)
@pytest.mark.parametrize("V,ld", C.SHAPES)
def test_topk_against_reference(K, cuda, batches, V, ld, k):
    kinds, lg = batches[(V, ld)]
    x = lg[:, :V].float()
    buf = lg.to(cuda)
    # lse given: ids exact, logp = bf16 value - lse in fp32, bit for bit
    lse = C.lse_of(x)
    want_ids, _ = C.top_logprobs_rows_ref(x, k, lse)
    ids, logp = K.topk_logprobs_rows(buf[:, :V], k, lse=lse.to(cuda))
    assert ids.dtype is torch.int32 and logp.dtype is torch.float32 and ids.shape == logp.shape == (len(kinds), k)
    bad = (ids.cpu() != want_ids).any(1).nonzero()[:, 0].tolist()
    assert not bad, f"rows {[kinds[r] for r in bad]}: ids {ids.cpu()[bad[0]].tolist()} want {want_ids[bad[0]].tolist()}"
    want_logp = x.gather(1, want_ids.long()) - lse[:, None]  # fp32
    assert C.same((ids.cpu(), logp.cpu()), (want_ids, want_logp)), (logp.cpu() - want_logp).abs().max()
    # lse null: the kernel's own lse, within 1e-5 of float64
    want_ids, want_logp = C.top_logprobs_rows_ref(x, k)
    ids0, logp0 = K.topk_logprobs_rows(buf[:, :V], k)
    assert torch.equal(ids0, ids)
    assert C.same((ids0.cpu(), logp0.cpu()), (want_ids, want_logp), atol=1e-5), (logp0.cpu().double() - want_logp).abs().nan_to_num(0, 0, 0).max()
    # ids[:, 0] is the top1 of llx_logprob_rows_fwd, on every row kind
    # ... and the kernel's own lse is the arithmetic of that kernel: labelled on the best token, its logp has the same bits (where it
    # is a number: rowlse.h turns a row with a whole chunk of -inf into NaN, this kernel does not)
    lp_fwd, _, top1 = K.logprob_rows_fwd(buf[:, :V], ids[:, 0].long(), want_top1=True)
    assert torch.equal(ids[:, 0], top1)
    num = ~torch.isnan(lp_fwd)
    assert num.any() and torch.equal(logp0[num, 0], lp_fwd[num])
    # a second launch is bit-identical (NaN payloads included: compare the bits), and the logits are only read
    ids2, logp2 = K.topk_logprobs_rows(buf[:, :V], k)
    assert torch.equal(ids2, ids0) and torch.equal(logp2.view(torch.int32), logp0.view(torch.int32))
    assert torch.equal(buf.view(torch.int16).cpu(), lg.view(torch.int16))


def test_scoring_mode_skips_ignored_rows(K, cuda):
    """labels -100 and rows at or past *rows rounded up to 256: -1 / 0.0, and their logits (NaN here) are never read; label_logp lands on
    the alternative that is the label and nowhere else."""
    R, V, k = 300, 1024, 5
    gen = torch.Generator().manual_seed(11)
    x = (torch.randn(R, V, generator=gen) * 2).to(torch.bfloat16)
    labels = torch.randint(0, V, (R,), generator=gen)
    labels[::4] = -100
    labels[1] = int(x[1].float().argmax())  # a label that is among the alternatives for sure
    live = labels != -100
    for rows in (None, 3):
        lim = R if rows is None else 256
        xin = x.clone()
        xin[~live] = NAN
        xin[lim:] = NAN
        lse = torch.logsumexp(x.double(), 1).float()
        marks = torch.arange(R, dtype=torch.float32) + 1000.0
        want_ids, _ = C.top_logprobs_rows_ref(x.float(), k, lse)
        want_logp = x.float().gather(1, want_ids.long()) - lse[:, None]
        keep = live.clone()
        keep[lim:] = False
        want_ids[~keep], want_logp[~keep] = -1, 0.0
        rows_t = None if rows is None else torch.tensor([rows], dtype=torch.int32, device=cuda)
        ids, logp = K.topk_logprobs_rows(xin.to(cuda), k, lse=lse.to(cuda), labels=labels.to(cuda), rows=rows_t)
        assert torch.equal(ids.cpu(), want_ids) and torch.equal(logp.cpu(), want_logp)
        ids2, logp2 = K.topk_logprobs_rows(xin.to(cuda), k, lse=lse.to(cuda), label_logp=marks.to(cuda), labels=labels.to(cuda), rows=rows_t)
        hit = (want_ids == labels[:, None].to(torch.int32)) & keep[:, None]
        assert hit[1].any() and torch.equal(ids2.cpu(), want_ids)
        assert torch.equal(logp2.cpu(), torch.where(hit, marks[:, None].expand(R, k), want_logp))
        # without lse the rows are skipped all the same
        ids3, logp3 = K.topk_logprobs_rows(xin.to(cuda), k, labels=labels.to(cuda), rows=rows_t)
        assert torch.equal(ids3.cpu(), want_ids) and (logp3.cpu()[~keep] == 0).all() and not torch.isnan(logp3).any()


def test_generation_mode_writes_one_column(K, cuda):
    """Row r writes [k] values at column pos[r] - hist_base only; a finished row and a column outside the buffer write nothing."""
    R, V, k, cap, base = 6, 1024, 3, 4, 10
    gen = torch.Generator().manual_seed(12)
    x = (torch.randn(R, V, generator=gen) * 2).to(torch.bfloat16)
    pos = torch.tensor([10, 13, 11, 14, 9, 12])  # columns 0, 3, 1, 4 (outside), -1 (outside), 2
    finished = torch.tensor([0, 0, 1, 0, 0, 0], dtype=torch.int32)
    want_ids, want_logp = C.top_logprobs_rows_ref(x.float(), k)
    for fin in (finished, None):
        ids = torch.full((R, cap, k), -7, dtype=torch.int32, device=cuda)
        logp = torch.full((R, cap, k), 123.5, dtype=torch.float32, device=cuda)
        pos_d = pos.to(cuda)
        fin_d = None if fin is None else fin.to(cuda)
        got = K.topk_logprobs_rows(x.to(cuda), k, pos=pos_d, hist_base=base, finished=fin_d, ids=ids, logp=logp)
        assert got[0].data_ptr() == ids.data_ptr() and got[1].data_ptr() == logp.data_ptr()
        assert torch.equal(pos_d.cpu(), pos) and (fin is None or torch.equal(fin_d.cpu(), fin))  # only read
        exp_ids = torch.full((R, cap, k), -7, dtype=torch.int32)
        exp_set = torch.zeros(R, cap, dtype=torch.bool)
        for r in range(R):
            h = int(pos[r]) - base
            if 0 <= h < cap and not (fin is not None and fin[r]):
                exp_ids[r, h] = want_ids[r]
                exp_set[r, h] = True
        assert exp_set.sum() == (3 if fin is not None else 4)
        assert torch.equal(ids.cpu(), exp_ids)
        lp = logp.cpu()
        assert (lp[~exp_set] == 123.5).all()
        for r, h in exp_set.nonzero().tolist():
            assert (lp[r, h].double() - want_logp[r]).abs().max() <= 1e-5


def test_wrapper_refuses_bad_arguments(K, cuda):
    from llx._lib import LlxError

    x = torch.zeros(2, 16, dtype=torch.bfloat16, device=cuda)
    for k in (0, 9, True, 2.0):
        with pytest.raises(LlxError, match="k must be an int in 1..8"):
            K.topk_logprobs_rows(x, k)
    with pytest.raises(LlxError, match="caller's ids / logp"):
        K.topk_logprobs_rows(x, 2, pos=torch.zeros(2, dtype=torch.int64, device=cuda))
    with pytest.raises(LlxError, match="lse must be"):
        K.topk_logprobs_rows(x, 2, lse=torch.zeros(3, device=cuda))


@pytest.mark.parametrize("T", [1, 300, 1025])
def test_topk_map_rows(K, cuda, T):
    """The [T, k] pair of the compacted rows back to the positions through inv: -1 / 0.0 at the ignored positions."""
    k = 5
    gen = torch.Generator().manual_seed(T)
    lb = torch.randint(0, 50, (T,), generator=gen)
    lb[torch.rand(T, generator=gen) < 0.4] = -100
    _, inv, _, cnt = K.head_compact_index(lb.to(cuda))
    n = int((lb != -100).sum())
    src_i = torch.randint(0, 1000, (T, k), generator=gen).to(torch.int32)
    src_f = torch.randn(T, k, generator=gen)
    want_i, want_f = torch.full((T, k), -1, dtype=torch.int32), torch.zeros(T, k)
    want_i[lb != -100], want_f[lb != -100] = src_i[:n], src_f[:n]
    got_i, got_f = K.topk_map_rows(inv, src_i.to(cuda), src_f.to(cuda))
    assert torch.equal(got_i.cpu(), want_i) and torch.equal(got_f.cpu(), want_f)
