"""CPU: the float64 restatement of the top-k log-probability kernel (tests/topk_cases.py) against torch.topk where no two values tie and
against hand-written rows where they do; the case table holds the kernel's dispatch corners, and every injected fault is caught."""
import math

import pytest
import torch

from tests import topk_cases as C

NINF = float("-inf")


@pytest.mark.parametrize("V", [8, 1000, 4104])
@pytest.mark.parametrize("k", C.KS)
def test_ref_matches_torch_topk_without_ties(V, k):
    gen = torch.Generator().manual_seed(V + k)
    x = torch.randperm(V, generator=gen).double() * 0.37 - 11.0  # all distinct
    ids, logp = C.top_logprobs_ref(x, k)
    want = torch.topk(torch.log_softmax(x, 0), k)
    assert ids.dtype is torch.int32 and torch.equal(ids.long(), want.indices)
    torch.testing.assert_close(logp, want.values, atol=1e-12, rtol=0)
    ids2, logp2 = C.top_logprobs_ref(x, k, lse=2.5)
    assert torch.equal(ids2, ids) and torch.equal(logp2, x[ids.long()] - 2.5)


def test_ref_hand_written_ties():
    ids, logp = C.top_logprobs_ref(torch.full((16,), 1.5), 8)  # all equal: the first eight, each -log V
    assert ids.tolist() == list(range(8))
    torch.testing.assert_close(logp, torch.full((8,), -math.log(16), dtype=torch.float64), atol=1e-12, rtol=0)
    x = torch.tensor([0.0, 3.0, 1.0, 3.0, 2.0, 1.0, -1.0, 2.0])  # two equal maxima: the lower index first, and so down the row
    assert C.top_logprobs_ref(x, 5)[0].tolist() == [1, 3, 4, 7, 2]
    assert C.top_logprobs_ref(x, 8)[0].tolist() == [1, 3, 4, 7, 2, 5, 0, 6]
    x = torch.tensor([NINF, 2.0, NINF, 5.0, NINF, NINF, 2.0, NINF])  # -inf last, among themselves by index
    ids, logp = C.top_logprobs_ref(x, 8)
    assert ids.tolist() == [3, 1, 6, 0, 2, 4, 5, 7]
    assert torch.isfinite(logp[:3]).all() and (logp[3:] == NINF).all()
    x = torch.tensor([NINF, NINF, -4.0, NINF, NINF, NINF, NINF, NINF])  # fewer than k finite entries
    ids, logp = C.top_logprobs_ref(x, 5)
    assert ids.tolist() == [2, 0, 1, 3, 4] and logp[0] == 0.0 and (logp[1:] == NINF).all()
    x = torch.tensor([float("nan"), -2.0, NINF, float("nan"), 0.0, -0.0, NINF, 1.0])  # a NaN ranks as -inf; -0.0 == +0.0
    ids, logp = C.top_logprobs_ref(x, 8, lse=0.0)
    assert ids.tolist() == [7, 4, 5, 1, 0, 2, 3, 6]
    assert torch.isnan(logp[4]) and logp[5] == NINF and torch.isnan(logp[6])


def test_case_table_holds_the_dispatch_corners():
    assert C.VS == (8, 8 * C.THREADS + 8, 1024, 128256) and C.KS == (1, 5, 8) and C.TOPK_MAX == 8
    assert any(ld > V for V, ld in C.SHAPES) and {V for V, _ in C.SHAPES} == set(C.VS)
    kinds, lg = C.batch(4104)
    assert {"one_thread", "per_wave", "dup_straddle", "wave_second", "max_last", "all_equal", "some_ninf", "few_finite", "nan_zero"} <= set(kinds)
    thread = lambda i: (i // 8) % C.THREADS  # noqa: E731
    top = lambda kind, k: C.top_logprobs_ref(lg[kinds.index(kind)], k)[0].tolist()  # noqa: E731
    assert {thread(i) for i in top("one_thread", 8)} == {0} and {i // 8 for i in top("one_thread", 8)} == {0, C.THREADS}  # two chunks of one thread
    assert sorted(thread(i) // C.WAVE for i in top("per_wave", 8)) == list(range(8))  # one per wave
    assert top("dup_straddle", 8)[:6] == [6, 7, 8, 9, 510, 511] and lg[kinds.index("dup_straddle")][[7, 8, 511, 512]].unique().numel() == 1
    assert top("max_last", 5)[:2] == [4103, 4096]
    a, b = top("wave_second", 5)[:2]
    assert thread(a) // C.WAVE == thread(b) // C.WAVE == 1 and thread(a) != thread(b)
    kinds, lg = C.batch(128256)
    assert lg.shape == (1, 128256) and C.top_logprobs_ref(lg[0], 1)[0].item() >= 128256 - 8  # the maximum in the last chunk
    vals = lg[0].float()[C.top_logprobs_ref(lg[0], 8)[0].long()]
    assert vals.unique().numel() < 8  # bf16 at this V ties inside the top eight
    _, lg = C.batch(1024, 1088)
    assert lg.shape[1] == 1088 and (lg[:, 1024:].float() == C.PAD_SENTINEL).all()


@pytest.mark.parametrize("fault", sorted(C.FAULTS))
def test_every_injected_fault_is_caught(fault):
    caught = []
    for V, ld in C.SHAPES:
        kinds, lg = C.batch(V, ld)
        x = lg[:, :V].float()
        for with_lse in (False, True):
            lse = C.lse_of(x) if with_lse else None
            for k in C.KS:
                want = C.top_logprobs_rows_ref(x, k, lse)
                if not C.same(C.FAULTS[fault](x, k, lse), want, atol=1e-9):
                    caught.append((V, ld, k, with_lse))
    assert caught, f"no case catches the fault {fault}"
