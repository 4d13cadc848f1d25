"""GPU: the loss row kernel (csrc/ce.hip) and the log-probability row kernel (csrc/logprob.hip) take their log-sum-exp from ONE online
(max, sum-exp) pass (csrc/rowlse.h), so on a single labelled row the loss is the forward kernel's lse minus the label's logit, bit for
bit: the count is 1, 1 / count is 1, the reduce adds a single term, both kernels form gm + __logf(s), and the library is built with
-ffp-contract=off.  Shapes (V, ld): (8, 8) one chunk and 511 idle threads, (1000, 1000) partial waves, (4096, 4096) exactly one chunk
per thread, (4104, 4112) one thread takes two chunks and the row has pad columns."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8), (1000, 1000), (4096, 4096), (4104, 4112)]


@pytest.mark.parametrize("kind", ["random", "equal"])
@pytest.mark.parametrize("V,ld", SHAPES)
def test_loss_is_lse_minus_label_logit(cuda, V, ld, kind):
    from llx import kernels as K

    gen = torch.Generator().manual_seed(V)
    if kind == "random":
        row = (torch.randn(1, ld, generator=gen) * 3).bfloat16()
    else:
        row = torch.full((1, ld), 1.375, dtype=torch.bfloat16)
    row[:, V:] = 3.0e4  # pad columns: read by neither kernel
    label = torch.randint(0, V, (1,), generator=gen)
    buf = row.to(cuda)
    _, lse, _ = K.logprob_rows_fwd(buf[:, :V], label.to(cuda))
    loss, none = K.ce_fwd_bwd(buf[:, :V], label.to(cuda), write_grad=False)
    assert none is None and torch.equal(buf.cpu(), row)
    want = lse.cpu()[0] - row[0, label[0]].float()  # fp32 on the host
    assert want.dtype is torch.float32 and torch.isfinite(want)
    print(f"V {V} ld {ld} {kind}: loss {loss.item()!r} lse - x[label] {want.item()!r}")
    assert torch.equal(loss.cpu(), want)
