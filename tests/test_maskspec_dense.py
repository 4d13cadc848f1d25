"""CPU: MaskSpec(dense=...) - the constructor's shape / dtype rules - and MaskSpec.from_mask_mod, which stands where the reference
calls create_block_mask(mask_mod, ...) (train_metamathqa.py:67-70): a mask the rule reproduces comes back as the rule spec (the
faster kernels), anything else as a dense spec holding exactly the grid evaluation of the mask_mod.  Host logic only."""
import pytest
import torch

from llx._lib import LlxError
from llx.kernels import MaskSpec

S = 96


def _band(S, w):
    i = torch.arange(S)
    return (i[:, None] - i[None, :]).abs() <= w


@pytest.mark.parametrize("shape", [(S, S), (1, S, S), (3, S, S), (1, 1, S, S), (3, 1, S, S)])
def test_constructor_accepts_the_three_shapes(shape):
    m = _band(S, 10).expand(shape).clone()
    spec = MaskSpec(dense=m)
    assert spec.dense is m and spec.doc_ids is None and spec.prefix_len is None


def test_rule_spec_has_no_dense_mask():
    assert MaskSpec().dense is None
    assert MaskSpec(doc_ids=torch.zeros(S, dtype=torch.int32)).dense is None


@pytest.mark.parametrize("bad,why", [
    (lambda: MaskSpec(dense=_band(S, 10)[None, None].expand(2, 4, S, S)), "per-head"),
    (lambda: MaskSpec(dense=_band(S, 10).float()), "bool"),
    (lambda: MaskSpec(dense=_band(S, 10).to(torch.uint8)), "bool"),
    (lambda: MaskSpec(dense=_band(S, 10)[:, : S - 1]), "[S, S]"),
    (lambda: MaskSpec(dense=_band(S, 10)[None, : S - 8]), "[S, S]"),
    (lambda: MaskSpec(dense=_band(S, 10)[0]), "[S, S]"),
    (lambda: MaskSpec(doc_ids=torch.zeros(S, dtype=torch.int32), dense=_band(S, 10)), "doc_ids"),
    (lambda: MaskSpec(prefix_len=torch.tensor([3]), dense=_band(S, 10)), "prefix_len"),
])
def test_constructor_rejects(bad, why):
    with pytest.raises(LlxError, match=why.replace("[", r"\[")):
        bad()


def test_from_mask_mod_causal_is_the_plain_rule():
    spec = MaskSpec.from_mask_mod(lambda b, h, q_idx, kv_idx: q_idx >= kv_idx, 2, S, "cpu")
    assert spec.dense is None and spec.doc_ids is None and spec.prefix_len is None


def test_from_mask_mod_document_mask_is_the_document_rule():
    document_id = torch.zeros(S, dtype=torch.int64)  # packed documents of uneven length (train_metamathqa.py:51-66)
    for c in (13, 40, 77):
        document_id[c:] += 1

    def mask_mod(b, h, q_idx, kv_idx):  # train_metamathqa.py:67-68
        return (q_idx >= kv_idx) & (document_id[q_idx] == document_id[kv_idx])

    spec = MaskSpec.from_mask_mod(mask_mod, 1, S, "cpu")
    assert spec.dense is None and spec.prefix_len is None
    d = spec.doc_ids.view(-1, S)[0]
    assert torch.equal(d[:, None] == d[None, :], document_id[:, None] == document_id[None, :])


def test_from_mask_mod_sliding_window_is_dense_and_equals_the_grid():
    W = 17

    def mask_mod(b, h, q_idx, kv_idx):
        return (q_idx >= kv_idx) & (q_idx - kv_idx < W)

    B = 2
    spec = MaskSpec.from_mask_mod(mask_mod, B, S, "cpu")
    assert spec.dense is not None and spec.doc_ids is None and spec.prefix_len is None
    i = torch.arange(S)
    want = (i[:, None] >= i[None, :]) & (i[:, None] - i[None, :] < W)
    assert spec.dense.dtype is torch.bool and spec.dense.shape[-2:] == (S, S)
    assert torch.equal(spec.dense.expand(B, S, S) if spec.dense.dim() == 3 else spec.dense[:, 0].expand(B, S, S), want.expand(B, S, S))


def test_from_mask_mod_per_sample_mask_keeps_the_batch():
    width = torch.tensor([5, 23])  # a sliding window whose width differs per sample

    def mask_mod(b, h, q_idx, kv_idx):
        return (q_idx >= kv_idx) & (q_idx - kv_idx < width[b])

    spec = MaskSpec.from_mask_mod(mask_mod, 2, S, "cpu")
    assert spec.dense is not None and spec.dense.shape[0] == 2
    m = spec.dense.reshape(2, S, S)
    assert bool(m[0, 50, 46]) and not bool(m[0, 50, 45]) and bool(m[1, 50, 28]) and not bool(m[1, 50, 27])


def test_from_mask_mod_left_padding_with_diagonal_is_a_document_rule():
    """Causal with padding keys masked and the diagonal kept: every padding position is a document of its own - the rule spec."""
    pad = torch.tensor([0, 9])

    def mask_mod(b, h, q_idx, kv_idx):
        return ((q_idx >= kv_idx) & (kv_idx >= pad[b])) | (q_idx == kv_idx)

    spec = MaskSpec.from_mask_mod(mask_mod, 2, S, "cpu")
    assert spec.dense is None and spec.doc_ids is not None and spec.doc_ids.shape == (2, S)


def test_from_mask_mod_rejects_a_non_bool_mask_mod():
    with pytest.raises(LlxError, match="bool"):
        MaskSpec.from_mask_mod(lambda b, h, q_idx, kv_idx: (q_idx >= kv_idx).float(), 1, S, "cpu")


def test_device_prefetcher_moves_a_dense_spec_as_a_dense_spec(monkeypatch):
    """DevicePrefetcher._to_device rebuilds a MaskSpec on the device: a dense spec must come out dense, not as the empty (causal) rule."""
    from llx.data import DevicePrefetcher

    monkeypatch.setattr(torch.Tensor, "is_pinned", lambda self, *a, **k: True)  # no pinned memory without a GPU
    pre = object.__new__(DevicePrefetcher)
    pre.device = torch.device("cpu")
    moved = pre._to_device(MaskSpec(dense=_band(S, 10)))
    assert moved.dense is not None and torch.equal(moved.dense, _band(S, 10)) and moved.doc_ids is None and moved.prefix_len is None
    rule = pre._to_device(MaskSpec(doc_ids=torch.zeros(S, dtype=torch.int64)))
    assert rule.dense is None and rule.doc_ids.dtype is torch.int32
