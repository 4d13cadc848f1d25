"""Shared cases and the float64 restatement of the token log-probability kernels (csrc/logprob.hip), used by the CPU checks of the
restatement itself (tests/test_logprob_cases.py) and by the GPU parity tests (tests/test_logprob_gpu.py).

forward:  lse[t] = logsumexp(x[t]), logp[t] = x[t, label] - lse[t], top1[t] = lowest index of the row maximum;
          an ignored row (label -100) gives logp = lse = 0, top1 = -1; a label outside [0, V) counts its logit as 0 (as the loss kernel).
backward: dlogits[t, v] = g[t] * ((v == label) - exp(x[t, v] - lse[t])); zero rows where ignored.
"""
import numpy as np
import torch

# (T, V, ld, rows): where a 512-thread row kernel over 16-byte chunks can go wrong
SHAPES = [
    (1, 8, 8, None),         # one chunk, 511 idle threads
    (3, 1000, 1000, None),   # 125 chunks
    (5, 4104, 4112, None),   # 513 chunks: one thread takes two; the pad columns hold a sentinel that must not be read
    (300, 512, 512, None),   # more rows than kinds: every (kind, gradient) pair in one launch
    (300, 512, 512, 3),      # compacted-row limit 3 -> rows 256.. are neither read nor written
]
GRADS = (0.0, 1.0, -1.0 / 7.0, 1e3)  # upstream gradients of the backward
N_KINDS = 10
PAD_SENTINEL = 29952.0  # (on the bf16 grid) in the columns V..ld of the logits: larger than every logit, would become the maximum if read
OUT_SENTINEL = 12352.0  # (on the bf16 grid) prefilled into d logits where nothing may be written


def _bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16)


def _row(kind: int, V: int, gen: torch.Generator):
    """(logits fp32 [V] on the bf16 grid, label) of one row kind."""
    x = _bf(torch.randn(V, generator=gen) * 2.0).float()
    if kind == 0:
        return x, 0
    if kind == 1:
        return x, V - 1
    if kind == 2:
        return x, 7  # last element of the first 16-byte chunk
    if kind == 3:
        return x, min(8, V - 1)  # first element of the second chunk
    if kind == 4:
        return x, -100
    if kind == 5:  # all equal: logp = -log V, top1 = 0
        return torch.full((V,), 1.5), V // 2
    if kind == 6:  # two equal maxima: top1 is the lower index
        lo, hi = V // 3, V - 2
        x[lo] = x[hi] = 16.0
        return x, hi
    if kind in (7, 8):  # one logit 80 above the rest, labelled on it (logp ~ 0) and off it (logp ~ -80)
        x = _bf(x.clamp(-4, 4) * 0.25).float()
        p = (2 * V) // 3
        x[p] = 81.0
        return x, (p if kind == 7 else 1)
    if kind == 9:  # all logits near -3e4 (bf16 spacing 128 there)
        return _bf(-3.0e4 + 300.0 * torch.randn(V, generator=gen)).float(), V // 2
    raise ValueError(kind)


def batches(T: int, V: int, ld: int):
    """Batches (logits bf16 [T, ld], labels int64 [T]) that together hold every row kind: row t of batch b is kind (b * T + t) % 10."""
    gen = torch.Generator().manual_seed(1000 * T + V)
    out = []
    for b in range((N_KINDS + T - 1) // T if T < N_KINDS else 1):
        lg = torch.full((T, ld), PAD_SENTINEL)
        lb = torch.empty(T, dtype=torch.int64)
        for t in range(T):
            x, lab = _row((b * T + t) % N_KINDS, V, gen)
            lg[t, :V] = x
            lb[t] = lab
        out.append((_bf(lg), lb))
    return out


def grads(T: int, rot: int) -> torch.Tensor:
    """Upstream gradient of row t: GRADS[(t + rot) % 4] - over rot = 0..3 every row kind meets every gradient."""
    return torch.tensor([GRADS[(t + rot) % 4] for t in range(T)], dtype=torch.float32)


def ref_fwd(logits: torch.Tensor, labels: torch.Tensor, rows=None):
    """float64 restatement of the forward kernel on logits [T, V] (any float dtype): (logp, lse, top1)."""
    x = logits.double()
    T, V = x.shape
    lse = torch.logsumexp(x, dim=1)
    inside = (labels >= 0) & (labels < V)
    xl = torch.where(inside, x.gather(1, labels.clamp(0, V - 1)[:, None])[:, 0], torch.zeros((), dtype=torch.float64))
    top1 = torch.from_numpy(np.argmax(x.numpy(), axis=1).astype(np.int32))  # numpy: the first occurrence of the maximum
    ignored = labels == -100
    logp = torch.where(ignored, torch.zeros((), dtype=torch.float64), xl - lse)
    lse = torch.where(ignored, torch.zeros((), dtype=torch.float64), lse)
    top1 = torch.where(ignored, torch.full((), -1, dtype=torch.int32), top1)
    if rows is not None:
        lim = (rows + 255) // 256 * 256
        logp[lim:], lse[lim:], top1[lim:] = 0, 0, 0
    return logp, lse, top1


def ref_bwd(logits: torch.Tensor, labels: torch.Tensor, g: torch.Tensor):
    """float64 restatement of the backward kernel: g[t] * (onehot(label) - softmax(x[t])), zero rows where the label is -100."""
    x = logits.double()
    T, V = x.shape
    lse = torch.logsumexp(x, dim=1, keepdim=True)
    onehot = (torch.arange(V)[None, :] == labels[:, None]).double()
    d = g.double()[:, None] * (onehot - torch.exp(x - lse))
    return torch.where((labels == -100)[:, None], torch.zeros((), dtype=torch.float64), d)
