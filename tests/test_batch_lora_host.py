"""CPU: LoRA / DoRA linears on the batched decode stream.  Which fused groups llx/decode.py::_batch_group sends to it (modules built
with apply_linear_adapter_ on the host), and that the two adapter entry points of csrc/decode_rows.hip (llx_gemm_rows16_bf16_lora,
llx_gemm_rows16_i8_lora) reject bad arguments before any launch, with a message that begins with their name.  The workspace functions
keep the values tests/test_batch_host.py and tests/test_batch_int8_host.py hold: the adapter term adds nothing to the workspace."""
import ctypes
import re
from pathlib import Path

import torch
from torch import nn

P16 = ctypes.c_void_p(16)
BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------- _batch_group
def _lin(kind=None, rank=16, alpha=None, n=32, k=64, int8=None):
    """nn.Linear(k, n) in bf16 on the host: int8 = None | "dynamic" | "weight-only" (quantised first, as the training script does),
    kind = None | "lora" | "dora" with scale alpha / rank (default 2)."""
    from modelling import apply_linear_adapter_
    from subclasses import quantize_linear_

    torch.manual_seed(0)
    m = nn.Linear(k, n, bias=False).bfloat16()
    if int8:
        quantize_linear_(m, "int8", dynamic_int8_act=int8 == "dynamic")
    if kind:
        apply_linear_adapter_(m, kind, rank=rank, alpha=float(alpha if alpha is not None else 2 * rank))
    return m


def test_batch_group_takes_adapters_of_the_stream_ranks():
    import llx.decode as D

    for r in (16, 32, 48, 64):
        assert D._batch_group((_lin("lora", r),)), f"LoRA r={r} on bf16"
        assert D._batch_group((_lin("lora", r), _lin("lora", r))), f"LoRA r={r} pair on bf16"
    assert D._batch_group((_lin("dora", 16),)) and D._batch_group((_lin("dora", 16), _lin("dora", 16)))
    assert D._batch_group((_lin("lora", 16, int8="dynamic"),)) and D._batch_group((_lin("lora", 16, int8="dynamic"), _lin("lora", 16, int8="dynamic")))
    assert D._batch_group((_lin("lora", 16), _lin("lora", 32), _lin("lora", 16))), "q|k|v with ranks (16, 32, 16)"
    # and the groups the stream took before
    assert D._batch_group((_lin(),)) and D._batch_group((_lin(int8="dynamic"), _lin(int8="dynamic")))


def test_batch_group_leaves_the_rest_on_the_generic_path():
    import llx.decode as D

    for r in (8, 24, 80):
        assert D._plain(_lin("lora", r)) == D.KIND_BF16, "batch 1 streams this rank"
        assert not D._batch_group((_lin("lora", r),)), f"LoRA r={r}"
        assert not D._batch_group((_lin("lora", 16), _lin("lora", r))), f"LoRA r=(16, {r})"
    assert not D._batch_group((_lin("lora", 16), _lin(), _lin("lora", 16))), "a group with one plain member"
    assert not D._batch_group((_lin(), _lin("lora", 16))), "a group with one plain member"
    assert not D._batch_group((_lin("lora", 16), _lin("dora", 16))), "LoRA + DoRA"
    assert not D._batch_group((_lin("lora", 16, alpha=32), _lin("lora", 16, alpha=16))), "two scales"
    assert not D._batch_group((_lin("lora", 16, int8="weight-only"),)), "weight-only int8 + LoRA"
    assert not D._batch_group((_lin("lora", 16, int8="dynamic"), _lin("lora", 16))), "two weight kinds"
    m = _lin("lora", 16, int8="dynamic")
    m.m = nn.Parameter(torch.ones(m.out_features, dtype=BF))  # (DoRALinear cannot take the row norms of an int8 weight itself)
    assert D._dora(m) and not D._batch_group((m,)), "DoRA on int8"


# ------------------------------------------------------------------------------------------------- the entry points
def _common(M, K, n0, ws, wsb):
    # w0 .. pos (llx_gemm_rows16_bf16's arguments up to workspace_bytes): one weight [n0, K], epilogue 0
    return [P16, K, n0, None, 0, 0, None, 0, 0, P16, K, M, K, None, 0.0, 0, P16, n0, None, 0, None, 0, 0, None, None, 0, 0, 128, 16, None, ws, wsb]


def _bf16_lora(lib, *, M=2, K=64, n0=64, rank=16, t=P16, ldt=None, bext=P16, cs=(None, None, None), ws=None, wsb=0, w1=False, bext1=None, rank1=0):
    a = _common(M, K, n0, ws, wsb)
    if w1:
        a[3:6] = [P16, K, n0]
    return lib.llx_gemm_rows16_bf16_lora(*a, bext, bext1, None, rank, rank1, 0, t, rank + rank1 if ldt is None else ldt, 2.0, *cs, None)


def _i8_lora(lib, *, M=2, K=64, n0=64, rank=16, t=P16, bext=P16, scale=P16, ws=None, wsb=0):
    return lib.llx_gemm_rows16_i8_lora(*_common(M, K, n0, ws, wsb), scale, None, None, bext, None, None, rank, 0, 0, t, rank, 2.0, None)


def test_adapter_entry_points_are_exported_declared_and_bound():
    from llx import _lib as L

    lib = L.load()
    text = (Path(__file__).resolve().parents[1] / "include" / "llx.h").read_text()
    for fn in ("llx_gemm_rows16_bf16_lora", "llx_gemm_rows16_i8_lora"):
        assert hasattr(lib, fn) and re.search(rf"\bint\s+{fn}\s*\(", text), fn
    p, i, f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    adapters = [p, p, p, i, i, i, p, i, f]  # bext0..2, rank0..2, t, ldt, lora_scale
    base = L.SIGNATURES["llx_gemm_rows16_bf16"][1]
    assert L.SIGNATURES["llx_gemm_rows16_bf16_lora"][1] == base[:-1] + adapters + [p, p, p] + base[-1:]
    base8 = L.SIGNATURES["llx_gemm_rows16_i8"][1]
    assert L.SIGNATURES["llx_gemm_rows16_i8_lora"][1] == base8[:-1] + adapters + base8[-1:]
    assert lib.llx_version() == 105


def test_adapter_entry_points_reject_bad_arguments():
    from llx import _lib as L

    lib = L.load()
    for name, call in (("llx_gemm_rows16_bf16_lora", _bf16_lora), ("llx_gemm_rows16_i8_lora", _i8_lora)):
        def rejected(what, **kw):
            assert call(lib, **kw) == -1, (name, what)
            msg = lib.llx_last_error_string()
            assert msg.startswith(name.encode() + b":"), (name, what, msg)
            return msg

        for r in (8, 24, 80, 0):
            assert b"multiple of 16, at most 64" in rejected(f"rank {r}", rank=r)
        assert b"t missing" in rejected("null t", t=None)
        assert b"B factor" in rejected("a weight without its factor", bext=None)
        for M in (1, 17):
            assert b"outside 2..16" in rejected(f"M={M}", M=M)
        # a split K with no workspace (K = 4096 with 4 tiles is cut into slices), and with one that is too small
        assert b"workspace" in rejected("missing workspace", K=4096)
        assert b"workspace" in rejected("small workspace", K=4096, ws=P16, wsb=1024)
    # bf16 only: a factor without its weight, a row stride of t below the sum of the ranks, DoRA factors for one of two segments
    assert _bf16_lora(lib, bext1=P16, rank1=16) == -1 and b"B factor" in lib.llx_last_error_string()
    assert _bf16_lora(lib, ldt=8) == -1 and b"t missing" in lib.llx_last_error_string()
    assert _bf16_lora(lib, w1=True, bext1=P16, rank1=16, cs=(P16, None, None)) == -1
    msg = lib.llx_last_error_string()
    assert msg.startswith(b"llx_gemm_rows16_bf16_lora:") and b"DoRA" in msg
    assert _bf16_lora(lib, w1=True, bext1=P16, rank1=16, cs=(None, P16, None)) == -1 and b"DoRA" in lib.llx_last_error_string()
    # int8 only: the per-row scales are still required
    assert _i8_lora(lib, scale=None) == -1 and b"null scale" in lib.llx_last_error_string()
    # the un-adapted entry points keep their messages (tests/test_batch_host.py, tests/test_batch_int8_host.py)
    assert lib.llx_gemm_rows16_bf16(*_common(2, 4096, 64, None, 0), None) == -1
    assert lib.llx_last_error_string().startswith(b"llx_gemm_rows16_bf16: workspace")


def test_workspace_functions_keep_their_values():
    from llx import _lib as L

    lib = L.load()
    wsb, wsb8 = lib.llx_gemm_rows16_workspace_bytes, lib.llx_gemm_rows16_i8_workspace_bytes
    assert wsb(16, 64, 4096, 0) == 4 * 16 * 1024 and wsb(2, 64, 256, 0) == 0
    assert wsb8(2, 64, 512, 0) == 0
    assert wsb8(16, 64, 4096, 0) == 64 + 4 * 8 * 1024
    assert wsb8(16, 4096, 14336, 0) == 64 + 256 * 14 * 1024
    assert wsb8(5, 36, 1040, 0) == 64 + 3 * 3 * 1024
    assert wsb8(2, 2 * 1792, 1024, 3) == 64 + 224 * 2 * 1024
    # the t product of a rank-16 group at K = 4096: one tile, 16 slices of one 256-element batch
    assert wsb(16, 16, 4096, 0) == 16 * 1024
