"""CPU: the MXFP4 entry points (csrc/mxfp4.hip: llx_quantize_mxfp4, llx_dequantize_mxfp4, llx_gemv_mxfp4) are exported, declared in
include/llx.h and bound in llx/_lib.py, and validate their arguments before any launch (an error code and a message naming the cause;
no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
NAMES = ("llx_quantize_mxfp4", "llx_dequantize_mxfp4", "llx_gemv_mxfp4")


@pytest.fixture(scope="module")
def lib():
    from llx import _lib as L

    return L.load()


def _err(lib, rc, *needles):
    msg = lib.llx_last_error_string() or b""
    assert rc == -1, (rc, msg)
    for n in needles:
        assert n in msg, (n, msg)


def _gemv(lib, *, K=2048, M=1, n0=64, w0=16, x=16, out=16, ldw0=None, ldx=None, scale0=16, lds0=None, epilogue=0, rope=None, kc=None, vc=None, pos=None,
          n1=0, w1=None, scale1=None, norm_w=None):
    ldw0 = K // 2 if ldw0 is None else ldw0
    lds0 = K // 32 if lds0 is None else lds0
    ldx = K if ldx is None else ldx
    return lib.llx_gemv_mxfp4(P(w0) if w0 else None, ldw0, n0, P(w1) if w1 else None, ldw0, n1, None, 0, 0, P(x) if x else None, ldx, M, K,
                              P(norm_w) if norm_w else None, 0.0, epilogue, P(out) if out else None, n0, None, 0, P(rope) if rope else None, 128, 128,
                              P(kc) if kc else None, P(vc) if vc else None, 1024, 128, P(pos) if pos else None, None, None, None, 0, 0, 0, None, 0, 0.0,
                              P(scale0) if scale0 else None, lds0, P(scale1) if scale1 else None, lds0, None, 0, None)


def test_entry_points_are_exported_declared_and_bound(lib):
    from llx import _lib as L

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llx.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name) and name in L.SIGNATURES
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in include/llx.h"
    # llx_gemv_bf16's argument list + three (scale pointer, row stride) pairs, stream last
    base, mx = L.SIGNATURES["llx_gemv_bf16"][1], L.SIGNATURES["llx_gemv_mxfp4"][1]
    assert mx == base[:-1] + [ctypes.c_void_p, ctypes.c_int64] * 3 + base[-1:]
    assert lib.llx_version() == 105


def test_quantize_rejects_before_launch(lib):
    q = lib.llx_quantize_mxfp4
    _err(lib, q(None, 64, 0, 4, 64, P(16), P(16), None), b"llx_quantize_mxfp4: null pointer")
    _err(lib, q(P(16), 64, 0, 4, 64, None, P(16), None), b"null pointer")
    _err(lib, q(P(16), 64, 0, 4, 64, P(16), None, None), b"null pointer")
    _err(lib, q(P(16), 48, 0, 4, 48, P(16), P(16), None), b"K=48", b"multiple of 32")
    _err(lib, q(P(16), 32, 0, 4, 64, P(16), P(16), None), b"row stride 32")            # shorter than K
    _err(lib, q(P(16), 68, 0, 4, 64, P(16), P(16), None), b"row stride 68")            # bf16 rows off 16 bytes
    _err(lib, q(P(16), 66, 1, 4, 64, P(16), P(16), None), b"row stride 66")            # fp32 rows off 16 bytes
    _err(lib, q(P(8), 64, 0, 4, 64, P(16), P(16), None), b"16-byte aligned")
    _err(lib, q(P(16), 64, 0, 4, 64, P(24), P(16), None), b"16-byte aligned")
    _err(lib, q(P(16), 64, 0, 0, 64, P(16), P(16), None), b"llx_quantize_mxfp4:")


def test_dequantize_rejects_before_launch(lib):
    dq = lib.llx_dequantize_mxfp4
    _err(lib, dq(None, 32, P(16), 2, 4, 64, P(16), 64, 0, None), b"llx_dequantize_mxfp4: null pointer")
    _err(lib, dq(P(16), 32, None, 2, 4, 64, P(16), 64, 0, None), b"null pointer")
    _err(lib, dq(P(16), 32, P(16), 2, 4, 64, None, 64, 0, None), b"null pointer")
    _err(lib, dq(P(16), 24, P(16), 1, 4, 48, P(16), 48, 0, None), b"K=48", b"multiple of 32")
    _err(lib, dq(P(16), 16, P(16), 2, 4, 64, P(16), 64, 0, None), b"row stride")       # packed rows shorter than K / 2
    _err(lib, dq(P(16), 40, P(16), 2, 4, 64, P(16), 64, 0, None), b"row stride")       # packed rows off 16 bytes
    _err(lib, dq(P(16), 32, P(16), 1, 4, 64, P(16), 64, 0, None), b"row stride")       # scale rows shorter than K / 32
    _err(lib, dq(P(16), 32, P(16), 2, 4, 64, P(16), 32, 0, None), b"output row stride 32")
    _err(lib, dq(P(16), 32, P(16), 2, 4, 64, P(16), 3, 1, None), b"output row stride 3")  # transposed: rows of N
    _err(lib, dq(P(8), 32, P(16), 2, 4, 64, P(16), 64, 0, None), b"16-byte aligned")
    _err(lib, dq(P(16), 32, P(16), 2, 4, 64, P(8), 64, 0, None), b"16-byte aligned")


def test_gemv_rejects_before_launch(lib):
    for kw in (dict(w0=0), dict(x=0), dict(out=0)):
        _err(lib, _gemv(lib, **kw), b"llx_gemv_mxfp4: null pointer")
    _err(lib, _gemv(lib, scale0=0), b"llx_gemv_mxfp4: null scale")
    _err(lib, _gemv(lib, n1=64, w1=16), b"null scale")                                 # a second weight without its scales
    _err(lib, _gemv(lib, w0=8), b"16-byte aligned")
    _err(lib, _gemv(lib, x=24), b"16-byte aligned")
    _err(lib, _gemv(lib, norm_w=4), b"16-byte aligned")
    _err(lib, _gemv(lib, K=2064), b"K=2064", b"multiple of 32")
    _err(lib, _gemv(lib, K=16), b"K=16", b"multiple of 32")
    for M in (0, 5):
        _err(lib, _gemv(lib, M=M), b"M=%d" % M, b"1..4")
    _err(lib, _gemv(lib, ldw0=1008), b"packed row stride")                             # shorter than K / 2
    _err(lib, _gemv(lib, ldw0=1032), b"multiples of 16 bytes")
    _err(lib, _gemv(lib, lds0=63), b"scale row stride")
    _err(lib, _gemv(lib, M=2, ldx=1024), b"activation row stride")
    _err(lib, _gemv(lib, ldx=2052), b"multiples of 16 bytes")
    _err(lib, _gemv(lib, K=30752), b"K too large for the LDS stage")
    # q|k|v without the caches, the table or the positions
    full = dict(epilogue=2, n0=384, rope=16, kc=16, vc=16, pos=16)
    for missing in ("rope", "kc", "vc", "pos"):
        _err(lib, _gemv(lib, **{**full, missing: None}), b"llx_gemv_mxfp4: bad q|k|v epilogue arguments")
    assert (lib.llx_last_error_string() or b"").startswith(b"llx_gemv_mxfp4:")
