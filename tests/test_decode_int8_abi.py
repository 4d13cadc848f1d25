"""CPU: the int8 weight-streaming GEMV entry point (csrc/decode.hip: llx_gemv_i8) is exported, declared in include/llx.h and bound in
llx/_lib.py, and validates its arguments before any launch (an error code and a message naming the cause; no GPU needed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call(lib, *, K=1024, M=1, scale0=16, dynamic=0, n0=64):
    P = ctypes.c_void_p
    return lib.llx_gemv_i8(P(16), K, n0, None, 0, 0, None, 0, 0, P(16), K, M, K, None, 0.0, 0, P(16), n0, None, 0, None, 0, 0, None, None, 0, 0, None,
                           None, None, None, 0, 0, 0, None, 0, 0.0, P(scale0) if scale0 else None, None, None, dynamic, None)


def test_gemv_i8_is_exported_declared_and_bound():
    from llx import _lib as L

    lib = L.load()
    assert hasattr(lib, "llx_gemv_i8")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llx.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+llx_gemv_i8\s*\(", text), "llx_gemv_i8 is not declared in include/llx.h"
    assert "llx_gemv_i8" in L.SIGNATURES
    # llx_gemv_bf16's argument list + three scale pointers + the dynamic flag, stream last
    base, i8 = L.SIGNATURES["llx_gemv_bf16"][1], L.SIGNATURES["llx_gemv_i8"][1]
    assert i8 == base[:-1] + [ctypes.c_void_p] * 3 + [ctypes.c_int] + base[-1:]
    assert lib.llx_version() == 105


def test_gemv_i8_rejects_before_launch():
    from llx import _lib as L

    lib = L.load()
    for dynamic in (0, 1):
        rc = _call(lib, K=1032, dynamic=dynamic)  # a lane's 16-byte load is 16 int8 elements
        assert rc == -1 and b"K=1032" in lib.llx_last_error_string() and b"multiple of 16" in lib.llx_last_error_string()
        rc = _call(lib, M=5, dynamic=dynamic)
        assert rc == -1 and b"M=5" in lib.llx_last_error_string()
        rc = _call(lib, scale0=0, dynamic=dynamic)
        assert rc == -1 and b"null scale" in lib.llx_last_error_string()
        assert lib.llx_last_error_string().startswith(b"llx_gemv_i8:")
    # the bf16 entry point keeps its own name in its messages
    P = ctypes.c_void_p
    rc = lib.llx_gemv_bf16(P(16), 1032, 64, None, 0, 0, None, 0, 0, P(16), 1032, 5, 1032, None, 0.0, 0, P(16), 64, None, 0, None, 0, 0, None, None, 0, 0,
                           None, None, None, None, 0, 0, 0, None, 0, 0.0, None)
    assert rc == -1 and lib.llx_last_error_string().startswith(b"llx_gemv_bf16: M=5")
