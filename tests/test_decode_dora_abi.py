"""CPU: the DoRA weight-streaming GEMV entry point (csrc/decode.hip: llx_gemv_bf16_dora) is exported, declared in include/llx.h and
bound in llx/_lib.py, and validates its arguments before any launch (an error code and a message that begins with its name; no GPU
needed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p


def _call(lib, *, K=1024, M=1, n0=64, n1=0, c0=16, c1=None):
    w1 = P(16) if n1 else None
    return lib.llx_gemv_bf16_dora(P(16), K, n0, w1, K if n1 else 0, n1, None, 0, 0, P(16), K, M, K, None, 0.0, 0, P(16), n0 + n1, None, 0, None, 0, 0,
                                  None, None, 0, 0, None, None, None, None, 0, 0, 0, None, 0, 0.0, P(c0) if c0 else None, P(c1) if c1 else None, None,
                                  None)


def test_gemv_bf16_dora_is_exported_declared_and_bound():
    from llx import _lib as L

    lib = L.load()
    assert hasattr(lib, "llx_gemv_bf16_dora")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llx.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+llx_gemv_bf16_dora\s*\(", text), "llx_gemv_bf16_dora is not declared in include/llx.h"
    # llx_gemv_bf16's argument list + three factor pointers, stream last
    base, dora = L.SIGNATURES["llx_gemv_bf16"][1], L.SIGNATURES["llx_gemv_bf16_dora"][1]
    assert dora == base[:-1] + [ctypes.c_void_p] * 3 + base[-1:]


def test_gemv_bf16_dora_rejects_before_launch():
    from llx import _lib as L

    lib = L.load()

    def rejected(what, **kw):
        assert _call(lib, **kw) == -1, what
        msg = lib.llx_last_error_string()
        assert msg.startswith(b"llx_gemv_bf16_dora:"), (what, msg)
        return msg

    assert b"null scale" in rejected("segment 1 present, colscale1 null", n1=64, c0=16, c1=None)
    assert b"null scale" in rejected("colscale0 null", c0=0)
    assert b"2-byte aligned" in rejected("odd colscale address", c0=17)
    assert b"2-byte aligned" in rejected("odd colscale1 address", n1=64, c0=16, c1=33)
    assert b"M=5" in rejected("M = 5", M=5)
    assert b"K=1028" in rejected("K % 8 != 0", K=1028)
