"""CPU: the sampler entry point (csrc/sample.hip: llx_sample_rows) is exported, declared in include/llx.h and bound in llx/_lib.py, and
validates its arguments before any launch (an error code and a message naming the cause; no GPU needed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p


def _call(lib, *, logits=16, dtype=0, ld=1024, R=1, V=1000, temperature=1.0, top_k=0, top_p=1.0, pos=16, out=16, history=None, cap=0):
    return lib.llx_sample_rows(P(logits) if logits else None, dtype, ld, R, V, temperature, top_k, top_p, 1234, P(pos) if pos else None,
                               P(out) if out else None, history, cap, cap, 0, 0, -1, None, None, None, None, None)


def test_sample_rows_is_exported_declared_and_bound():
    from llx import _lib as L

    lib = L.load()
    assert hasattr(lib, "llx_sample_rows")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llx.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+llx_sample_rows\s*\(([^;]*)\)\s*;", text)
    assert m, "llx_sample_rows is not declared in include/llx.h"
    res, args = L.SIGNATURES["llx_sample_rows"]
    assert res is ctypes.c_int and len(args) == len(m.group(1).split(","))
    assert args[8] is ctypes.c_uint64 and "uint64_t seed" in m.group(1).split(",")[8]  # the seed is a full unsigned 64-bit value
    assert lib.llx_version() == 105


def test_sample_rows_rejects_before_launch():
    from llx import _lib as L

    lib = L.load()
    err = lib.llx_last_error_string
    assert _call(lib, top_p=0.0) == -1 and b"top_p" in err() and err().startswith(b"llx_sample_rows:")
    assert _call(lib, top_p=1.5) == -1 and b"top_p" in err()
    assert _call(lib, temperature=-0.5) == -1 and b"temperature" in err()
    assert _call(lib, V=0) == -1 and b"V=0" in err()
    assert _call(lib, R=0) == -1 and b"R=0" in err()
    assert _call(lib, top_k=-1) == -1 and b"top_k" in err()
    assert _call(lib, out=0) == -1 and b"null" in err()
    assert _call(lib, logits=0) == -1 and b"null" in err()
    assert _call(lib, pos=0) == -1 and b"null" in err()
    assert _call(lib, ld=999) == -1 and b"stride" in err()
    assert _call(lib, dtype=2) == -1 and b"dtype" in err()
    assert _call(lib, history=P(16), cap=0) == -1 and b"history" in err()
