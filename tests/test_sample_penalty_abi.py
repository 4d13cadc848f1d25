"""CPU: the extended sampler entry point (csrc/sample.hip: llx_sample_rows_ext) is exported, declared in include/llx.h and bound in
llx/_lib.py, and validates its arguments before any launch (an error code and a message that begins with its name; no GPU needed)."""
import ctypes
import math
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
NAME = b"llx_sample_rows_ext:"


def _call(lib, *, logits=16, dtype=0, ld=1024, R=1, V=1000, temperature=1.0, top_k=0, top_p=1.0, pos=16, out=16, history=None, cap=0,
          counts=None, ldc=0, theta=1.0, alpha_p=0.0, alpha_f=0.0, logprob=None):
    return lib.llx_sample_rows_ext(P(logits) if logits else None, dtype, ld, R, V, temperature, top_k, top_p, 1234, P(pos) if pos else None,
                                   P(out) if out else None, history, cap, cap, 0, 0, -1, None, None, None, None, counts, ldc, theta, alpha_p,
                                   alpha_f, logprob, None)


def test_sample_rows_ext_is_exported_declared_and_bound():
    from llx import _lib as L

    lib = L.load()
    assert hasattr(lib, "llx_sample_rows_ext")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llx.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+llx_sample_rows_ext\s*\(([^;]*)\)\s*;", text)
    assert m, "llx_sample_rows_ext is not declared in include/llx.h"
    decl = [a.strip() for a in m.group(1).split(",")]
    res, args = L.SIGNATURES["llx_sample_rows_ext"]
    assert res is ctypes.c_int and len(args) == len(decl)
    # the arguments of llx_sample_rows, then the six new ones, then the stream
    plain = re.search(r"\bint\s+llx_sample_rows\s*\(([^;]*)\)\s*;", text)
    base = [a.strip() for a in plain.group(1).split(",")]
    assert decl[: len(base) - 1] == base[:-1] and args[: len(base) - 1] == L.SIGNATURES["llx_sample_rows"][1][:-1]
    assert decl[len(base) - 1 :] == ["int32_t* counts", "int64_t ldc", "float repetition_penalty", "float presence_penalty",
                                    "float frequency_penalty", "float* logprob_history", "llx_stream_t s"]
    assert args[len(base) - 1 :] == [P, ctypes.c_int64, ctypes.c_float, ctypes.c_float, ctypes.c_float, P, P]
    assert lib.llx_version() == 105


def test_sample_rows_ext_rejects_before_launch():
    from llx import _lib as L

    lib = L.load()
    err = lib.llx_last_error_string
    # the checks it shares with llx_sample_rows carry its own name
    assert _call(lib, top_p=0.0) == -1 and b"top_p" in err() and err().startswith(NAME)
    assert _call(lib, temperature=-0.5) == -1 and b"temperature" in err() and err().startswith(NAME)
    assert _call(lib, V=0) == -1 and b"V=0" in err() and err().startswith(NAME)
    assert _call(lib, logits=0) == -1 and b"null" in err() and err().startswith(NAME)
    assert _call(lib, ld=999) == -1 and b"stride" in err() and err().startswith(NAME)
    assert _call(lib, history=P(16), cap=0) == -1 and b"history" in err() and err().startswith(NAME)
    # theta finite and > 0
    for theta in (0.0, -1.0, math.nan, math.inf):
        assert _call(lib, theta=theta) == -1 and b"repetition_penalty" in err() and err().startswith(NAME), theta
    # alpha finite
    for bad in (math.nan, math.inf, -math.inf):
        assert _call(lib, alpha_p=bad) == -1 and b"presence_penalty" in err() and err().startswith(NAME), bad
        assert _call(lib, alpha_f=bad) == -1 and b"frequency_penalty" in err() and err().startswith(NAME), bad
    # counts: 4-byte aligned, row stride >= V
    assert _call(lib, counts=P(18), ldc=1000) == -1 and b"counts" in err() and b"aligned" in err() and err().startswith(NAME)
    assert _call(lib, counts=P(16), ldc=999) == -1 and b"ldc" in err() and err().startswith(NAME)
    # logprob_history shares the geometry of history
    assert _call(lib, logprob=P(16)) == -1 and b"logprob_history" in err() and err().startswith(NAME)
