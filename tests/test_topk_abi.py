"""CPU: llx_topk_logprobs_rows / llx_topk_map_rows exist, are declared in include/llx.h and bound in llx/_lib.py, and validate their
arguments before any launch - a bad argument returns -1 and leaves a message that begins with the export's name (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(4096)  # non-null, 16-byte aligned, never dereferenced: every call below fails its checks first
Q = ctypes.c_void_p(8192)
ODD2 = ctypes.c_void_p(4098)  # aligned to 2 bytes only
ODD4 = ctypes.c_void_p(4100)  # aligned to 4 bytes, not to 8 or 16


@pytest.fixture(scope="module")
def lib():
    from llx import _lib as L

    return L.load()


def test_exports_declared_and_bound(lib):
    from llx import _lib as L
    from llx import kernels as K

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llx.h")).read(), flags=re.S)
    for name in ("llx_topk_logprobs_rows", "llx_topk_map_rows"):
        assert hasattr(lib, name) and name in L.SIGNATURES and re.search(r"\b%s\s*\(" % name, header), name
    assert len(L.SIGNATURES["llx_topk_logprobs_rows"][1]) == 17 and len(L.SIGNATURES["llx_topk_map_rows"][1]) == 8
    assert lib.llx_version() == 105
    assert K.TOPK_MAX == 8 and callable(K.topk_logprobs_rows) and callable(K.topk_map_rows)


def _topk(lib, *, logits=P, ld=16, R=4, V=16, k=5, lse=None, label_logp=None, labels=None, rows=None, pos=None, hist_base=0, finished=None,
          ids=P, logp=Q, ld_out=8, hist_cap=0):
    return lib.llx_topk_logprobs_rows(logits, ld, R, V, k, lse, label_logp, labels, rows, pos, hist_base, finished, ids, logp, ld_out, hist_cap, None)


@pytest.mark.parametrize("bad,msg", [
    (dict(k=0), b"k = 0 outside 1..8"), (dict(k=9, ld_out=9), b"k = 9 outside 1..8"), (dict(k=-1), b"outside 1..8"),
    (dict(V=12), b"multiples of 8"), (dict(ld=20, V=16), b"multiples of 8"),
    (dict(logits=None), b"null pointer"), (dict(ids=None), b"null pointer"), (dict(logp=None), b"null pointer"),
    (dict(logits=ODD4), b"16-byte aligned"), (dict(ids=ODD2), b"aligned to 4 bytes"), (dict(logp=ODD2), b"aligned to 4 bytes"),
    (dict(lse=ODD2), b"aligned to 4 bytes"), (dict(labels=ODD4), b"aligned to 8 bytes"), (dict(pos=ODD4, hist_cap=4, ld_out=20), b"aligned to 8 bytes"),
    (dict(R=0), b"bad sizes"), (dict(V=16, ld=8), b"bad sizes"), (dict(ld_out=4), b"ld_out must be at least k"),
    (dict(labels=P, pos=P), b"exclude each other"), (dict(rows=P), b"rows goes with labels"), (dict(label_logp=P, labels=P), b"label_logp goes with"),
    (dict(finished=P), b"finished goes with pos"), (dict(pos=P, hist_cap=0), b"hist_cap > 0"), (dict(pos=P, hist_cap=4, ld_out=19), b"ld_out >= hist_cap * k"),
])
def test_topk_rejects_bad_arguments(lib, bad, msg):
    assert _topk(lib, **bad) == -1
    err = lib.llx_last_error_string()
    assert err.startswith(b"llx_topk_logprobs_rows") and msg in err, err


@pytest.mark.parametrize("args,msg", [
    ((None, P, P, Q, Q, 4, 3), b"null pointer"), ((P, None, P, Q, Q, 4, 3), b"null pointer"), ((P, P, None, Q, Q, 4, 3), b"null pointer"),
    ((P, P, P, None, Q, 4, 3), b"null pointer"), ((P, P, P, Q, None, 4, 3), b"null pointer"), ((P, P, P, Q, Q, 0, 3), b"bad T"),
    ((P, P, P, Q, Q, 4, 0), b"outside 1..8"), ((P, P, P, Q, Q, 4, 9), b"outside 1..8"), ((P, P, P, P, Q, 4, 3), b"must differ"),
])
def test_map_rows_rejects_bad_arguments(lib, args, msg):
    assert lib.llx_topk_map_rows(*args, None) == -1
    err = lib.llx_last_error_string()
    assert err.startswith(b"llx_topk_map_rows") and msg in err, err
