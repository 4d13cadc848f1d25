"""CPU: llx_logprob_rows_fwd / llx_logprob_rows_bwd / llx_logprob_map_rows validate their arguments before any launch - a bad argument returns -1 and leaves
a message (no GPU needed), as llx_ce_fwd_bwd does."""
import ctypes

import pytest

Q = ctypes.c_void_p(8192)
P = ctypes.c_void_p(4096)  # a non-null, 16-byte aligned address that is never dereferenced: every call below fails its checks first


@pytest.fixture(scope="module")
def lib():
    from llx import _lib as L

    return L.load()


def _fwd(lib, *, logits=P, ld=16, labels=P, logp=P, lse=P, top1=None, T=4, V=16, rows=None):
    return lib.llx_logprob_rows_fwd(logits, ld, labels, logp, lse, top1, T, V, rows, None)


def _bwd(lib, *, logits=P, ld=16, dlogits=P, dld=16, labels=P, lse=P, g=P, T=4, V=16, rows=None):
    return lib.llx_logprob_rows_bwd(logits, ld, dlogits, dld, labels, lse, g, T, V, rows, None)


@pytest.mark.parametrize("bad,msg", [
    (dict(logits=None), b"null pointer"), (dict(labels=None), b"null pointer"), (dict(logp=None), b"null pointer"), (dict(lse=None), b"null pointer"),
    (dict(V=12, ld=16), b"multiples of 8"), (dict(ld=12, V=8), b"multiples of 8"), (dict(T=0), b"bad sizes"), (dict(V=16, ld=8), b"bad sizes"),
    (dict(rows=ctypes.c_void_p(4098)), b"rows must be a device int32 pointer"), (dict(logits=ctypes.c_void_p(4104)), b"16-byte aligned"),
])
def test_forward_rejects_bad_arguments(lib, bad, msg):
    assert _fwd(lib, **bad) == -1
    err = lib.llx_last_error_string()
    assert err.startswith(b"llx_logprob_rows_fwd") and msg in err, err


@pytest.mark.parametrize("bad,msg", [
    (dict(logits=None), b"null pointer"), (dict(dlogits=None), b"null pointer"), (dict(labels=None), b"null pointer"), (dict(lse=None), b"null pointer"),
    (dict(g=None), b"null pointer"), (dict(V=12), b"multiples of 8"), (dict(ld=12, V=8), b"multiples of 8"), (dict(dld=12, V=8), b"multiples of 8"),
    (dict(T=0), b"bad sizes"), (dict(V=16, dld=8), b"bad sizes"), (dict(rows=ctypes.c_void_p(4098)), b"rows must be a device int32 pointer"),
    (dict(dlogits=ctypes.c_void_p(4104)), b"16-byte aligned"),
])
def test_backward_rejects_bad_arguments(lib, bad, msg):
    assert _bwd(lib, **bad) == -1
    err = lib.llx_last_error_string()
    assert err.startswith(b"llx_logprob_rows_bwd") and msg in err, err


@pytest.mark.parametrize("args,msg", [
    ((None, P, Q, 0.0, None, None, 0, 4), b"null pointer"), ((P, None, Q, 0.0, None, None, 0, 4), b"null pointer"),
    ((P, P, None, 0.0, None, None, 0, 4), b"null pointer"), ((P, P, Q, 0.0, P, None, 0, 4), b"null pointer"),
    ((P, P, Q, 0.0, None, None, 0, 0), b"bad T"), ((P, P, P, 0.0, None, None, 0, 4), b"must differ"),
])
def test_map_rows_rejects_bad_arguments(lib, args, msg):
    assert lib.llx_logprob_map_rows(*args, None) == -1
    err = lib.llx_last_error_string()
    assert err.startswith(b"llx_logprob_map_rows") and msg in err, err
