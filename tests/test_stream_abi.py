"""CPU: the checks the eight weight-stream entry points (csrc/decode.hip, csrc/decode_rows.hip, csrc/mxfp4.hip) share on their common
operands (stream_check_fill of csrc/wstream.h).  Every entry point refuses each bad call before any launch, with a message that begins
with its own name, and where a call has two faults the same one wins everywhere (no GPU needed: nothing here gets as far as a launch)."""
import ctypes

import pytest

P = ctypes.c_void_p
GEMVS = ("llx_gemv_bf16", "llx_gemv_bf16_dora", "llx_gemv_i8", "llx_gemv_mxfp4")
ROWS16 = ("llx_gemm_rows16_bf16", "llx_gemm_rows16_i8", "llx_gemm_rows16_bf16_lora", "llx_gemm_rows16_i8_lora")
# the first 25 arguments of all eight (include/llx.h); pointers are given as small fake addresses, 0 = null
COMMON = ("w0", "ldw0", "n0", "w1", "ldw1", "n1", "w2", "ldw2", "n2", "x", "ldx", "M", "K", "norm_w", "eps", "epilogue", "out", "ldo", "res", "ldr",
          "rope", "n_q", "n_k", "k_cache", "v_cache")
POINTERS = ("w0", "w1", "w2", "x", "norm_w", "out", "res", "rope", "k_cache", "v_cache")


@pytest.fixture(scope="module")
def lib():
    from llx import _lib as L

    return L.load()


def _ldw(name):
    """The stride of a weight row of K = 2048 elements: bf16 elements, int8 bytes, or the bytes of a packed MXFP4 row."""
    return 1024 if name == "llx_gemv_mxfp4" else 2048


def _epl(name):
    """Weight elements per 16-byte load as the common checks see them (MXFP4 rows are checked in bytes)."""
    return 16 if "_i8" in name or name == "llx_gemv_mxfp4" else 8


def _m_range(name):
    return (2, 16) if name in ROWS16 else (1, 4)


def _m_note(name):
    if name in ROWS16:
        return b"one row runs %s, more than 16 the MFMA GEMM" % (b"llx_gemv_i8" if "_i8" in name else b"llx_gemv_bf16")
    return b"larger row counts run the MFMA GEMM" + (b" on the dequantised image" if name == "llx_gemv_mxfp4" else b"")


def _call(lib, name, **over):
    """Entry point `name` on common operands that pass every common check (K = 2048, one segment of 384 rows, no norm, epilogue 0) except
    for what `over` replaces; the operands behind the common ones - cache strides, positions, scales, adapters, workspace - are absent."""
    from llx import _lib as L

    v = dict(w0=16, ldw0=_ldw(name), n0=384, w1=0, ldw1=0, n1=0, w2=0, ldw2=0, n2=0, x=16, ldx=2048, M=_m_range(name)[0], K=2048,
             norm_w=0, eps=0.0, epilogue=0, out=16, ldo=384, res=0, ldr=0, rope=0, n_q=0, n_k=0, k_cache=0, v_cache=0)
    assert set(over) <= set(v)
    v.update(over)
    a = [(P(v[k]) if v[k] else None) if k in POINTERS else v[k] for k in COMMON]
    for t in L.SIGNATURES[name][1][len(a):]:
        a.append(None if t is ctypes.c_void_p else (0.0 if t is ctypes.c_float else 0))
    return getattr(lib, name)(*a)


def _err(lib, rc, want):
    msg = lib.llx_last_error_string() or b""
    assert rc == -1, (rc, msg)
    assert msg.startswith(want), (want, msg)


@pytest.mark.parametrize("name", GEMVS + ROWS16)
def test_common_rejections(lib, name):
    fn = name.encode()
    bad_k = 2048 + _epl(name) // 2  # a multiple of half the load width only
    for kw in (dict(w0=0), dict(x=0), dict(out=0)):
        _err(lib, _call(lib, name, **kw), fn + b": null pointer")
    lo, hi = _m_range(name)
    for M in (lo - 1, hi + 1):
        _err(lib, _call(lib, name, M=M), fn + b": M=%d outside %d..%d (%s)" % (M, lo, hi, _m_note(name)))
    if name == "llx_gemv_mxfp4":  # its own rule on K comes first: one scale byte per 32 elements
        _err(lib, _call(lib, name, K=bad_k), fn + b": K=%d must be a multiple of 32 (one scale per block of 32)" % bad_k)
    else:
        _err(lib, _call(lib, name, K=bad_k), fn + b": K=%d must be a multiple of %d and at most 32768" % (bad_k, _epl(name)))
    _err(lib, _call(lib, name, K=32800), fn + b": K=32800 must be a multiple of %d and at most 32768" % _epl(name))
    for kw in (dict(n0=0), dict(n1=128), dict(w1=16, n1=-16), dict(w1=16, n1=0, w2=16, n2=128), dict(w1=16, n1=128, n2=128)):
        _err(lib, _call(lib, name, **kw), fn + b": bad segment sizes")
    gran = 16 if name in ROWS16 else 4
    _err(lib, _call(lib, name, n0=386, w1=16, n1=128), fn + b": inner segment sizes must be multiples of %d" % gran)
    _err(lib, _call(lib, name, w1=16, n1=136 if gran == 16 else 130, w2=16, n2=128), fn + b": inner segment sizes must be multiples of %d" % gran)
    ldw = _ldw(name)
    for kw in (dict(ldw0=ldw + _epl(name) // 2), dict(w1=16, n1=128, ldw1=ldw + 4), dict(w1=16, n1=128, w2=16, n2=128, ldw2=ldw + 4), dict(ldx=2052)):
        _err(lib, _call(lib, name, **kw), fn + b": row strides must be multiples of 16 bytes")
    for kw in (dict(w0=24), dict(w1=8, n1=128), dict(w1=16, n1=128, w2=4, n2=128), dict(x=8), dict(norm_w=20)):
        _err(lib, _call(lib, name, **kw), fn + b": pointers must be 16-byte aligned")
    _err(lib, _call(lib, name, epilogue=1), fn + b": residual missing")
    for kw in (dict(w1=16, n1=256), dict(), dict(w1=16, n1=384, w2=16, n2=384)):
        _err(lib, _call(lib, name, epilogue=3, **kw), fn + b": the SwiGLU epilogue takes gate and up weights of equal size")


@pytest.mark.parametrize("name", GEMVS + ROWS16)
def test_which_message_wins(lib, name):
    """Two faults in one call: the checks run in one order for all eight entry points."""
    fn = name.encode()
    _err(lib, _call(lib, name, x=0, epilogue=7), fn + b": null pointer")
    _err(lib, _call(lib, name, epilogue=7, n0=0), fn + b": unknown epilogue 7")
    _err(lib, _call(lib, name, n0=386, w1=16, n1=128, ldx=2052), fn + b": inner segment sizes must be multiples of")
    _err(lib, _call(lib, name, w0=24, epilogue=1), fn + b": pointers must be 16-byte aligned")
    # MXFP4's own rule on K is checked before the common operands, the others' K after the pointers and M
    k = 2048 + _epl(name) // 2
    _err(lib, _call(lib, name, out=0, K=k), fn + (b": K=%d must be a multiple of 32" % k if name == "llx_gemv_mxfp4" else b": null pointer"))
    _err(lib, _call(lib, name, M=0, K=32800), fn + b": M=0 outside")


@pytest.mark.parametrize("name", [n for n in GEMVS + ROWS16 if n not in ("llx_gemv_bf16", "llx_gemm_rows16_bf16", "llx_gemm_rows16_bf16_lora")])
def test_scales_come_after_the_common_operands(lib, name):
    """The entry points whose weights carry scales (int8 rows, DoRA factors, MXFP4 scale bytes): a call whose common operands are fine is
    refused for its null scales, and a fault in the common operands wins over them."""
    fn = name.encode()
    if name == "llx_gemv_mxfp4":
        what = b"MXFP4 weight needs its scale bytes"
    else:
        what = (b"DoRA" if name.endswith("_dora") else b"int8") + b" weight needs its per-row scales"
    _err(lib, _call(lib, name), fn + b": null scale (every " + what + b")")
    _err(lib, _call(lib, name, ldx=2052), fn + b": row strides must be multiples of 16 bytes")
