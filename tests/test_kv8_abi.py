"""CPU: the FP8 KV cache entry points (csrc/kvcache.hip: llx_kv_scatter_f8, llx_kv_scatter_rows_f8, llx_kv_dequantize_f8; csrc/decode.hip:
llx_attn_decode_f8) are exported, declared in include/llx.h and bound in llx/_lib.py, and refuse bad arguments before any launch with a
message that names the function; epilogue 4 (q|k|v into FP8 caches) is known to all eight weight-stream entry points and epilogue 5 to
none (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
NAMES = ("llx_kv_scatter_f8", "llx_kv_scatter_rows_f8", "llx_kv_dequantize_f8", "llx_attn_decode_f8")
GEMVS = ("llx_gemv_bf16", "llx_gemv_bf16_dora", "llx_gemv_i8", "llx_gemv_mxfp4")
ROWS16 = ("llx_gemm_rows16_bf16", "llx_gemm_rows16_i8", "llx_gemm_rows16_bf16_lora", "llx_gemm_rows16_i8_lora")


@pytest.fixture(scope="module")
def lib():
    from llx import _lib as L

    return L.load()


def _err(lib, rc, *needles):
    msg = lib.llx_last_error_string() or b""
    assert rc == -1, (rc, msg)
    for n in needles:
        assert n in msg, (n, msg)


def test_entry_points_are_exported_declared_and_bound(lib):
    from llx import _lib as L

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llx.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name) and name in L.SIGNATURES
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in include/llx.h"
    # the bf16 entry points' argument lists: the cache kind is in the name, the strides are bytes
    for f8, bf in (("llx_kv_scatter_f8", "llx_kv_scatter"), ("llx_kv_scatter_rows_f8", "llx_kv_scatter_rows"), ("llx_attn_decode_f8", "llx_attn_decode")):
        assert L.SIGNATURES[f8] == L.SIGNATURES[bf]
    assert lib.llx_version() == 105


def _scatter(lib, rows, *, k=16, v=16, kc=16, vc=16, pos=16, s=(4096, 128, 512), c=(65536, 8192, 128), p_sb=4, B=1, KVH=4, L=4, Smax=64, hd=128):
    a = [P(k) if k else None, P(v) if v else None, *s, P(kc) if kc else None, P(vc) if vc else None, *c, P(pos) if pos else None]
    if rows:
        return lib.llx_kv_scatter_rows_f8(*a, p_sb, B, KVH, L, Smax, hd, None)
    return lib.llx_kv_scatter_f8(*a, B, KVH, L, Smax, hd, None)


@pytest.mark.parametrize("rows", [False, True])
def test_scatter_rejects_before_launch(lib, rows):
    fn = b"llx_kv_scatter_rows_f8" if rows else b"llx_kv_scatter_f8"
    for kw in (dict(k=0), dict(v=0), dict(kc=0), dict(vc=0), dict(pos=0)):
        _err(lib, _scatter(lib, rows, **kw), fn + b": null pointer")
    _err(lib, _scatter(lib, rows, hd=64), fn + b": head_dim=64")
    for kw in (dict(k=8), dict(v=24), dict(kc=8), dict(vc=4)):
        _err(lib, _scatter(lib, rows, **kw), fn + b": pointers must be 16-byte aligned")
    _err(lib, _scatter(lib, rows, s=(4096, 128, 516)), fn + b": bad strides")           # source rows off 16 bytes
    _err(lib, _scatter(lib, rows, c=(65536, 8192, 136)), fn + b": bad strides")         # cache rows (bytes) off 16 bytes
    _err(lib, _scatter(lib, rows, c=(65536, 8200, 128)), fn + b": bad strides")
    _err(lib, _scatter(lib, rows, c=(65536, 8192, 64)), fn + b": bad strides")          # positions that overlap
    for kw in (dict(B=0), dict(KVH=0), dict(L=0), dict(Smax=0)):
        _err(lib, _scatter(lib, rows, **kw), fn + b": bad sizes")
    if rows:
        _err(lib, _scatter(lib, rows, p_sb=3), fn + b": bad sizes")                     # a position row shorter than L


def test_dequantize_rejects_before_launch(lib):
    dq, fn = lib.llx_kv_dequantize_f8, b"llx_kv_dequantize_f8"
    _err(lib, dq(None, 65536, 8192, 128, P(16), 1, 4, 64, 128, None), fn + b": null pointer")
    _err(lib, dq(P(16), 65536, 8192, 128, None, 1, 4, 64, 128, None), fn + b": null pointer")
    _err(lib, dq(P(16), 65536, 8192, 128, P(16), 1, 4, 64, 64, None), fn + b": head_dim=64")
    _err(lib, dq(P(8), 65536, 8192, 128, P(16), 1, 4, 64, 128, None), fn + b": pointers must be 16-byte aligned")
    _err(lib, dq(P(16), 65536, 8192, 128, P(8), 1, 4, 64, 128, None), fn + b": pointers must be 16-byte aligned")
    _err(lib, dq(P(16), 65536, 8192, 136, P(16), 1, 4, 64, 128, None), fn + b": bad strides")
    _err(lib, dq(P(16), 65536, 8192, 64, P(16), 1, 4, 64, 128, None), fn + b": bad strides")
    _err(lib, dq(P(16), 65536, 8192, 128, P(16), 0, 4, 64, 128, None), fn + b": bad sizes")
    _err(lib, dq(P(16), 65536, 8192, 128, P(16), 1, 4, 0, 128, None), fn + b": bad sizes")


def _decode(lib, *, q=16, kc=16, vc=16, o=16, mask=16, ws=16, qs=(4096, 128, 1024), cs=(65536, 8192, 128), H=8, KVH=2, M=1, Skv=64, nsplit=2, hd=128):
    return lib.llx_attn_decode_f8(P(q) if q else None, *qs, P(kc) if kc else None, P(vc) if vc else None, *cs, P(o) if o else None, 1024, 128, 1024,
                                  P(mask) if mask else None, 0, 0, 64, None, ctypes.cast(P(ws) if ws else None, ctypes.c_void_p), 1, H, KVH, M, Skv, nsplit, hd,
                                  0.088, None)


def test_attn_decode_f8_rejects_before_launch(lib):
    fn = b"llx_attn_decode_f8"
    for kw in (dict(q=0), dict(kc=0), dict(vc=0), dict(o=0), dict(mask=0), dict(ws=0)):
        _err(lib, _decode(lib, **kw), fn + b": null pointer")
    _err(lib, _decode(lib, hd=64), fn + b": head_dim=64")
    _err(lib, _decode(lib, H=8, KVH=3), fn + b": bad sizes")
    _err(lib, _decode(lib, nsplit=0), fn + b": bad sizes")
    _err(lib, _decode(lib, H=16, KVH=2, M=3), fn + b": 24 query rows")
    for kw in (dict(kc=8), dict(vc=24), dict(q=8), dict(ws=8), dict(cs=(65536, 8192, 132)), dict(cs=(65536, 8196, 128))):
        _err(lib, _decode(lib, **kw), fn + b": rows must be 16-byte aligned")


def _stream(lib, name, *, epilogue, kc=16, vc=16, rope=16, pos=16):
    """A call of weight-stream entry point `name` whose common operands are fine (K = 2048, one segment of 384 rows = a q, a k and a v
    head) and whose remaining operands - scales, adapters, workspace - are absent: the q|k|v check comes before theirs."""
    from llx import _lib as L

    rows16 = name in ROWS16
    types = L.SIGNATURES[name][1]
    a = [P(16), 1024 if name == "llx_gemv_mxfp4" else 2048, 384, None, 0, 0, None, 0, 0, P(16), 2048, 2 if rows16 else 1, 2048, None, 0.0, epilogue, P(16), 128,
         None, 0, P(rope) if rope else None, 128, 128, P(kc) if kc else None, P(vc) if vc else None]
    a += [65536, 8192, 128, 64, P(pos) if pos else None] if rows16 else [8192, 128, P(pos) if pos else None]
    for t in types[len(a):]:
        a.append(None if t is ctypes.c_void_p else (0.0 if t is ctypes.c_float else 0))
    return getattr(lib, name)(*a)


@pytest.mark.parametrize("name", GEMVS + ROWS16)
def test_epilogue_4_is_known_and_5_is_not(lib, name):
    fn = name.encode()
    for missing in ("kc", "vc", "rope", "pos"):
        _err(lib, _stream(lib, name, epilogue=4, **{missing: None}), fn + b": bad q|k|v epilogue arguments")
    # the caches hold bytes: 4-byte alignment is enough for the codes (2 is not), the bf16 epilogue keeps its 8
    _err(lib, _stream(lib, name, epilogue=4, kc=18), fn + b": bad q|k|v epilogue arguments")
    _err(lib, _stream(lib, name, epilogue=2, vc=20), fn + b": bad q|k|v epilogue arguments")
    _err(lib, _stream(lib, name, epilogue=5), fn + b": unknown epilogue 5")
    _err(lib, _stream(lib, name, epilogue=-1), fn + b": unknown epilogue -1")
