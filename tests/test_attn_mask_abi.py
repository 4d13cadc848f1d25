"""CPU: the mask-driven attention entries (KV-cache prefill) are declared, exported and bound, and their host-only parts answer."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("llx_attn_mask_flags_bytes", "llx_attn_mask_tile_flags", "llx_attn_mask_fwd")


def test_symbols_in_header_library_and_ctypes_table():
    from llx import _lib as L

    lib = L.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llx.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/llx.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES, f"{name} has no ctypes signature"
    assert lib.llx_version() == 105


def test_flags_bytes_and_argument_checks():
    from llx import _lib as L

    lib = L.load()
    assert lib.llx_attn_mask_flags_bytes(2, 300, 700) == 2 * 3 * 11  # 128-row blocks x 64-key tiles
    assert lib.llx_attn_mask_flags_bytes(1, 4096, 8192) == 32 * 128
    p = ctypes.c_void_p(16)
    # validation happens before any launch: no GPU needed
    rc = lib.llx_attn_mask_fwd(p, 0, 0, p, 0, 0, 0, p, 0, 0, 0, p, 0, 0, None, p, 0, 128, p, 1, 8, 128, 4, 1, 64, 0.1, None)
    assert rc == -1 and b"head_dim" in lib.llx_last_error_string()
    rc = lib.llx_attn_mask_fwd(p, 0, 0, p, 0, 0, 0, p, 0, 0, 0, p, 0, 0, None, p, 0, 3, p, 1, 8, 3, 4, 1, 128, 0.1, None)
    assert rc == -1 and b"Skv" in lib.llx_last_error_string()
    rc = lib.llx_attn_mask_tile_flags(p, 0, 3, p, 1, 8, 3, None)
    assert rc == -1 and b"Skv" in lib.llx_last_error_string()
