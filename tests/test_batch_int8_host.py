"""CPU: the int8 entry point of the batched decode stream (llx_gemm_rows16_i8) rejects bad arguments before any launch, and its
workspace function follows the plan stated above rows16_plan in csrc/decode_rows.hip."""
import ctypes

P16 = ctypes.c_void_p(16)


def _rows16_i8(lib, *, M=2, K=64, n0=64, epilogue=0, kc=None, vc=None, pos=None, rope=None, scale=P16, res=None):
    return lib.llx_gemm_rows16_i8(P16, K, n0, None, 0, 0, None, 0, 0, P16, K, M, K, None, 0.0, epilogue, P16, n0, res, n0 if res else 0, rope,
                                  128 if epilogue == 2 else 0, 0, kc, vc, 0, 0, 128, 16, pos, None, 0, scale, None, None, None)


def test_int8_batched_entry_point_rejects_bad_arguments():
    from llx import _lib as L

    lib = L.load()
    for M in (1, 17):
        assert _rows16_i8(lib, M=M) == -1 and b"outside 2..16" in lib.llx_last_error_string()
    assert _rows16_i8(lib, K=100) == -1 and b"multiple of 16" in lib.llx_last_error_string()
    assert _rows16_i8(lib, scale=None) == -1 and b"null scale" in lib.llx_last_error_string()
    # q|k|v mode without caches or positions
    assert _rows16_i8(lib, n0=384, epilogue=2, kc=None, vc=None, pos=P16, rope=P16) == -1 and b"q|k|v" in lib.llx_last_error_string()
    assert _rows16_i8(lib, n0=384, epilogue=2, kc=P16, vc=P16, pos=None, rope=P16) == -1 and b"q|k|v" in lib.llx_last_error_string()
    assert _rows16_i8(lib, epilogue=1) == -1 and b"residual" in lib.llx_last_error_string()
    # a split K with no workspace: K = 4096 with 4 tiles is cut into 8 slices of one 512-element batch
    assert _rows16_i8(lib, K=4096) == -1 and b"workspace" in lib.llx_last_error_string()
    assert b"llx_gemm_rows16_i8" in lib.llx_last_error_string()


def test_int8_workspace_follows_the_plan():
    """The plan's rules with the int8 sizes: a batch is 512 elements; ks_max = the largest multiple of 512 with M * KS bytes <= 60 KiB;
    S = max(ceil(K / ks_max), min(ceil(2048 / ntiles), ceil(K / 512), 64)), then the first count up to 2 S that cuts K into equal
    slices of whole batches; the workspace is a 64-byte header (16 row scales) + ntiles * S int32 tiles of 1 KiB, 0 without a split."""
    from llx import _lib as L

    lib = L.load()
    wsb = lib.llx_gemm_rows16_i8_workspace_bytes
    assert wsb(2, 64, 512, 0) == 0  # one batch: one slice
    # N = 64: 4 tiles ask for 512 slices, K = 4096 has 8 batches -> S = 8 equal slices of 512
    assert wsb(16, 64, 4096, 0) == 64 + 4 * 8 * 1024
    # N = 4096 (256 tiles) at K = 14336 (28 batches): 8 slices asked; 8 .. 13 do not cut 28 batches evenly, 14 does -> S = 14 x 1024
    assert wsb(16, 4096, 14336, 0) == 64 + 256 * 14 * 1024
    # K = 1040: 3 slices of 512, 512 and 16 elements (no equal cut exists)
    assert wsb(5, 36, 1040, 0) == 64 + 3 * 3 * 1024
    # the LDS cap: N = 16400 (1025 tiles) asks for 2 slices; at M = 16 a slice holds at most 3584 elements (16 x 3584 B = 56 KiB,
    # 16 x 4096 B > 60 KiB), so K = 8192 needs 3, and 4 is the first equal cut; at M = 2 two slices of 4096 fit
    assert wsb(2, 16400, 8192, 0) == 64 + 1025 * 2 * 1024
    assert wsb(16, 16400, 8192, 0) == 64 + 1025 * 4 * 1024
    # SwiGLU: a tile is 8 hidden units -> N = 2 x 1792 is 224 tiles, 10 slices asked, K = 512 is one batch
    assert wsb(2, 2 * 1792, 512, 3) == 0
    assert wsb(2, 2 * 1792, 1024, 3) == 64 + 224 * 2 * 1024
    # outside the entry point's range: nothing to allocate
    assert wsb(1, 64, 4096, 0) == 0 and wsb(17, 64, 4096, 0) == 0
    # the bf16 function keeps its results (tests/test_batch_host.py)
    assert lib.llx_gemm_rows16_workspace_bytes(16, 64, 4096, 0) == 4 * 16 * 1024
    assert lib.llx_gemm_rows16_workspace_bytes(2, 64, 256, 0) == 0
