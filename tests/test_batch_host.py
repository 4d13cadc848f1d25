"""CPU: the batched-decode entry points reject bad arguments before any launch, and the history bookkeeping of a batched generate()."""
import ctypes

import torch

P16 = ctypes.c_void_p(16)


def _rows16(lib, *, M=2, K=64, n0=64, epilogue=0, kc=None, vc=None, pos=None, rope=None):
    return lib.llx_gemm_rows16_bf16(P16, K, n0, None, 0, 0, None, 0, 0, P16, K, M, K, None, 0.0, epilogue, P16, n0, None, 0, rope, 128 if epilogue == 2 else 0,
                                    0, kc, vc, 0, 0, 128, 16, pos, None, 0, None)


def test_batched_entry_points_reject_bad_arguments():
    from llx import _lib as L

    lib = L.load()
    for M in (0, 17):
        assert _rows16(lib, M=M) == -1 and b"outside 2..16" in lib.llx_last_error_string()
    assert _rows16(lib, K=100) == -1 and b"multiple of 8" in lib.llx_last_error_string()
    # q|k|v mode without caches, positions or table
    assert _rows16(lib, n0=384, epilogue=2, kc=None, vc=None, pos=P16, rope=P16) == -1 and b"q|k|v" in lib.llx_last_error_string()
    assert _rows16(lib, n0=384, epilogue=2, kc=P16, vc=P16, pos=None, rope=P16) == -1 and b"q|k|v" in lib.llx_last_error_string()
    assert _rows16(lib, epilogue=1) == -1 and b"residual" in lib.llx_last_error_string()
    assert _rows16(lib, epilogue=7) == -1 and b"epilogue" in lib.llx_last_error_string()
    # a product that splits K needs its workspace: K = 4096 with 4 tiles is cut into 16 slices
    assert lib.llx_gemm_rows16_workspace_bytes(16, 64, 4096, 0) == 4 * 16 * 1024  # 4 tiles x 16 slices x one fp32 16 x 16 tile
    assert lib.llx_gemm_rows16_workspace_bytes(2, 64, 256, 0) == 0  # one slice: no partial tiles
    assert _rows16(lib, K=4096) == -1 and b"workspace" in lib.llx_last_error_string()
    rc = lib.llx_kv_scatter_rows(P16, P16, 0, 0, 0, P16, P16, 0, 0, 0, None, 1, 1, 1, 1, 8, 128, None)
    assert rc == -1 and b"null" in lib.llx_last_error_string()
    rc = lib.llx_kv_scatter_rows(P16, P16, 0, 0, 0, P16, P16, 0, 0, 0, P16, 1, 2, 1, 4, 8, 128, None)
    assert rc == -1 and b"bad sizes" in lib.llx_last_error_string()  # a position row shorter than L
    rc = lib.llx_kv_scatter_rows(P16, P16, 0, 0, 0, P16, P16, 0, 0, 0, P16, 1, 1, 1, 1, 8, 64, None)
    assert rc == -1 and b"head_dim" in lib.llx_last_error_string()


def test_history_bookkeeping_of_a_ragged_batch():
    from llx.generate import history_column, history_plan, history_rows

    for lens, n in (([40, 17, 29], 12), ([5, 5, 5, 5], 3), ([1, 9], 1), ([7], 4)):
        cols, base, shifts = history_plan(lens, n)
        assert cols == max(lens) - min(lens) + n and base == min(lens) - 1 and shifts == [v - min(lens) for v in lens]
        # the sampler writes the token drawn at counter pos to column pos - base: row b's k-th token is drawn at pos = lens[b] - 1 + k
        hist = torch.full((len(lens), cols), -1, dtype=torch.int64)
        for b, v in enumerate(lens):
            for k in range(n):
                col = (v - 1 + k) - base
                assert col == history_column(lens, b, k) == shifts[b] + k and 0 <= col < cols
                hist[b, col] = 100 * b + k
        full = history_rows(hist, shifts, torch.full((len(lens),), n), n, 999)
        assert full.tolist() == [[100 * b + k for k in range(n)] for b in range(len(lens))]
        # rows that ended early: their first counts[b] tokens, then the pad; the width is the longest row
        counts = torch.tensor([max(1, n - b) for b in range(len(lens))])
        T = int(counts.max())
        cut = history_rows(hist, shifts, counts, T, 999)
        assert cut.shape == (len(lens), T)
        assert cut.tolist() == [[100 * b + k if k < int(counts[b]) else 999 for k in range(T)] for b in range(len(lens))]
