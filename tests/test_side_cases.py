"""CPU checks of the side-kernel cases (tests/side_cases.py): every case reaches the dispatch class it is named for (a pure-Python
restatement of the dispatch rules, so that a later change of the dispatch fails here instead of silently moving a case onto a tested
path), the fp32 restatement of every kernel sits inside the bar the GPU test (tests/test_side_kernels_gpu.py) asserts against the
float64 reference, and every mutant lands at least ten times outside it on at least one case."""
import math

import pytest
import torch

from oracle import ref as O
from tests import side_cases as C


# ------------------------------------------------------------------------------------------------------------------ dispatch classes
@pytest.mark.parametrize("dim", list(C.RMS_DIMS))
def test_rmsnorm_dims_reach_their_class(dim):
    assert C.rms_class(dim) == C.RMS_DIMS[dim]


def test_rmsnorm_table_covers_every_instantiation_and_row_pattern():
    classes = {(c.full, c.nch) for c in C.RMS_DIMS.values()}
    assert {(True, 4), (True, 8), (True, 16)} <= classes and {(False, n) for n in (1, 2, 4, 8, 16)} <= classes
    guarded = [c for c in C.RMS_DIMS.values() if not c.full]
    assert any(c.absent for c in guarded if c.pipe) and any(c.absent for c in guarded if not c.pipe)        # a whole chunk absent
    assert any(c.last_lanes < 64 for c in guarded if c.pipe) and any(c.last_lanes < 64 for c in guarded if not c.pipe)  # a partial one
    assert C.RMS_DIMS[3072] == C.RmsClass(False, 8, True, 6, 64, 2)
    # forward: four rows per block
    assert [(-(-r // 4), r % 4) for r in C.RMS_FWD_ROWS] == [(1, 1), (1, 3), (1, 0), (2, 1)]
    # backward: a wave walks 0, 1, 2, 3 and 4 rows (the A / B register alternation leaves through its first exit on an odd count, its
    # second on an even one), a second block, a ragged last block
    per_wave = {n for r in C.RMS_BWD_ROWS_ALL for blk in C.rms_bwd_wave_rows(r) for n in blk}
    assert per_wave == {0, 1, 2, 3, 4}
    assert C.rms_bwd_wave_rows(17) == [[4, 4, 4, 4], [1, 0, 0, 0]] and C.rms_bwd_wave_rows(37)[-1] == [2, 1, 1, 1]
    assert C.rms_bwd_wave_rows(13) == [[4, 3, 3, 3]] and C.rms_bwd_wave_rows(9) == [[3, 2, 2, 2]]
    for dim, rows in C.RMS_BWD_ROWS.items():
        assert {5, 37} <= set(rows) and (set(rows) == set(C.RMS_BWD_ROWS_ALL)) == (dim in (3072, 5120))


@pytest.mark.parametrize("name", list(C.CE_CASES))
def test_ce_cases_reach_their_class(name):
    case = C.CE_CASES[name]
    cls = C.ce_class(case.V, case.T)
    assert (cls["lo"], cls["hi"], cls["idle"], cls["row_passes"]) == case.want


def test_ce_table_covers_the_row_decomposition():
    assert {c.want[:3] for c in C.CE_CASES.values()} == {(0, 1, 511), (0, 1, 1), (1, 1, 0), (1, 2, 0), (31, 32, 0)}
    assert {c.want[3] for c in C.CE_CASES.values()} == {1, 2}
    assert 128256 // 8 == 31 * 512 + 160  # 31 passes of the 512 threads and a partial one
    for V in C.CE_V:
        sp = C.ce_special_labels(V)
        assert {0, 7, V - 8, V - 1} <= set(sp) and all(0 <= s < V for s in sp)
        assert any(s % 2 for s in sp) and any(s % 2 == 0 for s in sp)  # both halves of a packed pair
        if V > 4096:
            assert {8, 4095, 4096, 13, 10} <= set(sp)  # thread 511's last element of pass 0, thread 0's first of pass 1
    d = C.ce_data(C.CE_CASES[C.CE_STRIDED])
    assert d["labels"].tolist()[:8] == C.ce_special_labels(4104) and d["labels"][8] == -100
    for name in ("v4104_t1025", "v8_t9", "v4088_t9", "v4096_t1025"):
        lab = C.ce_data(C.CE_CASES[name])["labels"]
        assert 0 < (lab == -100).sum() < lab.numel()
    assert (C.ce_data(C.CE_CASES["single"])["labels"] != -100).sum() == 1
    assert (C.ce_data(C.CE_CASES["all_ignored"])["labels"] != -100).sum() == 0
    # the compacted row counts sit on, below and above a chunk boundary, and one reaches into the last, ragged chunk
    assert [C.ce_rows_limit(c) for c in C.CE_CHUNK["counts"][1:]] == [256, 256, 512, 768]
    assert C.CE_CHUNK["T"] % C.CE_CHUNK["chunk"] != 0


def test_ce_dynamic_range_rows():
    d = C.ce_data(C.CE_CASES["range"])
    ref = C.ce_ref(d["logits"], d["labels"])
    assert d["logits"][0].float().mean() > 75
    assert ref["row"][1] < 1e-10 and abs(ref["row"][2].item() - C.PEAK) < 1.0  # label on the peak: ~0; off it: ~40
    assert torch.isnan(C.ce_ref(**{k: C.ce_data(C.CE_CASES["all_ignored"])[k] for k in ("logits", "labels")})["loss"])


def test_elementwise_shapes_reach_their_class():
    assert {d: C.emb_passes(d) for d in C.EMB_DIMS} == C.EMB_DIMS
    assert C.EMB_BWD["B"] * C.EMB_BWD["S"] <= 16 and C.EMB_BWD["dim"] % 256 != 0  # the bound of the bar; a ragged last pass of the 256 threads
    assert C.emb_bwd_ids("distinct").unique().numel() == 16 and C.emb_bwd_ids("one_id").unique().numel() == 1
    threads = {n: B * S * H * 16 for n, (B, S, H, W, SB, TS) in C.ROPE_CASES.items()}
    assert all(C.tail_block(t) for t in threads.values()) and threads["ragged"] > 256
    B, S, H, W, SB, TS = C.ROPE_CASES["strided"]
    assert B == 3 and SB > S and W > H * 128 and TS > S and C.ROPE_CASES["one_head"][2] == 1
    for name, (r, c) in C.SWIGLU_SHAPES.items():
        assert C.tail_block(r * c // 8)
    assert C.SWIGLU_SHAPES["cols8"][1] == 8 and C.SWIGLU_SHAPES["ragged"][0] * C.SWIGLU_SHAPES["ragged"][1] // 8 > 256
    g = C.swiglu_data("cols8")["g"].float().view(-1)[:12].tolist()
    assert g[::2] == C.bf(torch.tensor(C.SWIGLU_GATES)).float().tolist() and g[1::2] == [-v for v in g[::2]] and g[-2:] == [90.0, -90.0]
    for shape in (C.SCALE_SHAPE, C.ADD_SHAPE, C.GELU_SHAPE):
        assert C.tail_block(shape[0] * shape[1] // 8)
    z = C.gelu_data()["z"].float()
    assert z.min() == -6 and z.max() == 6 and (z == 0).any() and C.GELU_LD > C.GELU_SHAPE[1]
    for name, (M, Cc, P, stride) in C.COL2IM_CASES.items():
        assert C.col2im_guard_fires(M, P, stride), name
        assert P == (M + 2 if stride == 1 else None) or (stride == 2 and M == (P - 2 - 1) // 2 + 1)
    assert {(s, P % 2) for (M, Cc, P, s) in C.COL2IM_CASES.values()} == {(1, 0), (1, 1), (2, 0), (2, 1)}
    assert C.tail_block(103 * 64 // 8) and 103 * 64 // 8 > 256
    assert C.REORDER_SHAPE[1] % 8 != 0
    p = C.PREFIX
    assert p["L1"] % 2 == 1 and p["L2"] == (p["L1"] - 1) // 2 + 1 and p["B"] == 2


# ------------------------------------------------------------------------------------------------------ bars reachable and sharp
@pytest.mark.parametrize("dim", list(C.RMS_DIMS))
def test_rmsnorm_restatement_inside_the_bars(dim):
    worst = {}
    for rows in sorted(set(C.RMS_BWD_ROWS[dim]) | set(C.RMS_FWD_ROWS)):
        d = C.rms_data(dim, rows)
        ref = C.rms_ref(d)
        for k, v in C.rms_ratios(C.rms_f32(d), d, ref).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"[rmsnorm {dim}] restated / bar " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_rmsnorm_mutants_outside_the_bars():
    """Each mutant misses, by 10x or more, the bar of the output it corrupts on at least one (dim, rows) of the table."""
    seen = {"mean_over_nch": ("y", "rstd", "dx"), "drop_last_chunk": ("y", "dx", "dw"), "dw_lost_wave": ("dw",), "dres_before_rounding": ("join",)}
    where = {}
    for dim, rows in [(8, 5), (520, 37), (1536, 5), (1792, 37), (3072, 37), (5120, 16), (5120, 37), (8184, 5), (4096, 5)]:
        d = C.rms_data(dim, rows)
        ref = C.rms_ref(d)
        for m in C.RMS_MUTANTS:
            r = C.rms_ratios(C.rms_f32(d, m), d, ref)
            for k in seen[m]:
                where.setdefault((m, k), 0.0)
                where[(m, k)] = max(where[(m, k)], r[k])
    print("[rmsnorm] mutants / bar " + " ".join(f"{m}:{k} {v:.0f}x" for (m, k), v in where.items()))
    assert all(v >= 10.0 for v in where.values()), where
    # the FULL kernels have nothing for mean_over_nch to change: the mutant is invisible there, as the docstring says
    d = C.rms_data(4096, 5)
    assert C.rms_ratios(C.rms_f32(d, "mean_over_nch"), d, C.rms_ref(d))["y"] <= 1.0


@pytest.mark.parametrize("name", list(C.CE_CASES))
def test_ce_restatement_inside_the_bars(name):
    d = C.ce_data(C.CE_CASES[name])
    r = C.ce_ratios(C.ce_f32(d["logits"], d["labels"]), C.ce_ref(d["logits"], d["labels"]))
    print(f"[ce {name}] restated / bar loss {r['loss']:.3f} grad {r['grad']:.3f}")
    assert max(r.values()) <= 1.0, r


def test_ce_mutants_outside_the_bars():
    worst = {}
    for name in ("v8_t9", "v4104_t9", "v4104_t1025", "v128256_t9", "range"):
        d = C.ce_data(C.CE_CASES[name])
        ref = C.ce_ref(d["logits"], d["labels"])
        for m in C.CE_MUTANTS:
            r = C.ce_ratios(C.ce_f32(d["logits"], d["labels"], m), ref)
            for k, v in r.items():
                worst[(m, k)] = max(worst.get((m, k), 0.0), v)
    print("[ce] mutants / bar " + " ".join(f"{m}:{k} {v:.0f}x" for (m, k), v in worst.items()))
    assert worst[("norm_by_T", "loss")] >= 10 and worst[("norm_by_T", "grad")] >= 10
    # the one-hot does not enter the loss, and 8 of V columns move the log-sum-exp by less than 10x the loss bar: the gradient sees both
    assert worst[("onehot_off_by_one", "grad")] >= 10 and worst[("skip_last_chunk", "grad")] >= 10


@pytest.mark.parametrize("count", C.CE_CHUNK["counts"])
def test_ce_chunk_rows_inside_the_bars(count):
    d = C.ce_chunk_data(count)
    r = C.ce_ratios(C.ce_f32(d["logits"], d["labels"]), C.ce_ref(d["logits"], d["labels"]))
    assert max(r.values()) <= 1.0, r
    if count is not None:
        assert (d["labels"] != -100).sum() == count and (d["labels"][:count] != -100).all()


@pytest.mark.parametrize("name", list(C.SWIGLU_SHAPES))
def test_swiglu_restatement_inside_and_mutant_outside(name):
    d = C.swiglu_data(name)
    ref = C.swiglu_ref(d)
    r = C.swiglu_ratios(C.swiglu_f32(d), ref)
    bad = C.swiglu_ratios(C.swiglu_f32(d, "no_g_term"), ref)
    print(f"[swiglu {name}] restated / bar " + " ".join(f"{k} {v:.3f}" for k, v in r.items()) + f"; no_g_term dg {bad['dg']:.0f}x")
    assert max(r.values()) <= 1.0, r
    assert bad["dg"] >= 10.0


def test_glue_restatements_inside_the_bars():
    d = C.scale_data()
    assert C.ratio(C.scale_f32(d), C.scale_ref(d), C.R1) <= 1.0
    assert C.ratio(C.bf(d["x"].float() * d["cs"].float()), C.scale_ref(d), C.R1) >= 10.0  # the scalar factors forgotten
    a = C.add_data()
    assert C.ratio(C.bf(a["x"].float() + a["y"].float()), a["x"].double() + a["y"].double(), C.R1) <= 1.0
    for kind in ("one_id", "distinct"):
        ids = C.emb_bwd_ids(kind)
        dy = C.bf(O.randn("sc_embbwd_dy", (C.EMB_BWD["B"], C.EMB_BWD["S"], C.EMB_BWD["dim"])))
        ref = C.emb_bwd_ref(ids, dy)
        got = torch.zeros(C.EMB_BWD["vocab"], C.EMB_BWD["dim"])
        for t in torch.randperm(16, generator=torch.Generator().manual_seed(0)).tolist():  # fp32 adds in some other order
            got[ids.view(-1)[t]] += dy.view(16, -1)[t].float()
        assert C.ratio(got, ref["dt"], 0.0, ref["atol"]) <= 1.0
    for name in C.ROPE_CASES:
        d = C.rope_data(name)
        g = d["buf"][:, : d["S"], : d["H"] * 128].reshape(d["B"], d["S"], d["H"], 128)
        ref = C.rope_bwd_ref(g, d["table"])
        assert C.ratio(C.rope_bwd_f32(g, d["table"]), ref["dx"], C.R1, ref["atol"]) <= 1.0
        fwd = O.rope_apply(g, d["table"])  # the forward rotation instead of its transpose
        assert C.ratio(fwd, ref["dx"], C.R1, ref["atol"]) >= 10.0
    d = C.gelu_data()
    r = C.gelu_ratios(C.gelu_f32(d), C.gelu_ref(d))
    print(f"[gelu] restated / bar y {r['y']:.3f} dz {r['dz']:.3f}")
    assert max(r.values()) <= 1.0, r
    tanh = dict(y=C.bf(torch.nn.functional.gelu(d["z"].float(), approximate="tanh")), dz=C.gelu_f32(d)["dz"])  # the other GELU
    assert C.gelu_ratios(tanh, C.gelu_ref(d))["y"] >= 10.0
    for name in C.COL2IM_CASES:
        d = C.col2im_data(name)
        ref = C.col2im_ref(d)
        assert C.ratio(C.col2im_f32(d), ref["dpad"], C.R1, ref["atol"]) <= 1.0
        t = C.col2im_terms(d)
        assert C.ratio(C.bf(t[0] + t[1]), ref["dpad"], C.R1, ref["atol"]) >= 10.0  # the third tap lost


@pytest.mark.parametrize("L", C.MEL_LENGTHS)
def test_mel_clips_keep_nine_tenths_of_the_positions_strong(L):
    """The GPU comparison of the log-mel features looks only at positions above the fp32 noise floor (the existing test's `strong`
    mask): with a quarter of one of three clips silent, at most a tenth of the frame x bin positions fall outside it."""
    ref = O.mel_spectrogram(C.mel_audio(L))
    assert ref.shape == (C.MEL_B, 128, 1 + L // 160)
    strong = C.mel_strong(ref)
    share = 1.0 - strong.float().mean().item()
    print(f"[mel {L}] {share:.3f} of the positions outside the strong mask")
    assert share <= 0.1
    if L == 257:  # both reflections inside frame 1 (centred on sample 160: it reaches from -96 to 415)
        assert 160 - 256 < 0 and 160 + 255 >= L


def test_prefix_reference_and_output_bar():
    d = C.prefix_data()
    ref = C.prefix_ref(d)
    assert C.prefix_x_ratio(C.prefix_f32(d), ref) <= 1.0
    assert C.prefix_x_ratio(C.prefix_f32(d).roll(1, 1), ref) >= 10.0  # the audio tokens one frame late
    p = C.PREFIX
    assert ref["x"].shape == (p["B"], p["L2"] + p["St"], p["D"]) and ref["dw1"].shape == d["w1"].shape and ref["dw2"].shape == d["w2"].shape
    assert math.isfinite(ref["x"].abs().max().item()) and ref["db1"].abs().max() > 0 and ref["db2"].abs().max() > 0
