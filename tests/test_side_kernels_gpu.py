"""The memory-bound side kernels against float64 on the GPU: RMSNorm, cross-entropy, the element-wise glue and the audio glue at every
dispatch class, guard, tail and stride tests/side_cases.py names (tests/test_side_cases.py shows on the CPU that each case reaches its
class, that the bars below are reachable and that they catch a wrong divisor, a dropped chunk, a lost wave, an early add).

Every bar is the derived one of side_cases.py - k bf16 roundings plus the stated atol - except cross-entropy, which keeps the bars of
test_kernels_gpu.py::test_cross_entropy, and the AudioPrefixFn gradients, which keep the 6 % of the audio model test.  Each test prints
its worst error / bound, so that a rewrite of a kernel can see how much room the old one left."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref as O  # noqa: E402
from tests import side_cases as C  # noqa: E402
from tests.util import _close  # noqa: E402

SENTINEL = 3.0  # exact in bf16 and int8; never a value a kernel under test writes next to it


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


def _check(tag, ratios):
    print(f"[side {tag}] error / bound " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (tag, ratios)


def _worst(into, ratios):
    for k, v in ratios.items():
        if k not in into or not v <= into[k]:  # a NaN sticks
            into[k] = v


def _same_bits(a, b):
    """Two fp32 scalars with the same bits (NaN included)."""
    return torch.equal(a.reshape(1).view(torch.int32), b.reshape(1).view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------ RMSNorm
@pytest.mark.parametrize("dim", list(C.RMS_DIMS))
def test_rmsnorm_fwd(K, cuda, dim):
    """y (one rounding) and rstd (2^-20) against float64; the quantising variant returns the same y / rstd bits and q, qscale
    bit-identical to quantize_int8_rowwise of the kernel's own y."""
    worst = {}
    for rows in C.RMS_FWD_ROWS:
        d = C.rms_data(dim, rows)
        ref = C.rms_ref(d)
        x, w = d["x"].to(cuda), d["w"].to(cuda)
        y, rstd = K.rmsnorm_fwd(x, w, C.EPS)
        y1, r1, q1, s1 = K.rmsnorm_fwd(x, w, C.EPS, quant=True)
        assert torch.equal(y, y1) and torch.equal(rstd, r1)
        q0, s0 = O.quantize_int8_rowwise(y.cpu())
        assert torch.equal(q1.cpu(), q0) and torch.equal(s1.cpu(), s0)
        _worst(worst, {"y": C.ratio(y, ref["y"], C.R1), "rstd": C.ratio(rstd, ref["rstd"], 2.0 ** -20)})
    _check(f"rmsnorm_fwd {dim}", worst)


@pytest.mark.parametrize("dim", [8, 1792, 3072, 4096, 8184])
def test_rmsnorm_fwd_quant_row_stride(cuda, dim):
    """int8 rows wider than dim (ldq > dim, reachable through the C entry point only): the bytes beyond dim stay untouched."""
    from llx import _lib as L

    rows, ldq = 5, dim + 64
    d = C.rms_data(dim, rows)
    x, w = d["x"].to(cuda), d["w"].to(cuda)
    y = torch.empty_like(x)
    rstd = torch.empty(rows, device=cuda, dtype=torch.float32)
    q = torch.full((rows, ldq), int(SENTINEL), device=cuda, dtype=torch.int8)
    qs = torch.empty(rows, device=cuda, dtype=torch.bfloat16)
    L.check(L.load().llx_rmsnorm_fwd_quant(L.ptr(x), L.ptr(w), L.ptr(y), L.ptr(rstd), L.ptr(q), ldq, L.ptr(qs), rows, dim, C.EPS, L.stream()),
            "llx_rmsnorm_fwd_quant")
    q0, s0 = O.quantize_int8_rowwise(y.cpu())
    assert torch.equal(q[:, :dim].cpu(), q0) and torch.equal(qs.cpu(), s0)
    assert (q[:, dim:] == int(SENTINEL)).all()
    assert C.ratio(y, C.rms_ref(d)["y"], C.R1) <= 1.0


@pytest.mark.parametrize("dim", list(C.RMS_DIMS))
def test_rmsnorm_bwd(K, cuda, dim):
    """dx and dw against float64 at the derived bars, for every row count of the dim (a wave with 0 .. 4 rows, a second, ragged block);
    dx with dres = bf16(bf16(dx) + dres) bit for bit; dx identical with and without dw, dw identical with and without dres."""
    worst = {}
    for rows in C.RMS_BWD_ROWS[dim]:
        d = C.rms_data(dim, rows)
        ref = C.rms_ref(d)
        x, w, dy, dres = (d[k].to(cuda) for k in ("x", "w", "dy", "dres"))
        y, rstd = K.rmsnorm_fwd(x, w, C.EPS)
        dx0, dw0 = K.rmsnorm_bwd(dy, x, w, rstd, True)
        dx1, dw1 = K.rmsnorm_bwd(dy, x, w, rstd, True, dres)
        dx2, none2 = K.rmsnorm_bwd(dy, x, w, rstd, False)
        dx3, none3 = K.rmsnorm_bwd(dy, x, w, rstd, False, dres)
        assert none2 is None and none3 is None
        assert torch.equal(dx2, dx0) and torch.equal(dx3, dx1), f"rows {rows}: dx depends on whether dw is requested"
        assert torch.equal(dw0, dw1), f"rows {rows}: dw depends on dres"
        r = C.rms_ratios(dict(y=y, rstd=rstd, dx=dx0, dx_res=dx1, dw=dw0), d, ref)
        assert r["join"] == 0.0, f"rows {rows}: dx with dres is not bf16(bf16(dx) + dres)"
        _worst(worst, r)
    _check(f"rmsnorm_bwd {dim}", worst)


# ------------------------------------------------------------------------------------------------------------------ cross-entropy
def _ce_run(K, buf, labels):
    """(loss, grad in place, loss of the write_grad=False call) - the latter must leave the logits alone."""
    keep = buf.clone()
    loss0, none = K.ce_fwd_bwd(buf, labels, False)
    assert none is None and torch.equal(buf, keep), "write_grad=False touched the logits"
    loss, dl = K.ce_fwd_bwd(buf, labels, True)
    assert _same_bits(loss0, loss), "the loss depends on write_grad"
    return loss, dl


@pytest.mark.parametrize("name", list(C.CE_CASES))
def test_cross_entropy(K, cuda, name):
    d = C.ce_data(C.CE_CASES[name])
    ref = C.ce_ref(d["logits"], d["labels"])
    loss, dl = _ce_run(K, d["logits"].to(cuda).clone(), d["labels"].to(cuda))
    if C.CE_CASES[name].kind == "all_ignored":
        assert torch.isnan(loss).item() and (dl == 0).all()
    _check(f"ce {name}", C.ce_ratios(dict(loss=loss, grad=dl), ref))


def test_cross_entropy_strided_rows(K, cuda):
    """Logits as a [T, V] column view of a [T, V + 64] buffer: the 64 columns behind every row keep their bits, loss and gradient equal
    the dense call's bit for bit."""
    case = C.CE_CASES[C.CE_STRIDED]
    d = C.ce_data(case)
    labels = d["labels"].to(cuda)
    loss_d, dl_d = _ce_run(K, d["logits"].to(cuda).clone(), labels)
    wide = torch.full((case.T, case.V + 64), SENTINEL, device=cuda, dtype=torch.bfloat16)
    wide[:, : case.V] = d["logits"].to(cuda)
    loss_s, dl_s = _ce_run(K, wide[:, : case.V], labels)
    assert dl_s.data_ptr() == wide.data_ptr() and dl_s.stride(0) == case.V + 64
    assert (wide[:, case.V:] == SENTINEL).all()
    assert torch.equal(wide[:, : case.V], dl_d) and _same_bits(loss_s, loss_d)


@pytest.mark.parametrize("count", C.CE_CHUNK["counts"])
def test_ce_chunk(K, cuda, count):
    """ce_chunk over 700 rows in chunks of 256, with and without a compacted row count: loss and gradients bit-identical to ONE
    ce_fwd_bwd call over the same rows (and so inside the bars against float64); rows from the end of the last labelled row's 256-row
    tile on keep their logits and book zero loss."""
    T, V, chunk = C.CE_CHUNK["T"], C.CE_CHUNK["V"], C.CE_CHUNK["chunk"]
    d = C.ce_chunk_data(count)
    labels = d["labels"].to(cuda)
    rows = None if count is None else torch.tensor([count], device=cuda, dtype=torch.int32)
    one = d["logits"].to(cuda).clone()
    loss1, _ = K.ce_fwd_bwd(one, labels, True, rows=rows)
    parts = d["logits"].to(cuda).clone()
    ws = torch.full((T + 2,), float("nan"), device=cuda, dtype=torch.float32)
    loss = torch.full((), float("nan"), device=cuda, dtype=torch.float32)
    for r0 in range(0, T, chunk):
        n = min(chunk, T - r0)
        K.ce_chunk(parts[r0 : r0 + n], labels, ws, loss, r0, True, rows, first=r0 == 0, last=r0 + n == T)
    assert _same_bits(loss, loss1) and torch.equal(parts, one)
    limit = T if count is None else min(T, C.ce_rows_limit(count))
    assert torch.equal(parts[limit:].cpu(), d["logits"][limit:]) and (ws[2 + limit:] == 0).all() and not torch.isnan(ws).any()
    ref = C.ce_ref(d["logits"], d["labels"])
    _check(f"ce_chunk {count}", C.ce_ratios(dict(loss=loss, grad=parts[:limit]), dict(loss=ref["loss"], grad=ref["grad"][:limit])))


# -------------------------------------------------------------------------------------------------------------------- element-wise
@pytest.mark.parametrize("dim", list(C.EMB_DIMS))
def test_embedding_fwd(K, cuda, dim):
    table = C.bf(O.randn(f"sc_emb_t{dim}", (24, dim)))
    ids = O.randint(f"sc_emb_ids{dim}", (2, 5), 0, 24)
    want = torch.nn.functional.embedding(ids, table)
    assert torch.equal(K.embedding_fwd(ids.to(cuda), table.to(cuda)).cpu(), want)
    buf = torch.full((2, 10, dim), SENTINEL, device=cuda, dtype=torch.bfloat16)  # rows 3 .. 7 of each batch are the destination
    K.embedding_fwd(ids.to(cuda), table.to(cuda), out=buf[:, 3:8])
    assert torch.equal(buf[:, 3:8].cpu(), want)
    assert (buf[:, :3] == SENTINEL).all() and (buf[:, 8:] == SENTINEL).all()  # in front of, between and behind the batches


@pytest.mark.parametrize("kind", ["one_id", "distinct"])
def test_embedding_bwd(K, cuda, kind):
    p = C.EMB_BWD
    ids = C.emb_bwd_ids(kind)
    dy = C.bf(O.randn("sc_embbwd_dy", (p["B"], p["S"], p["dim"])))
    ref = C.emb_bwd_ref(ids, dy)
    dt = K.embedding_bwd(ids.to(cuda), dy.to(cuda), p["vocab"])
    wide = torch.full((p["B"], 3 + p["S"], p["dim"]), SENTINEL, device=cuda, dtype=torch.bfloat16)  # dy behind a 3-row prefix
    wide[:, 3:] = dy.to(cuda)
    dt_s = K.embedding_bwd(ids.to(cuda), wide[:, 3:], p["vocab"])
    _check(f"embedding_bwd {kind}", {"dense": C.ratio(dt, ref["dt"], 0.0, ref["atol"]), "strided": C.ratio(dt_s, ref["dt"], 0.0, ref["atol"])})


@pytest.mark.parametrize("name", list(C.ROPE_CASES))
def test_rope(K, cuda, name):
    """Forward bit-exact against O.rope_apply, backward against float64 with one rounding; everything outside the first nheads heads of
    the first S rows of every batch (wider rows, a batch stride larger than S rows) keeps its bits."""
    d = C.rope_data(name)
    B, S, H = d["B"], d["S"], d["H"]
    buf, table = d["buf"], d["table"]
    inner = buf[:, :S, : H * 128].reshape(B, S, H, 128)
    whole = buf.to(cuda).clone()
    K.rope_(whole[:, :S], table.to(cuda), H)
    want = buf.clone()
    want[:, :S, : H * 128] = O.rope_apply(inner, table).reshape(B, S, H * 128)
    assert torch.equal(whole.cpu(), want)
    whole = buf.to(cuda).clone()
    K.rope_(whole[:, :S], table.to(cuda), H, backward=True)
    got = whole.cpu()
    ref = C.rope_bwd_ref(inner, table)
    _check(f"rope_bwd {name}", {"dx": C.ratio(got[:, :S, : H * 128].reshape(B, S, H, 128), ref["dx"], C.R1, ref["atol"])})
    got[:, :S, : H * 128] = buf[:, :S, : H * 128]
    assert torch.equal(got, buf)


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("name", list(C.SWIGLU_SHAPES))
def test_swiglu(K, cuda, name, strided):
    """h, dg, du against float64 (two roundings each); strided: gate | up and dg | du are the halves of one buffer."""
    d = C.swiglu_data(name)
    ref = C.swiglu_ref(d)
    rows, cols = d["g"].shape
    dh = d["dh"].to(cuda)
    if strided:
        gu = torch.cat([d["g"], d["u"]], 1).to(cuda)
        g, u = gu[:, :cols], gu[:, cols:]
        dgu = torch.empty(rows, 2 * cols, device=cuda, dtype=torch.bfloat16)
        dg, du = dgu[:, :cols], dgu[:, cols:]
    else:
        g, u = d["g"].to(cuda), d["u"].to(cuda)
        dg, du = torch.empty_like(g), torch.empty_like(g)
    h = K.swiglu_fwd(g, u)
    K.swiglu_bwd(dh, g, u, dg, du)
    _check(f"swiglu {name}{' strided' if strided else ''}", C.swiglu_ratios(dict(h=h, dg=dg, du=du), ref))


def test_scale(K, cuda):
    """Device scalar, host scale and column scale together (one rounding); a strided destination; the destination aliasing the source."""
    d = C.scale_data()
    ref = C.scale_ref(d)
    r, c = C.SCALE_SHAPE
    x, cs = d["x"].to(cuda), d["cs"].to(cuda)
    kw = dict(dev_scalar=torch.tensor([C.SCALE_DEV], device=cuda), host_scale=C.SCALE_HOST, colscale=cs)
    y = K.scale(x, **kw)
    wide = torch.full((r, c + 16), SENTINEL, device=cuda, dtype=torch.bfloat16)
    K.scale(x, out=wide[:, 8 : 8 + c], **kw)
    assert torch.equal(wide[:, 8 : 8 + c], y) and (wide[:, :8] == SENTINEL).all() and (wide[:, 8 + c:] == SENTINEL).all()
    xa = x.clone()
    K.scale(xa, out=xa, **kw)
    assert torch.equal(xa, y)
    _check("scale", {"y": C.ratio(y, ref, C.R1)})


def test_add(K, cuda):
    a = C.add_data()
    r, c = C.ADD_SHAPE
    x, y = a["x"].to(cuda), a["y"].to(cuda)
    z = K.add(x, y)
    wide = torch.full((r, c + 16), SENTINEL, device=cuda, dtype=torch.bfloat16)
    K.add(x, y, out=wide[:, 8 : 8 + c])
    assert torch.equal(wide[:, 8 : 8 + c], z) and (wide[:, :8] == SENTINEL).all() and (wide[:, 8 + c:] == SENTINEL).all()
    _check("add", {"z": C.ratio(z, a["x"].double() + a["y"].double(), C.R1)})


def test_transpose_and_widen_remaining_classes(K, cuda):
    """What test_transpose_and_widen leaves out: a matrix inside one 64 x 64 tile, whole tiles only, a strided source with a padded
    destination; the scalar tail of i8_to_bf16 (n = 1 .. 17 around its 8-element vector path)."""
    for R, Cc in ((5, 7), (64, 128)):
        x = C.bf(O.randn(f"sc_tr_{R}", (R, Cc)))
        assert torch.equal(K.transpose(x.to(cuda)).cpu(), x.T.contiguous())
        q = O.randint(f"sc_tr_q{R}", (R, Cc), -127, 128).to(torch.int8)
        assert torch.equal(K.transpose(q.to(cuda)).cpu(), q.T.contiguous().to(torch.bfloat16))
    wide = C.bf(O.randn("sc_tr_wide", (13, 100)))
    out = K.transpose(wide.to(cuda)[:, 10:87], pad_to=8).cpu()  # [77, 16]
    assert out.shape == (77, 16) and torch.equal(out[:, :13], wide[:, 10:87].T) and (out[:, 13:] == 0).all()
    for n in range(1, 18):
        q = O.randint(f"sc_widen_{n}", (n,), -128, 128).to(torch.int8)
        assert torch.equal(K.i8_to_bf16(q.to(cuda)).cpu(), q.to(torch.bfloat16)), n


# --------------------------------------------------------------------------------------------------------------------- audio glue
def test_gelu(cuda):
    """GELU (exact erf) forward and backward over z in [-6, 6] against float64; source and destination rows of wider buffers."""
    from llx import audio_ops as A

    d = C.gelu_data()
    ref = C.gelu_ref(d)
    r, c = C.GELU_SHAPE

    def wide(t):
        buf = torch.full((r, C.GELU_LD), SENTINEL, device=cuda, dtype=torch.bfloat16)
        buf[:, 8 : 8 + c] = t.to(cuda)
        return buf

    zb, dyb, yb = wide(d["z"]), wide(d["dy"]), wide(torch.zeros(r, c))
    A._gelu_fwd(zb[:, 8 : 8 + c], yb[:, 8 : 8 + c])
    assert (yb[:, :8] == SENTINEL).all() and (yb[:, 8 + c:] == SENTINEL).all()
    dz = A._gelu_bwd(dyb[:, 8 : 8 + c], zb[:, 8 : 8 + c])
    _check("gelu", C.gelu_ratios(dict(y=yb[:, 8 : 8 + c], dz=dz), ref))


@pytest.mark.parametrize("name", list(C.COL2IM_CASES))
def test_col2im3(cuda, name):
    from llx import audio_ops as A

    d = C.col2im_data(name)
    ref = C.col2im_ref(d)
    got = A._col2im3(d["dA"].to(cuda), d["C"], d["P"], d["stride"])
    _check(f"col2im3 {name}", {"dpad": C.ratio(got, ref["dpad"], C.R1, ref["atol"])})


def test_conv_w_reorder(cuda):
    from llx import audio_ops as A

    D, Cc = C.REORDER_SHAPE
    w = C.bf(O.randn("sc_reorder", (D, Cc, 3)))
    g = A._reorder(w.to(cuda), True)
    assert torch.equal(g.cpu(), w.permute(0, 2, 1).reshape(D, 3 * Cc))
    back = A._reorder(g, False)
    assert torch.equal(back.cpu(), w)
    wg = C.bf(O.randn("sc_reorder_g", (D, 3 * Cc)))
    assert torch.equal(A._reorder(wg.to(cuda), False).cpu(), wg.view(D, 3, Cc).permute(0, 2, 1).contiguous())


@pytest.mark.parametrize("L", C.MEL_LENGTHS)
def test_mel_and_log_mel(cuda, L):
    """Mel power and log-mel / CMN features of three clips at the shortest length, a length off the hop grid and one on it, at the bars
    of test_model_gpu.py::test_mel_spectrogram_kernel."""
    from llx.audio_ops import MelSpectrogram, logmel_cmn_padded

    audio = C.mel_audio(L)
    ref = O.mel_spectrogram(audio)
    mel = MelSpectrogram().to(cuda)(audio.to(cuda))
    F = 1 + L // 160
    assert mel.shape == ref.shape == (C.MEL_B, 128, F)
    torch.testing.assert_close(mel.cpu(), ref, atol=1e-4 * ref.abs().max().item(), rtol=1e-3)
    feat = logmel_cmn_padded(mel).cpu().float()
    rf = O.log_mel_cmn(ref).transpose(1, 2)
    assert feat.shape == (C.MEL_B, F + 1, 128) and feat[:, 0].abs().sum() == 0 and feat[:, -1].abs().sum() == 0
    strong = C.mel_strong(ref)
    assert strong.float().mean() >= 0.9
    err = (feat[:, 1:-1] - rf).abs()[strong].max().item()
    print(f"[side mel {L}] log-mel error {err:.4f} (bar 0.07)")
    assert err < 0.07


def test_audio_prefix_fn_batch_of_two_odd_frames(cuda):
    """AudioPrefixFn at B = 2 with an odd number of feature frames (L1 101 -> L2 51; D 64, C 128) against the float64 conv stack.
    The parameter gradients, summed over the batch, keep the 6 % max-norm bar of test_audio_model_loss_and_conv_grads (the path crosses
    three GEMMs: the bar is kept, not derived).  The output's audio rows went through four bf16 roundings (z1, h1, z2, x), each at most
    2^-8 of a value no larger than the largest on the path, carried on by GELU (slope <= 1.13) and a convolution of unit gain (w2 is
    drawn at std 1 / sqrt(3 D)): |err| <= 4 R1 max|ref|.  The token rows are a gather: bit-exact."""
    from llx.audio_ops import AudioPrefixFn

    d = C.prefix_data()
    ref = C.prefix_ref(d)
    L2 = C.PREFIX["L2"]
    ps = {k: d[k].to(cuda).requires_grad_() for k in ("w1", "b1", "w2", "b2")}
    x = AudioPrefixFn.apply(d["feat"].to(cuda), d["tokens"].to(cuda), d["emb"].to(cuda), ps["w1"], ps["b1"], ps["w2"], ps["b2"])
    x.backward(d["dx"].to(cuda))
    xc = x.detach().float().cpu()
    assert torch.equal(xc[:, L2:].double(), ref["x"][:, L2:])
    r = {"x": C.prefix_x_ratio(xc[:, :L2], ref)}
    for k, q in ps.items():
        g, want = q.grad.float().cpu(), ref["d" + k].float()
        r["d" + k] = (g - want).abs().max().item() / (0.06 * want.abs().max().item() + 1e-6)
        _close(g, want, 0.06, k)
    _check("audio_prefix", r)
