"""GPU: the FP8 KV cache kernels against the numpy oracle of tests/kv8_cases.py, bit for bit.

  * scatter (llx_kv_scatter_f8 / llx_kv_scatter_rows_f8): every bf16 pattern goes through q() on the device - the exhaustive check of
    the hardware conversion behind the clamp - at permuted positions; out-of-range positions write nothing.
  * dequantise (llx_kv_dequantize_f8): every code, through a strided cache.
  * epilogue relation: each of the eight weight-stream entry points run twice on the same operands, with epilogue 2 into bf16 caches
    and (picked by the wrapper from the cache dtype) epilogue 4 into uint8 caches: equal q rows, and cache bytes == q(bf16 cache)
    everywhere, unwritten bytes included.  The kernels are deterministic, so the values that reach the two epilogues are the same bits
    whatever they are; the weights span binades so that the cached values cover subnormals, normals and the clamp.
  * attention (llx_attn_decode_f8): every decode case of tests/infer_attn_cases.py, its k and v replaced by dq(q(.)) and handed over
    as codes, at that module's own bars (selection: torch.equal, census: integer equality).
  * beam move: kv_reorder_rows on a table of uint8 caches, two positions per row."""
import math

import pytest
import torch

from oracle import ref as O
from tests import infer_attn_cases as A
from tests import kv8_cases as C

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
U8 = torch.uint8
FILL = 0xA5  # sentinel byte of cache positions that must stay unwritten (only ever compared as a byte)


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


# ----------------------------------------------------------------------------------------------------------------------------- scatter
def _fused_kv(k, v, cuda):
    """k, v [B, KVH, L, 128] as the strided views of rows [B, L, (H + 2 KVH) 128] (H = 2 q heads of NaN in front), as _run_dense cuts them."""
    B, KVH, L, hd = k.shape
    H = 2
    rows = torch.full((B, L, (H + 2 * KVH) * hd), float("nan"), dtype=BF, device=cuda)
    rows[..., H * hd:(H + KVH) * hd] = k.to(cuda).transpose(1, 2).reshape(B, L, KVH * hd)
    rows[..., (H + KVH) * hd:] = v.to(cuda).transpose(1, 2).reshape(B, L, KVH * hd)
    kk = rows[..., H * hd:(H + KVH) * hd].unflatten(-1, (KVH, hd)).transpose(1, 2)
    vv = rows[..., (H + KVH) * hd:].unflatten(-1, (KVH, hd)).transpose(1, 2)
    assert kk.stride() == vv.stride() and not kk.is_contiguous()
    return kk, vv


@pytest.fixture(scope="module")
def patterns():
    """k = all 65 536 bf16 patterns as [1, 4, 128, 128], v = the same reversed, and their codes by the oracle."""
    k = C.all_bf16().view(1, 4, 128, 128)
    v = C.all_bf16().flip(0).view(1, 4, 128, 128).contiguous()
    return k, v, C.encode(k), C.encode(v)


@pytest.mark.parametrize("form", ["shared", "rows"])
def test_scatter_every_bf16_pattern(K, cuda, patterns, form):
    k, v, ck, cv = patterns
    Smax = 131
    if form == "rows":  # two sequences at their own positions
        k, v, ck, cv = (t.view(2, 2, 128, 128) for t in (k, v, ck, cv))
    B, KVH, L, _ = k.shape
    g = torch.Generator().manual_seed(11)
    pos = torch.stack([torch.randperm(L, generator=g) for _ in range(B)]) if form == "rows" else torch.randperm(L, generator=g)
    kc = torch.full((B, KVH, Smax, 128), FILL, dtype=U8, device=cuda)
    vc = torch.full((B, KVH, Smax, 128), FILL, dtype=U8, device=cuda)
    kk, vv = _fused_kv(k, v, cuda)
    K.kv_scatter(kk, vv, kc, vc, pos.to(cuda))
    for got, want, what in ((kc, ck, "k"), (vc, cv, "v")):
        got = got.cpu()
        exp = torch.full((B, KVH, Smax, 128), FILL, dtype=U8)
        for b in range(B):
            exp[b, :, pos[b] if form == "rows" else pos] = want[b]
        assert C.same_codes(got, exp), f"{what}: {int((got != exp).sum())} bytes differ from the oracle's (NaN codes modulo sign)"
    # rows at positions -1 and Smax (and beyond) write nothing; their neighbour at position 129 does
    kc.fill_(FILL), vc.fill_(FILL)
    p2 = torch.tensor([-1, Smax, 129, Smax + 7])
    p2 = p2.expand(B, 4).contiguous() if form == "rows" else p2
    K.kv_scatter(kk[:, :, :4], vv[:, :, :4], kc, vc, p2.to(cuda))
    for got, want in ((kc, ck), (vc, cv)):
        exp = torch.full((B, KVH, Smax, 128), FILL, dtype=U8)
        exp[:, :, 129] = want[:, :, 2]
        assert C.same_codes(got.cpu(), exp)


def test_scatter_refuses_mixed_caches(K, cuda):
    from llx._lib import LlxError

    k = torch.zeros(1, 1, 2, 128, dtype=BF, device=cuda)
    with pytest.raises(LlxError, match="both"):
        K.kv_scatter(k, k, torch.zeros(1, 1, 4, 128, dtype=U8, device=cuda), torch.zeros(1, 1, 4, 128, dtype=BF, device=cuda), torch.arange(2, device=cuda))


# -------------------------------------------------------------------------------------------------------------------------- dequantise
def test_dequantize_every_code_through_strides(K, cuda):
    codes = torch.arange(256, dtype=torch.int32).to(U8).repeat(16).view(2, 2, 8, 128)
    full = torch.full((2, 3, 11, 128), 0x7F, dtype=U8, device=cuda)  # NaN codes around the slice
    full[:, :2, :8] = codes.to(cuda)
    cache = full[:, :2, :8]
    assert not cache.is_contiguous()
    got = K.kv_dequantize(cache).cpu()
    want = C.decode(codes)
    nan = C.is_nan_code(codes)
    assert got.dtype is BF and got.shape == codes.shape and got.is_contiguous()
    assert torch.equal(got.float().isnan(), nan)
    assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan])  # bit for bit: the sign of -0 too


# ------------------------------------------------------------------------------------------------------------------ epilogue relation
N_Q, N_K, SMAX = 256, 128, 8
NS = (N_Q, N_K, 128)


def _weights(seed, Kd):
    """bf16 weights [n_s, Kd] whose rows span binades: the k / v values they produce cover subnormals, normals and the clamp at 448."""
    ws = []
    for i, n in enumerate(NS):
        w = O.randn(f"kv8_w{seed}_{i}_{Kd}", (n, Kd), 0.05)
        e = O.randint(f"kv8_e{seed}_{i}_{Kd}", (n, 1), -12, 11).float()
        ws.append((w * torch.exp2(e)).to(BF))
    return ws


def _int8(seed, Kd):
    ws = [O.randint(f"kv8_i{seed}_{i}_{Kd}", (n, Kd), -127, 128).to(torch.int8) for i, n in enumerate(NS)]
    sc = [(0.002 * torch.exp2(O.randint(f"kv8_is{seed}_{i}_{Kd}", (n,), -10, 12).float())).to(BF) for i, n in enumerate(NS)]
    return ws, sc


def _adapters(seed, Kd, rank=16):
    a = [O.randn(f"kv8_a{seed}_{i}_{Kd}", (rank, Kd), 0.05).to(BF) for i in range(3)]
    b = [O.randn(f"kv8_b{seed}_{i}_{Kd}", (n, rank), 0.5).to(BF) for i, n in enumerate(NS)]
    return a, b


def _dev(ts, cuda):
    return [t.to(cuda) for t in ts]


def _relation(K, cuda, stream, kind, M, Kd, norm):
    """One entry point on one set of operands, into bf16 caches (epilogue 2) and into uint8 caches (epilogue 4)."""
    batched = stream == "rows16"
    x = O.randn(f"kv8_x_{kind}_{M}_{Kd}", (M, Kd), 1.0).to(BF).to(cuda)
    nm = ((1.0 + O.randn(f"kv8_n_{Kd}", (Kd,), 0.1)).to(BF).to(cuda), 1e-5) if norm else None
    fn = K.gemm_rows16 if batched else K.gemv
    kw = {}
    if kind in ("bf16", "dora", "lora"):
        ws = _dev(_weights(1, Kd), cuda)
    elif kind == "mx4":
        pk = [K.quantize_mxfp4(w) for w in _dev(_weights(2, Kd), cuda)]
        ws, kw["mxscale"] = [p[0] for p in pk], [p[1] for p in pk]
    else:  # i8w | i8d | i8d_lora
        wi, sc = _int8(3, Kd)
        ws, kw["wscale"] = _dev(wi, cuda), _dev(sc, cuda)
        if not batched:
            kw["dynamic"] = kind != "i8w"
    if kind in ("dora", "lora", "i8d_lora"):
        a, b = _adapters(4, Kd)
        kw["lora"] = (_dev(b, cuda), fn(_dev(a, cuda), x, norm=nm), 0.5)
    if kind == "dora":
        kw["colscale"] = [(0.5 + O.randn(f"kv8_c{i}", (n,), 0.2).abs()).to(BF).to(cuda) for i, n in enumerate(NS)]
    table = O.rope_table(O.TINY._replace(max_seq_len=16))
    if batched:  # row m -> cache[m] at pos[m]; the last row is out of range and writes nothing
        rope = table[5:6].contiguous().to(cuda)
        pos = torch.tensor([(3 * m + 1) % SMAX for m in range(M)])
        pos[-1] = SMAX
        slots = M
    else:        # rows of one sequence at distinct positions, table rows 0 .. M-1
        rope = table[:M].contiguous().to(cuda)
        pos = torch.tensor([6, 0, 3, 7][:M])
        slots = 1
    pos = pos.to(cuda)
    kb = torch.full((slots, 1, SMAX, 128), -7.5, dtype=BF, device=cuda)
    vb = kb.clone()
    fill = int(C.encode(torch.tensor([-7.5], dtype=BF))[0])
    k8 = torch.full((slots, 1, SMAX, 128), fill, dtype=U8, device=cuda)
    v8 = k8.clone()
    q2 = fn(ws, x, norm=nm, epilogue=K.GV_QKV, qkv=(rope, N_Q, N_K, kb, vb, pos), **kw)
    q4 = fn(ws, x, norm=nm, epilogue=K.GV_QKV, qkv=(rope, N_Q, N_K, k8, v8, pos), **kw)
    what = f"{stream} {kind} M={M} K={Kd} norm={norm}"
    assert torch.equal(q2, q4), f"{what}: the q rows differ"
    written = 0
    for c2, c4, name in ((kb, k8, "k"), (vb, v8, "v")):
        c2, c4 = c2.cpu(), c4.cpu()
        assert not bool(c2.float().isnan().any())
        want = C.encode(c2)
        assert torch.equal(c4, want), f"{what}: {name} cache: {int((c4 != want).sum())} bytes are not q() of the bf16 cache's"
        written += int((c2 != -7.5).any(-1).sum())
    assert written == 2 * (M - 1 if batched else M), f"{what}: {written} cache rows were written"
    return kb.cpu(), vb.cpu()


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("kind", ["bf16", "dora", "i8w", "i8d", "mx4"])
def test_epilogue_relation_gemv(K, cuda, kind, norm):
    seen = []
    for M in (1, 2, 3, 4):  # (MXFP4 and weight-only int8: 3 and 4 rows are two passes)
        kb, vb = _relation(K, cuda, "gemv", kind, M, 256, norm)
        seen.append(torch.cat([kb.flatten(), vb.flatten()]).float().abs())
    a = torch.cat(seen)
    a = a[a != 7.5]
    # the operands do exercise the format: subnormal results, the clamp and ordinary values
    assert bool((a > 448).any()) and bool(((a > 0) & (a < 2.0 ** -6)).any()) and bool(((a > 1) & (a < 100)).any())


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("kind,Ks", [("bf16", (256, 512)), ("lora", (256, 512)), ("dora", (256, 512)), ("i8d", (512, 1024)), ("i8d_lora", (512, 1024))])
def test_epilogue_relation_rows16(K, cuda, kind, Ks, norm):
    """K = Ks[0]: one K slice, the epilogue runs in the main kernel (finish); K = Ks[1]: two slices, it runs in the combine launch."""
    from llx import _lib as L

    lib = L.load()
    wsb = lib.llx_gemm_rows16_i8_workspace_bytes if kind.startswith("i8") else lib.llx_gemm_rows16_workspace_bytes
    for M in (2, 16):
        assert wsb(M, sum(NS), Ks[0], 4) == 0 and wsb(M, sum(NS), Ks[1], 4) > 0
        assert wsb(M, sum(NS), Ks[1], 4) == wsb(M, sum(NS), Ks[1], 2)
        for Kd in Ks:
            _relation(K, cuda, "rows16", kind, M, Kd, norm)


# --------------------------------------------------------------------------------------------------------------------------- attention
TAIL = 19  # cache positions allocated beyond Skv


def _f8_case(cid, fam):
    """The case with k and v replaced by dq(q(.)) - what the fp8 cache holds - and the selection family's expectation through the same map."""
    d = dict(A.build(cid, fam))  # (a copy: the cached case stays as it is)
    d["k8"], d["v8"] = C.encode(d["k"]), C.encode(d["v"])
    d["k"], d["v"] = C.decode(d["k8"]), C.decode(d["v8"])
    if fam == "sel":
        d["want"] = C.roundtrip(d["want"])
        # the codes survive the format: q . k over the 14 code dims is what it was
        assert torch.equal(d["k"][..., :A.CODE_BITS], A.build(cid, fam)["k"][..., :A.CODE_BITS])
    else:
        assert torch.equal(d["v"], A.build(cid, fam)["v"]) and float(d["k"].float().abs().max()) == 448.0  # one-hot V exact, garbage clamped
    return d


def _cache8(t, cuda):
    """codes [B, KVH, Skv, 128] as the slice of an allocation TAIL positions longer, NaN codes beyond the slice."""
    B, KVH, S, hd = t.shape
    full = torch.full((B, KVH, S + TAIL, hd), 0x7F, dtype=U8, device=cuda)
    full[:, :, :S] = t.to(cuda)
    return full[:, :, :S]


def _fused_q(d, cuda):
    c = d["case"]
    rows = torch.full((c.B, c.M, (c.H + 2 * c.KVH) * A.HD), float("nan"), dtype=BF, device=cuda)
    rows[..., :c.H * A.HD] = d["q"].to(cuda).transpose(1, 2).reshape(c.B, c.M, c.H * A.HD)
    return rows[..., :c.H * A.HD].view(c.B, c.M, c.H, A.HD).transpose(1, 2)


def _out(c, cuda):
    big = torch.full((c.B, c.M + 2, c.H * A.HD + 256), A.SENTINEL, dtype=BF, device=cuda)
    return big, big[:, 1:c.M + 1, A.HD:A.HD + c.H * A.HD]


def _result(c, big, out):
    rest = big.clone()
    rest[:, 1:c.M + 1, A.HD:A.HD + c.H * A.HD] = A.SENTINEL
    assert bool((rest == A.SENTINEL).all()), f"{c.id}: bytes outside out= were written"
    return out.reshape(c.B, c.M, c.H, A.HD).transpose(1, 2).contiguous().cpu()


def _decode(K, d, cuda, use_ext, entry):
    """Through the wrapper, or (entry) through llx_attn_decode_f8 itself with a workspace of its own and the case's nsplit (the wrapper's
    where the case fixes none)."""
    from llx import _lib as L

    c = d["case"]
    q, kc, vc, mask = _fused_q(d, cuda), _cache8(d["k8"], cuda), _cache8(d["v8"], cuda), d["mask"].to(cuda)
    ext = torch.tensor([d["ext"]], dtype=torch.int32, device=cuda) if use_ext else None
    big, out = _out(c, cuda)
    if not entry:
        ret = K.attn_decode(q, kc, vc, mask, extent=ext, out=out)
        assert ret.data_ptr() == out.data_ptr()
        return _result(c, big, out)
    m, m_sb, m_sh = K._mask_norm(mask, c.B, c.M, c.Skv, c.H)
    lib = L.load()
    nsplit = c.nsplit or K._decode_nsplit(c.B, c.KVH, c.Skv)
    ws = torch.full((lib.llx_attn_decode_workspace_bytes(c.B, c.H, c.M, nsplit) // 4,), float("nan"), device=cuda)
    o4 = out.view(c.B, c.M, c.H, A.HD)
    L.check(lib.llx_attn_decode_f8(L.ptr(q), q.stride(0), q.stride(1), q.stride(2), L.ptr(kc), L.ptr(vc), kc.stride(0), kc.stride(1), kc.stride(2), L.ptr(out),
                                   o4.stride(0), o4.stride(2), o4.stride(1), L.ptr(m), m_sb, m_sh, m.stride(2), L.ptr(ext), L.ptr(ws), c.B, c.H, c.KVH, c.M,
                                   c.Skv, nsplit, A.HD, 1.0 / math.sqrt(A.HD), L.stream()), "llx_attn_decode_f8")
    return _result(c, big, out)


@pytest.mark.parametrize("cid", [c.id for c in A.cases_of("decode")])
def test_attn_decode_f8_exact(K, cuda, cid):
    for fam in A.FAMILIES:
        d = _f8_case(cid, fam)
        for use_ext in (True, False):
            for entry in (False, True):
                o = _decode(K, d, cuda, use_ext, entry)
                assert o.shape == d["q"].shape and o.dtype is BF
                assert A.family_ok(o, d), f"{cid} {fam} extent {'on the device' if use_ext else 'None'}, {'C entry' if entry else 'wrapper'}"


def test_attn_decode_f8_equals_bf16_kernel_on_the_image(K, cuda):
    """Random codes (NaN codes excluded), every ROWS class: the f8 kernel and the bf16 kernel on the dequantised image give the same bits."""
    g = torch.Generator().manual_seed(5)
    for G, M in ((4, 1), (4, 2), (8, 2)):
        B, KVH, S = 2, 2, 300
        codes = torch.randint(0, 256, (2, B, KVH, S, 128), generator=g, dtype=torch.int32)
        codes = torch.where((codes & 0x7F) == 0x7F, codes & 0x80, codes).to(U8).to(cuda)
        kc, vc = codes[0], codes[1]
        q = (torch.randn(B, G * KVH, M, 128, generator=g) * 0.1).to(BF).to(cuda)
        mask = (torch.rand(B, 1, M, S, generator=g) < 0.7).to(cuda)
        mask[..., 0] = True
        o8 = K.attn_decode(q, kc, vc, mask)
        o16 = K.attn_decode(q, K.kv_dequantize(kc), K.kv_dequantize(vc), mask)
        assert torch.equal(o8.view(torch.int16), o16.view(torch.int16)), (G, M)


# --------------------------------------------------------------------------------------------------------------------------- beam move
@pytest.mark.parametrize("length", [5, 6])
def test_beam_move_two_positions_per_row(K, cuda, length):
    g = torch.Generator().manual_seed(length)
    B, KVH, Smax, W = 4, 2, 12, 3
    caches = [torch.randint(0, 256, (B, KVH, Smax, 128), generator=g, dtype=torch.int32).to(U8).to(cuda) for _ in range(4)]
    before = [c.clone() for c in caches]
    table = K.kv_cache_table(caches)
    parent = [2, 1, 0]  # slot 1 keeps its rows
    K.kv_reorder_rows(table, torch.tensor(parent, dtype=torch.int32, device=cuda), length)
    moved = 2 * ((length + 1) // 2)
    for c, old in zip(caches, before):
        for b in range(W):
            assert torch.equal(c[b, :, :length], old[parent[b], :, :length]), f"slot {b} below len"
            assert torch.equal(c[b, :, moved:], old[b, :, moved:]), f"slot {b} at or above {moved}"
        assert torch.equal(c[W:], old[W:]), "slots >= W"


def test_cache_table_refusals(K, cuda):
    from llx._lib import LlxError

    with pytest.raises(LlxError, match="even Smax"):
        K.kv_cache_table([torch.zeros(2, 1, 7, 128, dtype=U8, device=cuda)])
    with pytest.raises(LlxError):
        K.kv_cache_table([torch.zeros(2, 1, 8, 128, dtype=U8, device=cuda), torch.zeros(2, 1, 8, 128, dtype=BF, device=cuda)])
