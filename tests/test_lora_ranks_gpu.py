"""GPU: LoRA and DoRA at every rank class the group planner and the skinny kernels distinguish (tests/lora_cases.py).

a. one linear group (q|k|v, gate|up) driven the way the transformer blocks drive llx.ops.GroupPlan, against the float64 ground truth
   at the GEMM bar (2^-7 of max|ref| + 2^-7 relative), with per-rank row cosines, first / last rank probes, the operand images of the
   fused plans, the column-slice and in-place-accumulation contracts of the per-member plans, and a bit-identical second run;
b. the same comparison on an int8 base (weight-only, dynamic) and for DoRA;
c. a whole TransformerLayer at lora_cases.MID against O.layer with the bars of test_full_dimension_layer_parity: the stand-alone
   RoPE / SwiGLU after an unfused group, the residual and the norm joins.
Every test prints its worst error next to its bar."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref as O  # noqa: E402
from tests import lora_cases as C  # noqa: E402
from tests.util import _rows_close, layer_parity  # noqa: E402

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def K(cuda):
    from llx import kernels

    return kernels


def _drive(K, cuda, d, mods, need_grads=True):
    """forward + backward of one group as AttnBlockFn / MLPBlockFn run them: out is a column slice of a wider buffer, the data gradient
    goes to a caller-owned buffer, the second stages of the adapter-gradient products are flushed at the end."""
    from llx.ops import GroupPlan

    plan = GroupPlan(mods)
    M, N = d["x"].shape[0], sum(d["Ns"])
    x, dy = d["x"].to(BF16).to(cuda), d["dy"].to(BF16).to(cuda)
    wide = torch.full((M, N + 256), 7.0, device=cuda, dtype=BF16)
    y, saved = plan.forward(x, wide[:, 128 : 128 + N])
    assert y.data_ptr() == wide[:, 128:].data_ptr()
    assert bool((wide[:, :128] == 7).all()) and bool((wide[:, 128 + N :] == 7).all()), "columns outside the out view were written"
    if not need_grads:
        return plan, y, saved, None, None
    needs = [t.requires_grad for t in plan.tensors()]
    pend = []
    dx_out = torch.full((M, d["K"]), float("nan"), device=cuda, dtype=BF16)  # whatever is read before it is written would show
    dx, grads = plan.backward(dy, x, saved, needs, need_dx=True, dx_out=dx_out, pending=pend)
    K.skinny_tn_flush(pend)
    assert dx.data_ptr() == dx_out.data_ptr()
    by_id = {id(t): g for t, g in zip(plan.tensors(), grads)}
    g = dict(dA=[by_id[id(m.lora_a)] if m.rank else None for m in plan.members], dB=[by_id[id(m.lora_b)] if m.rank else None for m in plan.members],
             dm=[by_id[id(m.dora_m)] if m.dora_m is not None else None for m in plan.members])
    for t, gr in zip(plan.tensors(), grads):
        assert (gr is not None) == t.requires_grad
    return plan, y, saved, dx, g


def _cuda_mods(d, cuda, **kw):
    return [m.to(cuda) for m in C.group_modules(d, **kw)]


def _check_bar(got, ref, what, worst):
    e = C.over_bar(got.float().cpu(), ref)
    worst[what] = max(worst.get(what, 0.0), e)
    assert e <= 1.0, f"{what}: {e:.2f}x the GEMM bar (2^-7 max|ref| + 2^-7 |ref|)"


@pytest.mark.parametrize("which", ["qkv", "gu"])
@pytest.mark.parametrize("name", list(C.CASES))
def test_group_against_float64(K, cuda, name, which):
    from llx.ops import weight_t

    case = C.CASES[name]
    want = case.mid[0] if which == "qkv" else case.mid[1]
    d = C.group_data(case, C.MID, which)
    ref = C.group_math(d)
    plan, y, saved, dx, g = _drive(K, cuda, d, _cuda_mods(d, cuda))
    assert plan.fused == want.fused and plan.R == want.R
    worst = {}
    _check_bar(y, ref["y"], "y", worst)
    _check_bar(dx, ref["dx"], "dx", worst)
    for i, (ga, gb) in enumerate(zip(g["dA"], g["dB"])):
        if ref["dA"][i] is None:
            assert ga is None and gb is None
            continue
        assert ga.shape == ref["dA"][i].shape and gb.shape == ref["dB"][i].shape
        _check_bar(ga, ref["dA"][i], "dA", worst)
        _check_bar(gb, ref["dB"][i], "dB", worst)
        # per rank: a dropped or duplicated rank shows here however small its share
        _rows_close(ga.float().cpu(), ref["dA"][i], f"dA_{i} rows", min_cos=0.999)
        _rows_close(gb.float().cpu().T, ref["dB"][i].T, f"dB_{i}^T rows", min_cos=0.999)
    print(f"[{name} {which}] {'fused' if plan.fused else 'per member'} R {plan.R}: worst / bar " + " ".join(f"{k} {v:.2f}" for k, v in worst.items()))

    x, dy = d["x"].to(BF16).to(cuda), d["dy"].to(BF16).to(cuda)
    As = [a.to(BF16).to(cuda) for a in d["A"] if a is not None]
    if plan.fused:  # the operand images riding in `saved` equal their torch construction bit for bit
        t, bT, a2t = saved
        R, N = plan.R, plan.N
        a_cat = torch.cat(As, 0)
        want_bT = torch.zeros(R, N, device=cuda, dtype=BF16)
        no = ro = 0
        for b, n in zip(d["B"], d["Ns"]):
            want_bT[ro : ro + b.shape[1], no : no + n] = b.to(BF16).to(cuda).T
            no, ro = no + n, ro + b.shape[1]
        want_a2t = torch.zeros(d["K"], 64, device=cuda, dtype=BF16)
        want_a2t[:, :R] = (a_cat.float() * C.SCALE).to(BF16).T
        assert torch.equal(bT, want_bT) and torch.equal(a2t, want_a2t)
        assert t.shape == (x.shape[0], 64) and bool((t[:, R:] == 0).all()) and torch.equal(t, K.skinny_nt(x, a_cat))
    else:
        # the in-place accumulation (output and residual of the GEMM aliased) equals, bit for bit, the first member's product followed
        # by residual-epilogue launches into SEPARATE buffers
        acc, off = None, 0
        for i, (w, a, b, s, n) in enumerate(zip(d["W"], d["A"], d["B"], d["s"], d["Ns"])):
            dyi = dy[:, off : off + n]
            off += n
            kw = {}
            if a is not None:
                a_, b_ = a.to(BF16).to(cuda), b.to(BF16).to(cuda)
                kw = dict(a2=K.skinny_nt(dyi, K.transpose(b_)), b2=K.pad64(a_, s, transposed=True))
            wt = weight_t(plan.members[i].weight)
            acc = K.gemm_nt(dyi, wt, **kw) if acc is None else K.gemm_nt(dyi, wt, epilogue=K.EPI_RESIDUAL, e=acc, **kw)
        assert torch.equal(dx, acc), "in-place dx accumulation differs from the out-of-place sum"

    # second run, fresh plan: bit-identical
    _, y2, _, dx2, g2 = _drive(K, cuda, d, _cuda_mods(d, cuda))
    assert torch.equal(y2, y) and torch.equal(dx2, dx)
    for k in ("dA", "dB"):
        for a, b in zip(g[k], g2[k]):
            assert (a is None and b is None) or torch.equal(a, b), k


@pytest.mark.parametrize("name", list(C.CASES))
def test_first_and_last_rank_probes(K, cuda, name):
    """B zero except rank column c of every member, c = 0 and c = r - 1: y - base = s bf16(t[:, c]) B[:, c]^T.  A clamp or member-offset
    error is localised to one column (tests/test_lora_cases.py: the neighbouring column lands 10x outside this bar)."""
    case = C.CASES[name]
    d = C.group_data(case, C.MID, "qkv")
    x = d["x"].double()
    base = x @ torch.cat(d["W"]).double().T
    for label, c_of in (("first", lambda r: 0), ("last", lambda r: r - 1)):
        B = C.probe_B(d, c_of)
        _, y, _, _, _ = _drive(K, cuda, d, _cuda_mods(d, cuda, B=B), need_grads=False)
        add = []
        for a, b, s in zip(d["A"], B, d["s"]):
            if a is None:
                add.append(torch.zeros(x.shape[0], 0, dtype=torch.float64))
                continue
            c = c_of(a.shape[0])
            t_c = (x @ a[c].double()).to(BF16).double()
            add.append(s * torch.outer(t_c, b[:, c].double()))
        ref, off = base.clone(), 0
        for a_, n in zip(add, d["Ns"]):
            if a_.shape[1]:
                ref[:, off : off + n] += a_
            off += n
        e = C.over_bar(y.float().cpu(), ref)
        print(f"[{name}] {label} rank probe: {e:.2f}x the GEMM bar")
        assert e <= 1.0, (label, e)


# ------------------------------------------------------------------------------------------------------------------------- other bases
def _oracle_group(d, kind, base, dyn):
    """fp32 oracle of the group: O.linear per member (O.int8_linear / O.dora_linear inside), with autograd on x, A, B, m."""
    p, leaves = {}, dict(A=[], B=[], m=[])
    x = d["x"].clone().requires_grad_()
    ys = []
    for i, (w, a, b, s) in enumerate(zip(d["W"], d["A"], d["B"], d["s"])):
        key = f"g{i}"
        if base == "bf16":
            p[key + ".weight"] = w
        else:
            q, sc = O.quantize_int8_rowwise(w.to(BF16))
            p[key + ".int_data"], p[key + ".scale"], p[key + ".dynamic"] = q, sc.float(), dyn
        p[key + ".lora_a"], p[key + ".lora_b"] = a.clone().requires_grad_(), b.clone().requires_grad_()
        leaves["A"].append(p[key + ".lora_a"])
        leaves["B"].append(p[key + ".lora_b"])
        if kind == "dora":
            p[key + ".m"] = C.dora_m(d, i).clone().requires_grad_()
            leaves["m"].append(p[key + ".m"])
        ys.append(O.linear(x, p, key, s))
    y = torch.cat(ys, 1)
    y.backward(d["dy"])
    return y.detach(), x.grad, leaves


@pytest.mark.parametrize("which", ["qkv", "gu"])
@pytest.mark.parametrize("name", ["r21", "r32"])
@pytest.mark.parametrize("base", ["int8-weight-only", "int8-dynamic"])
def test_group_on_int8_base(K, cuda, base, name, which):
    """r21: fused and odd; r32: q|k|v member by member through LinearPlan's int8 branch with a strided out, gate|up fused at R = 64.
    Reference: O.int8_linear per member plus the adapter, as O.linear composes them; bars of test_int8_mm_dequant_with_lora_extension."""
    case = C.CASES[name]
    d = C.group_data(case, C.MID, which)
    ref_y, ref_dx, leaves = _oracle_group(d, "lora", base, base == "int8-dynamic")
    plan, y, _, dx, g = _drive(K, cuda, d, _cuda_mods(d, cuda, base=base))
    want = case.mid[0] if which == "qkv" else case.mid[1]
    assert plan.fused == want.fused and plan.int8 and plan.dynamic == (base == "int8-dynamic")
    worst = {}
    _check_bar(y, ref_y, "y", worst)
    _check_bar(dx, ref_dx, "dx", worst)
    for i in range(len(d["Ns"])):
        _check_bar(g["dA"][i], leaves["A"][i].grad, "dA", worst)
        _check_bar(g["dB"][i], leaves["B"][i].grad, "dB", worst)
        _rows_close(g["dA"][i].float().cpu(), leaves["A"][i].grad, f"dA_{i} rows", min_cos=0.999)
        _rows_close(g["dB"][i].float().cpu().T, leaves["B"][i].grad.T, f"dB_{i}^T rows", min_cos=0.999)
    print(f"[{base} {name} {which}] {'fused' if plan.fused else 'per member'}: worst / bar " + " ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    _, y2, _, dx2, g2 = _drive(K, cuda, d, _cuda_mods(d, cuda, base=base))
    assert torch.equal(y2, y) and torch.equal(dx2, dx) and all(torch.equal(a, b) for k in ("dA", "dB") for a, b in zip(g[k], g2[k]))


def _rel(got, ref):
    return ((got.float().cpu() - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("which", ["qkv", "gu"])
@pytest.mark.parametrize("name", ["r5", "r32"])
def test_group_dora(K, cuda, name, which):
    """DoRA on a bf16 base against O.dora_linear: the column scale and the norm at the bars of test_dora_colscale_and_dm (2^-6 / 2^-7
    relative), output within 0.02 and dx, dA, dB, dm within 0.03 of their max-norms (test_dora_linear_standalone)."""
    case = C.CASES[name]
    d = C.group_data(case, C.MID, which)
    ref_y, ref_dx, leaves = _oracle_group(d, "dora", "bf16", False)
    plan, y, saved, dx, g = _drive(K, cuda, d, _cuda_mods(d, cuda, kind="dora"))
    want = case.mid[0] if which == "qkv" else case.mid[1]
    assert plan.fused == want.fused and plan.dora
    # c = m / ||W + s B A||_row and 1 / norm as the plan saved them
    cs, invs = ([saved[4]], [saved[5]]) if plan.fused else ([s[2] for s in saved], [s[3] for s in saved])
    c, inv = torch.cat(cs).float().cpu(), torch.cat(invs).cpu()
    norm = torch.cat([(w + s * (b @ a)).norm(dim=1) for w, a, b, s in zip(d["W"], d["A"], d["B"], d["s"])])
    m = torch.cat([C.dora_m(d, i) for i in range(len(d["Ns"]))])
    torch.testing.assert_close(1.0 / inv, norm, rtol=2 ** -7, atol=0)
    torch.testing.assert_close(c, m / norm, rtol=2 ** -6, atol=0)
    errs = {"y": _rel(y, ref_y), "dx": _rel(dx, ref_dx)}
    for k, key in (("dA", "A"), ("dB", "B"), ("dm", "m")):
        errs[k] = max(_rel(a, b.grad) for a, b in zip(g[k], leaves[key]))
    print(f"[dora {name} {which}] {'fused' if plan.fused else 'per member'}: " + " ".join(f"{k} {v:.4f}" for k, v in errs.items()) + " (bars y 0.02, others 0.03)")
    assert errs["y"] <= 0.02 and max(v for k, v in errs.items() if k != "y") <= 0.03, errs
    for i in range(len(d["Ns"])):
        _rows_close(g["dA"][i].float().cpu(), leaves["A"][i].grad, f"dA_{i} rows", min_cos=0.999)
        _rows_close(g["dB"][i].float().cpu().T, leaves["B"][i].grad.T, f"dB_{i}^T rows", min_cos=0.999)
    _, y2, _, dx2, g2 = _drive(K, cuda, d, _cuda_mods(d, cuda, kind="dora"))
    assert torch.equal(y2, y) and torch.equal(dx2, dx) and all(torch.equal(a, b) for k in ("dA", "dB", "dm") for a, b in zip(g[k], g2[k]))


# ------------------------------------------------------------------------------------------------------------------------- layer level
LAYER_CASES = [(n, "bf16", "lora") for n in C.CASES] + [(n, b, "lora") for n in ("r21", "r32") for b in ("int8-weight-only", "int8-dynamic")] \
    + [(n, "bf16", "dora") for n in ("r5", "r32")]


@pytest.mark.parametrize("name,base,kind", LAYER_CASES)
def test_layer_parity_at_every_rank_class(cuda, name, base, kind):
    """TransformerLayer at MID, S = 320, causal, against O.layer - bars, row cosines and the bit-identical second run of
    test_full_dimension_layer_parity.  From rank 22 (q|k|v) and 33 (gate|up) the groups run member by member: RoPE and SwiGLU are then
    stand-alone kernels, checked here against the oracle's arithmetic together with the residual and norm joins."""
    case = C.CASES[name]
    scales = {suf: case.scale(suf) for suf in O.LINEAR_SUFFIXES}
    layer_parity(cuda, C.MID, C.M_TOK, "causal", base, (kind, C.layer_lora(case, C.MID), scales), tag=f"{name}-{kind}")
