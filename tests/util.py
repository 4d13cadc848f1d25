"""Shared helpers of the parity tests: build the product model from oracle-style parameter dicts."""
import torch

from oracle import ref as O


def bf16_params(p: dict) -> dict:
    """Round every floating tensor to bf16 (the GPU dtype) and return (bf16 dict, fp32 dict of the same rounded values)."""
    pb = {k: (v.to(torch.bfloat16) if v.is_floating_point() else v) for k, v in p.items()}
    pf = {k: (v.float() if v.is_floating_point() else v) for k, v in pb.items()}
    return pb, pf


def to_model_config(cfg: O.Cfg):
    from modelling import LlamaConfig

    return LlamaConfig(**{f: getattr(cfg, f) for f in LlamaConfig._fields})


def build_model(cfg: O.Cfg, params_bf16: dict, device, *, lora_rank: int = 0, lora_alpha: float | None = None, quantize: str | None = None,
                quantize_kwargs: dict | None = None, audio: bool = False):
    """Product model on ``device`` with the given weights; surgery order = quantise then adapt (train_metamathqa.py:178-179)."""
    from modelling import Llama, LlamaAudio, apply_linear_adapter_
    from subclasses import quantize_linear_

    model = (LlamaAudio if audio else Llama)(to_model_config(cfg))
    model = model.bfloat16()
    base = {k: v for k, v in params_bf16.items() if not (k.endswith(".lora_a") or k.endswith(".lora_b"))}
    missing = model.load_state_dict(base, strict=False)
    assert not missing.unexpected_keys, missing
    model.build_cache()
    if quantize:
        quantize_linear_(model.layers, quantize, **(quantize_kwargs or {}))
    if lora_rank:
        apply_linear_adapter_(model.layers, "lora", rank=lora_rank, alpha=float(lora_alpha if lora_alpha is not None else lora_rank))
        with torch.no_grad():
            for name, mod in model.layers.named_modules():
                key = f"layers.{name}"
                if key + ".lora_a" in params_bf16:
                    mod.lora_a.copy_(params_bf16[key + ".lora_a"])
                    mod.lora_b.copy_(params_bf16[key + ".lora_b"])
    return model.to(device)


def _close(a, b, rel, name):
    scale = b.abs().max().item()
    err = (a - b).abs().max().item()
    assert err <= rel * scale + 1e-6, f"{name}: max err {err:.4e} vs scale {scale:.4e} (allowed {rel * scale:.4e})"


def _rows_close(a, b, name, min_cos=0.999, floor=1e-3):
    """Per-row check next to the max-norm one: every row (last dim) of `a` must point the same way as the reference row and have
    the same length - an error confined to small-magnitude rows (a dropped LoRA row block, a mis-rotated head) passes `_close` but
    not this.  Rows whose reference norm is below `floor` x the largest row norm carry rounding noise only and are skipped."""
    a2, b2 = a.reshape(-1, a.shape[-1]).double(), b.reshape(-1, b.shape[-1]).double()
    nb = b2.norm(dim=1)
    keep = nb > floor * nb.max()
    cos = (a2 * b2).sum(1) / (a2.norm(dim=1) * nb).clamp_min(1e-30)
    worst = cos[keep].min().item()
    assert worst >= min_cos, f"{name}: worst per-row cosine {worst:.5f} < {min_cos} (row {int(cos.masked_fill(~keep, 2).argmin())})"
    ratio = (a2.norm(dim=1) / nb.clamp_min(1e-30))[keep]
    assert (ratio - 1).abs().max().item() < 0.05, f"{name}: per-row norm ratio off by {(ratio - 1).abs().max().item():.4f}"


def _mask_for(kind, S):
    """(dense bool oracle mask | None, MaskSpec | None) for the layer-parity cases."""
    from modelling.llama import MaskSpec

    if kind == "causal":
        return None, None
    if kind == "doc":  # packed documents of uneven length + the packer's id-0 tail (train_metamathqa.py:51-83)
        doc = torch.zeros(S, dtype=torch.int64)
        for c in (S // 16 + 5, S // 3 + 77, S // 2 - 130, (7 * S) // 8 + 9):
            doc[c:] += 1
        doc[S - 100 :] = 0
        return O.document_mask(doc), MaskSpec(doc_ids=doc)
    if kind == "prefix":  # prefix-LM: bidirectional over the first P positions (P not a multiple of the 64/128 tiles)
        P = S // 2 - 56
        return O.prefix_lm_mask(S, [P])[0, 0], MaskSpec(prefix_len=torch.tensor([P]))
    raise ValueError(kind)


def layer_parity(cuda, cfg: O.Cfg, S: int, kind: str, base: str, adapters, tag: str = ""):
    """One TransformerLayer at `cfg` against the oracle (O.layer, fp32 on the same bf16-rounded weights): output, dx, the gradients of
    the adapter factors and the norm weights, each max-norm and per row, then a bit-identical second run.  kind: the mask ("causal",
    "doc", "prefix", "mixed-prefix-b2"); base: "bf16" | "int8-dynamic" | "int8-weight-only" (quantise, then adapt); adapters = (adapter
    kind "lora" | "dora", factors under the oracle's key names - a linear without factors stays a plain frozen nn.Linear -, alpha / rank
    as one number or per linear suffix).  Returns the measured (output, dx, worst gradient) errors relative to their max-norms."""
    from modelling import apply_linear_adapter_
    from modelling.llama import LlamaConfig, MaskSpec, TransformerLayer, build_rope
    from subclasses import quantize_linear_

    akind, factors, scales = adapters
    scale_of = (lambda suf: scales[suf]) if isinstance(scales, dict) else (lambda suf: scales)
    adapted = [suf for suf in O.LINEAR_SUFFIXES if f"layers.0.{suf}.lora_a" in factors]
    s_ref = scale_of(adapted[0])  # the oracle takes ONE alpha / rank: a linear with another one gets B * (its scale / s_ref), which is
    fold = {suf: scale_of(suf) / s_ref for suf in adapted}  # the same function (exact for powers of two), and d B = fold * d (fold B)
    p = {k: v for k, v in O.init_params(cfg._replace(vocab_size=8)).items() if k.startswith("layers.0.")}
    p.update(factors)
    if akind == "dora":
        p.update({k: v for k, v in O.init_dora_m(p, cfg).items() if k[: -len(".m")] + ".lora_a" in factors})
    pb, pf = bf16_params(p)
    for suf in adapted:
        pf[f"layers.0.{suf}.lora_b"] = pf[f"layers.0.{suf}.lora_b"] * fold[suf]
    B = 2 if kind == "mixed-prefix-b2" else 1
    x = O.randn("x_full", (B, S, cfg.embed_dim), 0.5).bfloat16()
    dy = O.randn("dy_full", (B, S, cfg.embed_dim), 0.1).bfloat16()
    if base != "bf16":  # oracle side: quantise the bf16 weights exactly as Int8LinearWeight.from_float does (scales in bf16)
        for suf in O.LINEAR_SUFFIXES:
            key = f"layers.0.{suf}"
            q, sc = O.quantize_int8_rowwise(pb[key + ".weight"])
            pf.pop(key + ".weight")
            pf[key + ".int_data"], pf[key + ".scale"], pf[key + ".dynamic"] = q, sc.float(), base == "int8-dynamic"
    train = [k for k in pf if "lora_" in k or k.endswith("_norm.weight") or k.endswith(".m")]
    pr = {k: (v.clone().requires_grad_() if k in train else v) for k, v in pf.items()}
    xr = x.float().requires_grad_()
    if kind == "mixed-prefix-b2":  # configs[4]: per-sample prefix lengths {2048, 4096} in one batch
        P = torch.tensor([2048, 4096])
        spec = MaskSpec(prefix_len=P)
        outs = []
        for b in range(B):  # the oracle sample by sample (its [H, S, S] fp32 scores are 8.6 GB each); parameter gradients add up
            ob = O.layer(xr[b : b + 1], pr, 0, cfg, O.rope_table(cfg)[:S], O.prefix_lm_mask(S, P[b : b + 1])[0, 0], s_ref)
            ob.backward(dy[b : b + 1].float())
            outs.append(ob.detach())
        ref = torch.cat(outs)
    else:
        dense, spec = _mask_for(kind, S)
        ref = O.layer(xr, pr, 0, cfg, O.rope_table(cfg)[:S], dense, s_ref)
        ref.backward(dy.float())
        ref = ref.detach()
    want = {k: pr[k].grad * (fold[k[len("layers.0."): -len(".lora_b")]] if k.endswith(".lora_b") else 1.0) for k in train}

    layer = TransformerLayer(LlamaConfig(**{f: getattr(cfg, f) for f in LlamaConfig._fields})).bfloat16()
    layer.load_state_dict({k[len("layers.0."):]: v for k, v in pb.items() if "lora_" not in k and not k.endswith(".m")})
    if base != "bf16":
        quantize_linear_(layer, "int8", dynamic_int8_act=base == "int8-dynamic")
    with torch.no_grad():
        for name, mod in layer.named_modules():
            if f"layers.0.{name}.lora_a" in pb:
                rank = pb[f"layers.0.{name}.lora_a"].shape[0]
                apply_linear_adapter_(mod, akind, rank=rank, alpha=float(scale_of(name) * rank))
                mod.lora_a.copy_(pb[f"layers.0.{name}.lora_a"])
                mod.lora_b.copy_(pb[f"layers.0.{name}.lora_b"])
                if akind == "dora":
                    mod.m.copy_(pb[f"layers.0.{name}.m"])
    layer = layer.to(cuda)
    for n, q in layer.named_parameters():
        q.requires_grad_("lora_" in n or n.endswith("_norm.weight") or n.endswith(".m"))
    rope = build_rope(LlamaConfig(**{f: getattr(cfg, f) for f in LlamaConfig._fields})).to(cuda)
    xg = x.to(cuda).requires_grad_()
    out = layer(xg, rope[:S], block_mask=spec)
    out.backward(dy.to(cuda))
    # Dynamic int8 activations: the oracle runs in fp32, the product rounds every activation to bf16 before the row-wise quantiser, so
    # a few per cent of the int8 codes differ by one step between the two - a difference of the size of the quantisation noise itself
    # (the heavy-tailed silu(g)*u rows carry ~3 % of it).  The max-norm bars widen accordingly; the per-row cosine bars stay tight
    # enough to catch any structural error (a wrong scale, a dropped row block, a mis-rotated head).
    dyn = base == "int8-dynamic"
    t_out, t_dx, t_g = (0.06, 0.08, 0.08) if dyn else (0.02, 0.04, 0.05)
    c_out, c_dx, c_g = (0.998, 0.995, 0.99) if dyn else (0.999, 0.998, 0.995)
    o_cpu, dx_cpu = out.float().cpu(), xg.grad.float().cpu()
    e_out, e_dx = ((o_cpu - ref).abs().max() / ref.abs().max()).item(), ((dx_cpu - xr.grad).abs().max() / xr.grad.abs().max()).item()
    e_g = max(((q.grad.float().cpu() - want["layers.0." + n]).abs().max() / want["layers.0." + n].abs().max()).item()
              for n, q in layer.named_parameters() if q.requires_grad)
    print(f"[{tag or S}-{kind}-{base}] out err {e_out:.4f} (bar {t_out}), dx err {e_dx:.4f} (bar {t_dx}), worst gradient err {e_g:.4f} (bar {t_g})")
    _close(o_cpu, ref, t_out, "layer output")
    _rows_close(o_cpu, ref, "layer output rows", min_cos=c_out)
    _close(dx_cpu, xr.grad, t_dx, "dx")
    _rows_close(dx_cpu, xr.grad, "dx rows", min_cos=c_dx)
    for name, q in layer.named_parameters():
        if q.requires_grad:
            _close(q.grad.float().cpu(), want["layers.0." + name], t_g, name)
            if q.grad.dim() == 2:
                # per-row direction of the gradient.  A row of d lora_b has `rank` elements: below 16 of them (one at rank 1, where the
                # "cosine" is a sign) a row's rounding error is not small against the row itself, so narrow factors are compared along
                # their other axis - one row of N elements per rank, which is also where a dropped or exchanged rank shows
                g_, w_ = q.grad.float().cpu(), want["layers.0." + name]
                if g_.shape[1] < 16:
                    g_, w_ = g_.T, w_.T
                _rows_close(g_, w_, name, min_cos=c_g)
    # determinism: a second run is bit-identical (no atomics anywhere on the path)
    xg2 = x.to(cuda).requires_grad_()
    for q in layer.parameters():
        q.grad = None
    out2 = layer(xg2, rope[:S], block_mask=spec)
    out2.backward(dy.to(cuda))
    assert torch.equal(out2, out) and torch.equal(xg2.grad, xg.grad)
    return e_out, e_dx, e_g
