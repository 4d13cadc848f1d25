"""Batched text generation at 8B dimensions: one generate() over B right-padded prompts next to B sequential batch-1 generate() calls -
the only alternative without a batch cache - on the same build in the same process, and the MFMA weight stream (llx_gemm_rows16_bf16)
next to the GEMV (llx_gemv_bf16) on the five products of an 8B decode step.

Setup: Llama-3.1-8B dimensions, random weights, max_seq_len 8192, prompts of `--prompt` tokens (about that many cached positions), `--new`
tokens, greedy.  For each B in 1, 2, 4, 8, 16:
  * ms per decode step: `--steps` steps of model(tok [B, 1], input_pos=pos[:, None]) + the sampler launch, between device events, against
    the cache a prefill left; the sequential side is the batch-1 step (same loop, batch-1 cache) times B;
  * generated tokens/s of whole generate() calls (prefill included), wall clock between device synchronisations: one batched call against
    B batch-1 calls, one per prompt row.
The batched and the sequential window alternate, `--rounds` times each after an untimed pass of both; medians with min-max.
`batched_faster` holds when the batched step beats B single steps by more than the two windows' spreads together.
Kernels: each product is launched alone between device events, the variants (GEMV M = 1; rows16 M = 2, 8, 16) and products interleaved
so that 1.5 GB of other weights pass between two launches on the same matrix; median of `--kernel-rounds`; GB/s = weight bytes / time.

--int8: the layers quantised with quantize_linear_(model.layers, "int8", dynamic_int8_act=True), the head bf16 - the int8 workload of
bench.py.  The batched step then runs the int8 weight stream (llx_gemm_rows16_i8); a third window, alternating with the other two,
times the same batched step on the generic inference path (llx.decode.BATCHED = False: MFMA GEMMs at M = B with a row-quantise launch
per linear - what a dynamic-int8 batch ran before the int8 stream existed); `faster_than_generic` holds by the same spread rule.  A
fourth window times the batched step of a bf16 model of the same dimensions and seed (llx_gemm_rows16_bf16) against the same caches:
`bf16_batched_step_ms`.  The
kernel table then has the five products through gemm_rows16 on int8 rows next to the bf16 rows16 and the int8 GEMV (dynamic) figures.

--adapter lora|dora: every layer linear dressed with apply_linear_adapter_(model.layers, ..., rank=16, alpha=32) (B factors drawn
N(0, 0.02^2)); with --int8 (LoRA only) on the dynamic-int8 layers.  The batched step then runs the adapter entry points of the weight
stream (llx_gemm_rows16_bf16_lora / llx_gemm_rows16_i8_lora).  Four windows alternate for B in 2, 4, 8, 16: (a) the batched adapted step,
(b) the same model on the generic inference path (llx.decode.BATCHED = False: the route of an adapted batch before these entry points
existed), (c) B batch-1 steps, (d) the batched step of the un-adapted model of the same base and seed (`base_batched_step_ms`: what
the adapters cost).  `keep_fast_path` holds when (a) beats both (b) and (c) by more than the larger of the two windows' min-max
spreads.  The kernel table is skipped.  Default output: profiles/generate_batch_lora_bench[_dora | _int8].json.

    python tools/generate_batch_bench.py [--int8] [--adapter lora|dora] [--prompt 1024] [--new 64] [--rounds 5] [--layers 32] [--out profiles/generate_batch_bench.json]
(--int8: the default output is profiles/generate_batch_int8_bench.json)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 2, 4, 8, 16)


def build(layers: int, seq: int, device):
    import torch
    from modelling import Llama, LlamaConfig

    cfg = LlamaConfig(embed_dim=4096, num_layers=layers, head_dim=128, num_heads=32, num_kv_heads=8, intermediate_dim=14336, max_seq_len=seq,
                      vocab_size=128_256, rope_base=500_000, is_llama3_1=True)
    with torch.device("meta"):
        model = Llama(cfg)
    model = model.to(torch.bfloat16).to_empty(device=device)
    g = torch.Generator(device=device)
    g.manual_seed(1234)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("norm.weight"):
                p.fill_(1.0)
            else:
                p.normal_(0.0, 0.02, generator=g)
    model.requires_grad_(False)
    model.eval()
    return model, cfg


def caches_for(model, cfg, B, device):
    """A KV cache of batch B per layer (the rope table and mask are built once by the caller)."""
    from modelling.llama import KVCache

    return [KVCache(B, cfg, model.tok_embeddings.weight.dtype).to(device) for _ in model.layers]


def install(model, caches):
    for layer, c in zip(model.layers, caches):
        layer.attention.kv_cache = c


def stats(xs):
    s = sorted(xs)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=1024)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--kernel-rounds", type=int, default=15)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--int8", action="store_true", help="dynamic-int8 layers (bf16 head): the int8 batched weight stream")
    ap.add_argument("--adapter", choices=("lora", "dora"), default=None, help="rank-16 adapters on every layer linear (with --int8: lora only)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.adapter == "dora" and args.int8:
        raise SystemExit("generate_batch_bench: DoRA rides on bf16 weights only")
    for p in (ROOT, os.path.join(ROOT, "llama-x_amd")):
        sys.path.insert(0, p)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("generate_batch_bench: no GPU (there is no CPU path to time)")
    import llx.decode as DEC
    from llx import kernels as K
    from llx.generate import generate, prefill

    dev = torch.device("cuda:0")
    model, cfg = build(args.layers, 8192, dev)
    model.build_cache(inference=True)
    model = model.to(dev)
    P, n = args.prompt, args.new
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    prompts = torch.randint(0, cfg.vocab_size, (max(BATCHES), P), device=dev, generator=g)
    res = {"workload": f"Llama-3.1-8B dimensions ({args.layers} layers), random weights{', layers dynamic int8 (bf16 head)' if args.int8 else ''}"
                       f"{f', {args.adapter} r=16 alpha=32 on every layer linear' if args.adapter else ''}, "
                       f"max_seq_len 8192, prompts of {P} tokens, {n} new tokens, greedy; medians (min-max) of {args.rounds} alternating rounds"}
    if args.adapter and args.out is None:
        args.out = os.path.join(ROOT, "profiles", f"generate_batch_lora_bench{'_dora' if args.adapter == 'dora' else ''}{'_int8' if args.int8 else ''}.json")
    if args.int8 and args.out is None:
        args.out = os.path.join(ROOT, "profiles", "generate_batch_int8_bench.json")

    def events(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    # ---- the five products of a decode step, kernel by kernel
    lay = model.layers[0]
    att, ff = lay.attention, lay.feed_forward
    D, I, H, KVH = cfg.embed_dim, cfg.intermediate_dim, cfg.num_heads, cfg.num_kv_heads
    rope = model.rope[:1].float().contiguous()
    kc = torch.zeros(16, KVH, 64, 128, device=dev, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    xD = torch.randn(16, D, device=dev, generator=g).bfloat16()
    xI = torch.randn(16, I, device=dev, generator=g).bfloat16()
    n1 = (lay.attention_norm.weight.detach(), 1e-5)
    pos16 = torch.arange(16, device=dev)
    # the weights of layer 0 and the head, by kind: bf16 as built; --int8: also their int8 rows and scales (the head's for this table only)
    mods = {"wq": att.wq, "wk": att.wk, "wv": att.wv, "wo": att.wo, "w1": ff.w1, "w3": ff.w3, "w2": ff.w2, "output": model.output}
    bf = {k: m.weight.detach() for k, m in mods.items()}
    q8 = {}
    model_bf16 = model_base = None
    if args.int8:
        from subclasses import quantize_linear_
        from subclasses.int8 import quantize_int8_rowwise

        if not args.adapter:
            q8 = {k: quantize_int8_rowwise(w) for k, w in bf.items()}
        quantize_linear_(model.layers, "int8", dynamic_int8_act=True)
        if not args.adapter:
            model_bf16, _ = build(args.layers, 8192, dev)  # the bf16 twin for the bf16 batched-step window
            model_bf16.build_cache(inference=True)
            model_bf16 = model_bf16.to(dev)
    if args.adapter:
        from modelling import apply_linear_adapter_

        model_base, _ = build(args.layers, 8192, dev)  # the un-adapted twin of the same base
        model_base.build_cache(inference=True)
        model_base = model_base.to(dev)
        if args.int8:
            quantize_linear_(model_base.layers, "int8", dynamic_int8_act=True)
        apply_linear_adapter_(model.layers, args.adapter, rank=16, alpha=32.0)
        with torch.no_grad():
            for m in model.layers.modules():
                if getattr(m, "lora_b", None) is not None:
                    m.lora_b.normal_(0.0, 0.02, generator=g)
        model.requires_grad_(False)
        x1 = torch.zeros(2, 1, cfg.embed_dim, device=dev, dtype=torch.bfloat16)
        install(model, caches_for(model, cfg, 2, dev))
        assert DEC.layer_ok(model.layers[0], x1, model.causal_mask[torch.zeros(2, 1, dtype=torch.int64, device=dev)][:, None]), "the adapted layer is not on the batched fast path"

    def operands(kind, names):
        return dict(ws=[bf[k] for k in names]) if kind == "bf16" else dict(ws=[q8[k][0] for k in names], wscale=[q8[k][1] for k in names])

    products = {
        "q|k|v (6144 x 4096, norm, RoPE + scatter)": (("wq", "wk", "wv"), 6144 * 4096, lambda M, c: dict(x=xD[:M], norm=n1, epilogue=K.GV_QKV,
                                                                                                      qkv=(rope, H * 128, KVH * 128, c[0], c[1], pos16[:M]))),
        "wo (4096 x 4096, + residual)": (("wo",), 4096 * 4096, lambda M, c: dict(x=xD[:M], epilogue=K.GV_RESIDUAL, res=xD[:M])),
        "gate|up (28672 x 4096, norm, SwiGLU)": (("w1", "w3"), 28672 * 4096, lambda M, c: dict(x=xD[:M], norm=n1, epilogue=K.GV_SWIGLU)),
        "w2 (4096 x 14336, + residual)": (("w2",), 4096 * 14336, lambda M, c: dict(x=xI[:M], epilogue=K.GV_RESIDUAL, res=xD[:M])),
        "head (128256 x 4096, norm)": (("output",), 128256 * 4096, lambda M, c: dict(x=xD[:M], norm=n1)),
    }
    # (name, entry point, rows, caches, weight kind, extra arguments)
    variants = [("gemv M=1", K.gemv, 1, (kc[:1], vc[:1]), "bf16", {})] if not args.int8 else [("gemv int8 M=1", K.gemv, 1, (kc[:1], vc[:1]), "int8", dict(dynamic=True))]
    variants += [(f"rows16 M={M}", K.gemm_rows16, M, (kc, vc), "bf16", {}) for M in (2, 8, 16)]
    if args.int8:
        variants += [(f"rows16 int8 M={M}", K.gemm_rows16, M, (kc, vc), "int8", {}) for M in (2, 8, 16)]
    if args.adapter:
        variants = []  # the adapter windows below are the measurement
    times = {(v[0], name): [] for v in variants for name in products}
    for r in range(args.kernel_rounds + 1):
        for vname, f, M, c, kind, extra in variants:
            for name, (names, _, kw) in products.items():
                w = operands(kind, names)
                t = events(lambda: f(**w, **kw(M, c), **extra), 1)
                if r > 0:  # the first round is untimed
                    times[(vname, name)].append(t * 1e3)
    if variants:
        res["kernels_us_and_GBps"] = {name: {v[0]: {"us": stats(times[(v[0], name)]),
                                                    "GBps": round(products[name][1] * (2 if v[4] == "bf16" else 1) / (stats(times[(v[0], name)])["median"] * 1e-6) / 1e9, 1)}
                                             for v in variants} for name in products}

    # ---- decode steps and whole generate() calls, batched against sequential
    if not args.kernels_only:
        one = caches_for(model, cfg, 1, dev)
        res["batches"] = {}
        for B in (BATCHES[1:] if args.adapter else BATCHES):
            many = one if B == 1 else caches_for(model, cfg, B, dev)
            pr = prompts[:B]

            def step_ms(batch, model=model):
                """ms per decode step of `batch` sequences against the installed cache (prefilled here)."""
                pb = prompts[:batch]
                logits = prefill(model, pb)
                pos = torch.full((batch,), P - 1, device=dev, dtype=torch.int64)
                tok = torch.empty(batch, 1, device=dev, dtype=torch.int64)
                kw = dict(temperature=0.0, pos=pos, out=tok.view(batch), advance=True)
                K.sample(logits[:, 0], **kw)

                def one_step():
                    K.sample(model(tok, input_pos=pos[:, None])[:, 0], **kw)

                with torch.no_grad():
                    one_step()
                    return events(one_step, args.steps)

            def gen_batched():
                install(model, many)
                return generate(model, pr, n)

            def gen_sequential():
                install(model, one)
                return [generate(model, pr[b : b + 1], n) for b in range(B)]

            def wall(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            gen_batched(), gen_sequential()  # untimed pass of both
            ms = {"batched_step": [], "single_step": [], "batched_generate": [], "sequential_generate": [], "generic_step": [], "bf16_batched_step": [],
                  "base_batched_step": []}
            for _ in range(args.rounds):
                install(model, many)
                ms["batched_step"].append(step_ms(B))
                if (args.int8 or args.adapter) and B > 1:  # the same step on the generic inference path
                    DEC.BATCHED = False
                    try:
                        ms["generic_step"].append(step_ms(B))
                    finally:
                        DEC.BATCHED = True
                if model_bf16 is not None:  # the bf16 model's batched step against the same caches
                    install(model_bf16, many)
                    ms["bf16_batched_step"].append(step_ms(B, model_bf16))
                if model_base is not None:  # the un-adapted model's batched step against the same caches
                    install(model_base, many)
                    ms["base_batched_step"].append(step_ms(B, model_base))
                install(model, one)
                ms["single_step"].append(step_ms(1))
                ms["batched_generate"].append(wall(gen_batched))
                ms["sequential_generate"].append(wall(gen_sequential))
            bs, ss = stats(ms["batched_step"]), stats([x * B for x in ms["single_step"]])
            bg, sg = stats(ms["batched_generate"]), stats(ms["sequential_generate"])
            res["batches"][str(B)] = {
                "batched_step_ms": bs, "sequential_steps_ms": ss, "step_speedup": round(ss["median"] / bs["median"], 2),
                "batched_generate_ms": bg, "sequential_generate_ms": sg,
                "batched_tokens_per_s": round(B * n / (bg["median"] * 1e-3), 1), "sequential_tokens_per_s": round(B * n / (sg["median"] * 1e-3), 1),
                "batched_faster": ss["median"] - bs["median"] > (bs["max"] - bs["min"]) + (ss["max"] - ss["min"]),
            }
            if ms["generic_step"]:
                gs = stats(ms["generic_step"])
                res["batches"][str(B)].update({"generic_step_ms": gs, "speedup_over_generic": round(gs["median"] / bs["median"], 2),
                                               "faster_than_generic": gs["median"] - bs["median"] > (bs["max"] - bs["min"]) + (gs["max"] - gs["min"])})
            if ms["bf16_batched_step"]:
                fs = stats(ms["bf16_batched_step"])
                res["batches"][str(B)].update({"bf16_batched_step_ms": fs, "int8_over_bf16_step": round(bs["median"] / fs["median"], 2)})
            if ms["base_batched_step"]:
                fs, gs = stats(ms["base_batched_step"]), stats(ms["generic_step"])
                spread = lambda a, b: max(a["max"] - a["min"], b["max"] - b["min"])  # noqa: E731
                res["batches"][str(B)].update({
                    "base_batched_step_ms": fs, "adapted_over_base_step": round(bs["median"] / fs["median"], 2),
                    "keep_fast_path": gs["median"] - bs["median"] > spread(gs, bs) and ss["median"] - bs["median"] > spread(ss, bs)})
            print(f"B={B}: {json.dumps(res['batches'][str(B)])}", file=sys.stderr, flush=True)
            if B > 1:
                del many
                torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
