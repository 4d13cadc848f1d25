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

    python tools/generate_batch_bench.py [--prompt 1024] [--new 64] [--rounds 5] [--layers 32] [--out profiles/generate_batch_bench.json]
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "llama-x_amd")):
        sys.path.insert(0, p)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("generate_batch_bench: no GPU (there is no CPU path to time)")
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
    res = {"workload": f"Llama-3.1-8B dimensions ({args.layers} layers), random weights, max_seq_len 8192, prompts of {P} tokens, {n} new tokens, greedy; "
                       f"medians (min-max) of {args.rounds} alternating rounds"}

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
    products = {
        "q|k|v (6144 x 4096, norm, RoPE + scatter)": lambda f, M, c: f([att.wq.weight, att.wk.weight, att.wv.weight], xD[:M], norm=n1, epilogue=K.GV_QKV,
                                                                      qkv=(rope, H * 128, KVH * 128, c[0], c[1], pos16[:M])),
        "wo (4096 x 4096, + residual)": lambda f, M, c: f([att.wo.weight], xD[:M], epilogue=K.GV_RESIDUAL, res=xD[:M]),
        "gate|up (28672 x 4096, norm, SwiGLU)": lambda f, M, c: f([ff.w1.weight, ff.w3.weight], xD[:M], norm=n1, epilogue=K.GV_SWIGLU),
        "w2 (4096 x 14336, + residual)": lambda f, M, c: f([ff.w2.weight], xI[:M], epilogue=K.GV_RESIDUAL, res=xD[:M]),
        "head (128256 x 4096, norm)": lambda f, M, c: f([model.output.weight], xD[:M], norm=n1),
    }
    wbytes = {"q|k|v (6144 x 4096, norm, RoPE + scatter)": 6144 * 4096 * 2, "wo (4096 x 4096, + residual)": 4096 * 4096 * 2,
              "gate|up (28672 x 4096, norm, SwiGLU)": 28672 * 4096 * 2, "w2 (4096 x 14336, + residual)": 4096 * 14336 * 2,
              "head (128256 x 4096, norm)": 128256 * 4096 * 2}
    variants = [("gemv M=1", K.gemv, 1, (kc[:1], vc[:1])), ("rows16 M=2", K.gemm_rows16, 2, (kc, vc)), ("rows16 M=8", K.gemm_rows16, 8, (kc, vc)),
                ("rows16 M=16", K.gemm_rows16, 16, (kc, vc))]
    times = {(v[0], name): [] for v in variants for name in products}
    for r in range(args.kernel_rounds + 1):
        for vname, f, M, c in variants:
            for name, call in products.items():
                t = events(lambda: call(f, M, c), 1)
                if r > 0:  # the first round is untimed
                    times[(vname, name)].append(t * 1e3)
    res["kernels_us_and_GBps"] = {name: {v[0]: {"us": stats(times[(v[0], name)]), "GBps": round(wbytes[name] / (stats(times[(v[0], name)])["median"] * 1e-6) / 1e9, 1)}
                                         for v in variants} for name in products}

    # ---- decode steps and whole generate() calls, batched against sequential
    if not args.kernels_only:
        one = caches_for(model, cfg, 1, dev)
        res["batches"] = {}
        for B in BATCHES:
            many = one if B == 1 else caches_for(model, cfg, B, dev)
            pr = prompts[:B]

            def step_ms(batch):
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
            ms = {"batched_step": [], "single_step": [], "batched_generate": [], "sequential_generate": []}
            for _ in range(args.rounds):
                install(model, many)
                ms["batched_step"].append(step_ms(B))
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
