"""Single-token decode of the 8B model with MXFP4 weight-only linears, next to the bf16 and the int8 weight-only model, in one process run.

Mirrors tools/decode_int8_bench.py (8B dimensions, random weights and cache, one hipGraph replay per token, device events around every
replay) for four models: bf16, int8 weight-only, mxfp4, mxfp4 + LoRA r=16 - quantised on the device with quantize_linear_(model.layers,
...) as the training scripts do, so the head stays bf16.  All models are built and captured first; the timed windows then alternate
between them, `--rounds` times, so that a drift of the machine hits every model alike; per model and context the median round is
reported with the min-max spread over the rounds.  ms/token is also given as the fraction of the 8 TB/s HBM peak that the algorithmic
bytes make of it: weights at their stored width (MXFP4: 0.53125 bytes per layer weight = 4 bits + one scale byte per 32) and live K/V.
The int8wo arm of the same run is the yardstick of the mxfp4 arm.  The time quantize_linear_ takes on the 8B layers (device quantiser
plus its one finiteness check per linear) is recorded too.

    python tools/decode_mxfp4_bench.py [--models bf16,int8wo,mxfp4,mxfp4_lora] [--contexts 4096] [--steps 50] [--warmup 10] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

HBM_PEAK_GBS = 8000.0
MODELS = ("bf16", "int8wo", "mxfp4", "mxfp4_lora")


def build(kind: str, seq: int, device):
    """(model, config, seconds spent in quantize_linear_ or None)."""
    import torch
    from modelling import Llama, LlamaConfig, apply_linear_adapter_
    from subclasses import quantize_linear_

    cfg = LlamaConfig(embed_dim=4096, num_layers=32, head_dim=128, num_heads=32, num_kv_heads=8, intermediate_dim=14336, max_seq_len=seq,
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
    quant_s = None
    if not kind.startswith("bf16"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind.startswith("int8"):
            quantize_linear_(model.layers, "int8", dynamic_int8_act=False)
        else:
            quantize_linear_(model.layers, "mxfp4")
        torch.cuda.synchronize()
        quant_s = time.perf_counter() - t0
    if kind.endswith("_lora"):
        torch.manual_seed(1234)
        apply_linear_adapter_(model.layers, "lora", rank=16, alpha=16.0)
        with torch.no_grad():
            for n, p in model.named_parameters():
                if n.endswith("lora_b"):
                    p.normal_(0.0, 0.01, generator=g)
    model.requires_grad_(False)
    model.eval()
    model.build_cache(inference=True)
    model = model.to(device)
    for layer in model.layers:
        layer.attention.kv_cache.k_cache.normal_(0.0, 1.0, generator=g)
        layer.attention.kv_cache.v_cache.normal_(0.0, 1.0, generator=g)
    return model, cfg, quant_s


def weight_bytes(model, cfg) -> int:
    """Bytes of weights one decoded token reads: every parameter but the embedding table (one row of it); quantised matrices at their
    stored width plus their scales."""
    from subclasses import Int8LinearWeight, MXFP4LinearWeight

    total = cfg.embed_dim * 2
    for n, p in model.named_parameters():
        if n.startswith("tok_embeddings"):
            continue
        if isinstance(p, Int8LinearWeight):
            total += p.int_data.numel() * p.int_data.element_size() + p.scale.numel() * p.scale.element_size()
        elif isinstance(p, MXFP4LinearWeight):
            total += p.packed.numel() + p.scale.numel()
        else:
            total += p.numel() * p.element_size()
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--contexts", default="4096")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "llama-x_amd")):
        sys.path.insert(0, p)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("decode_mxfp4_bench: no GPU (there is no CPU path to time)")
    import llx.decode as D

    device = torch.device("cuda:0")
    kinds = [k for k in args.models.split(",") if k]
    assert all(k in MODELS for k in kinds), kinds
    contexts = [int(c) for c in args.contexts.split(",")]
    runs = {}
    with torch.no_grad():
        for kind in kinds:
            model, cfg, quant_s = build(kind, max(contexts), device)
            tok = torch.randint(0, cfg.vocab_size, (1, 1), device=device)
            pos = torch.zeros(1, dtype=torch.int64, device=device)
            fast = D.layer_ok(model.layers[0], model.tok_embeddings(tok), model.causal_mask[None, None, pos])
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    model(tok, input_pos=pos)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                logits = model(tok, input_pos=pos)
            layer_w = sum(p.numel() for n, p in model.layers.named_parameters() if n.endswith(".weight") and p.dim() == 2)
            runs[kind] = dict(model=model, cfg=cfg, pos=pos, graph=graph, logits=logits, weight_bytes=weight_bytes(model, cfg), quant_s=quant_s,
                              fast=bool(fast), layer_weights=layer_w, ms={c: [] for c in contexts})
        for _ in range(args.rounds):
            for kind in kinds:
                r = runs[kind]
                for ctx in contexts:
                    r["pos"].fill_(ctx - 1)
                    for _ in range(args.warmup):
                        r["graph"].replay()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.steps):
                        r["graph"].replay()
                    e1.record()
                    torch.cuda.synchronize()
                    r["ms"][ctx].append(e0.elapsed_time(e1) / args.steps)
    out = {"workload": "Llama-3.1-8B single-token decode (batch 1), random-init weights and cache, one hipGraph replay per token",
           "label": args.label, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "hbm_peak_gbs": HBM_PEAK_GBS, "models": {}}
    for kind in kinds:
        r, cfg = runs[kind], runs[kind]["cfg"]
        d = {"weight_bytes": r["weight_bytes"], "layer_weights": r["layer_weights"], "decode_fast_path": r["fast"],
             "finite_logits": bool(torch.isfinite(r["logits"].float()).all())}
        if r["quant_s"] is not None:
            d["quantize_layers_s"] = round(r["quant_s"], 3)
        for ctx in contexts:
            ms = sorted(r["ms"][ctx])
            med = ms[len(ms) // 2]
            kv_bytes = cfg.num_layers * 2 * cfg.num_kv_heads * ctx * cfg.head_dim * 2
            gbs = (r["weight_bytes"] + kv_bytes) / (med * 1e-3) / 1e9
            d[f"ctx{ctx}"] = {"ms_per_token": round(med, 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "tokens_per_s": round(1e3 / med, 1),
                              "kv_bytes": kv_bytes, "algorithmic_bytes": r["weight_bytes"] + kv_bytes, "achieved_gbs": round(gbs, 1),
                              "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
        out["models"][kind] = d
    if "mxfp4" in runs and "int8wo" in runs:
        out["mxfp4_over_int8wo"] = {f"ctx{c}": round(out["models"]["mxfp4"][f"ctx{c}"]["ms_per_token"] / out["models"]["int8wo"][f"ctx{c}"]["ms_per_token"], 4)
                                    for c in contexts}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
