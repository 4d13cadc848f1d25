"""Single-token decode of the 8B model with DoRA linears, next to the bf16 and the LoRA model, in one process run.

Built like tools/decode_int8_bench.py (8B dimensions, random weights and cache, one hipGraph replay per token, context 4096, device
events around every replay) for three models: bf16, bf16_lora (r = 16) and bf16_dora (r = 16, m = ||W||_row * (1 + 0.1 * noise)) -
adapted with apply_linear_adapter_(model.layers, ...) as the training scripts do, so the head stays plain.  All models are built and
captured first; the timed windows then alternate between them, `--rounds` times, so that a drift of the machine hits every model
alike; per model the median round is reported with the min-max spread over the rounds.

Only the public model API is used, so the script runs unchanged on a tree without the DoRA decode kernels (`--root` = that tree):
there the DoRA model decodes through the generic inference path, which is the baseline of the DoRA fast path.  Where the tree has
llx.decode.prepare it is called before the capture (the cached row factors must not be first allocated inside a capture; the two
warm-up steps before the capture would build them as well).

    python tools/decode_dora_bench.py [--root TREE] [--models bf16,bf16_lora,bf16_dora] [--steps 50] [--warmup 10] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys

HBM_PEAK_GBS = 8000.0
MODELS = ("bf16", "bf16_lora", "bf16_dora")


def build(kind: str, seq: int, device):
    import torch
    from modelling import Llama, LlamaConfig, apply_linear_adapter_

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
    if kind != "bf16":
        torch.manual_seed(1234)
        apply_linear_adapter_(model.layers, kind[len("bf16_"):], rank=16, alpha=16.0)
        with torch.no_grad():
            for n, p in model.named_parameters():
                if n.endswith("lora_b"):
                    p.normal_(0.0, 0.01, generator=g)
                elif n.endswith(".m"):  # DoRA's magnitudes: initialised to ||W||_row, moved off it as training would
                    p.mul_(1 + 0.1 * torch.randn(p.shape, device=p.device, generator=g).to(p.dtype))
    model.requires_grad_(False)
    model.eval()
    model.build_cache(inference=True)
    model = model.to(device)
    for layer in model.layers:
        layer.attention.kv_cache.k_cache.normal_(0.0, 1.0, generator=g)
        layer.attention.kv_cache.v_cache.normal_(0.0, 1.0, generator=g)
    return model, cfg


def weight_bytes(model, cfg) -> int:
    """Bytes of weights one decoded token reads: every parameter but the embedding table (one row of it); DoRA's m counts for the
    2 bytes per output row of the cached factor that stands in for it."""
    return cfg.embed_dim * 2 + sum(p.numel() * p.element_size() for n, p in model.named_parameters() if not n.startswith("tok_embeddings"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree whose package is measured")
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--contexts", default="4096")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for p in (args.root, os.path.join(args.root, "llama-x_amd")):
        sys.path.insert(0, p)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("decode_dora_bench: no GPU (there is no CPU path to time)")
    device = torch.device("cuda:0")
    kinds = [k for k in args.models.split(",") if k]
    assert all(k in MODELS for k in kinds), kinds
    contexts = [int(c) for c in args.contexts.split(",")]
    runs = {}
    with torch.no_grad():
        for kind in kinds:
            model, cfg = build(kind, max(contexts), device)
            tok = torch.randint(0, cfg.vocab_size, (1, 1), device=device)
            pos = torch.zeros(1, dtype=torch.int64, device=device)
            import llx.decode as D

            if hasattr(D, "prepare"):
                D.prepare(model)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    model(tok, input_pos=pos)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                logits = model(tok, input_pos=pos)
            runs[kind] = dict(model=model, cfg=cfg, pos=pos, graph=graph, logits=logits, weight_bytes=weight_bytes(model, cfg),
                              ms={c: [] for c in contexts})
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
        d = {"weight_bytes": r["weight_bytes"], "finite_logits": bool(torch.isfinite(r["logits"].float()).all())}
        for ctx in contexts:
            ms = sorted(r["ms"][ctx])
            med = ms[len(ms) // 2]
            kv_bytes = cfg.num_layers * 2 * cfg.num_kv_heads * ctx * cfg.head_dim * 2
            gbs = (r["weight_bytes"] + kv_bytes) / (med * 1e-3) / 1e9
            d[f"ctx{ctx}"] = {"ms_per_token": round(med, 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "tokens_per_s": round(1e3 / med, 1),
                              "kv_bytes": kv_bytes, "algorithmic_bytes": r["weight_bytes"] + kv_bytes, "achieved_gbs": round(gbs, 1),
                              "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
        out["models"][kind] = d
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
