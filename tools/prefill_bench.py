"""KV-cache prefill of the 8B model: a prompt into the cache through Llama.forward(x, input_pos=...), and its attention call alone.

8B dimensions, random weights, max_seq_len 8192, batch 1.  Model cases (public model API only, so the script runs unchanged on a
tree without the mask-driven prefill kernel: `--root` = that tree):
  a  one 4096-token prompt                 ms per call, prompt tokens/s
  b  the same prompt as 8 chunks of 512    ms for the 8 calls, prompt tokens/s
  c  8 tokens at position 4096             ms per call (the first shape past the decode path)
Attention cases (d), at the layer's shapes (q the view of a q|k|v row buffer, the caches [1, 8, 8192, 128], mask = tril[pos]): the
mask-driven MFMA kernel (K.attn_mask_fwd, with its tile-flag pass timed separately; absent on an older tree), the per-row kernel
(K.attn_dense_fwd plus the [B,H,L,hd] -> rows copy its route makes), and K.attn_fwd causal at S = 4096 beside (a): the same key
tiles, so the ratio says what the mask bytes and the flags cost.

The timed windows alternate between the cases, `--rounds` times; per case the median round is reported with the min-max spread.
Device events around calls that end in a synchronise.  FLOPs and bytes are computed from the shapes: linears 2 * tokens * weights,
attention 4 * 128 * H * (allowed query-key pairs); bytes = weights once per call + K/V rows read once per call + mask bytes.
`--layers` shortens the model (the per-layer work is what differs between trees); the result records it.

    python tools/prefill_bench.py [--root TREE] [--layers 32] [--cases a,b,c,d] [--steps 3] [--warmup 1] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys

PROMPT, CHUNK, SMAX, TAIL = 4096, 512, 8192, 8
H, KVH, HD = 32, 8, 128


def build(layers: int, device):
    import torch
    from modelling import Llama, LlamaConfig

    cfg = LlamaConfig(embed_dim=4096, num_layers=layers, head_dim=HD, num_heads=H, num_kv_heads=KVH, intermediate_dim=14336, max_seq_len=SMAX,
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
    model.build_cache(inference=True)
    return model.to(device), cfg


def pairs(lo: int, hi: int) -> int:
    """Allowed query-key pairs of tril rows lo..hi-1."""
    return sum(p + 1 for p in range(lo, hi))


def model_cost(cfg, calls):
    """(FLOPs, bytes) of a list of (lo, hi) prefill calls: every linear of every layer and the head on all tokens, attention on the
    allowed pairs; weights and the live K/V rows read once per call, the mask bytes once per call."""
    per_layer_w = cfg.embed_dim * (H + 2 * KVH) * HD + H * HD * cfg.embed_dim + 3 * cfg.embed_dim * cfg.intermediate_dim
    head_w = cfg.embed_dim * cfg.vocab_size
    flops = byts = 0
    for lo, hi in calls:
        n = hi - lo
        flops += 2 * n * (cfg.num_layers * per_layer_w + head_w) + cfg.num_layers * 4 * HD * H * pairs(lo, hi)
        byts += 2 * (cfg.num_layers * per_layer_w + head_w) + cfg.num_layers * 2 * KVH * hi * HD * 2 + n * SMAX
    return flops, byts


def timed(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def stats(ms):
    ms = sorted(ms)
    return {"ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree whose package is measured")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--cases", default="a,b,c,d")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for p in (args.root, os.path.join(args.root, "llama-x_amd")):
        sys.path.insert(0, p)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("prefill_bench: no GPU (there is no CPU path to time)")
    from llx import kernels as K

    device = torch.device("cuda:0")
    cases = [c for c in args.cases.split(",") if c]
    has_new = hasattr(K, "attn_mask_fwd")
    fns, meta = {}, {}
    with torch.no_grad():
        if set(cases) & {"a", "b", "c"}:
            model, cfg = build(args.layers, device)
            tokens = torch.randint(0, cfg.vocab_size, (1, PROMPT + TAIL), device=device)
            calls = {"a": [(0, PROMPT)], "b": [(lo, lo + CHUNK) for lo in range(0, PROMPT, CHUNK)], "c": [(PROMPT, PROMPT + TAIL)]}
            last = {}

            def run(name):
                for lo, hi in calls[name]:
                    last[name] = model(tokens[:, lo:hi], input_pos=torch.arange(lo, hi, device=device))

            for name in ("a", "b", "c"):
                if name in cases:
                    fns[name] = (lambda n=name: run(n))
                    fl, by = model_cost(cfg, calls[name])
                    meta[name] = {"tokens": sum(hi - lo for lo, hi in calls[name]), "calls": len(calls[name]), "flops": fl, "bytes": by}
        if "d" in cases:
            g = torch.Generator(device=device)
            g.manual_seed(7)
            kc = torch.randn(1, KVH, SMAX, HD, device=device, generator=g).bfloat16()
            vc = torch.randn(1, KVH, SMAX, HD, device=device, generator=g).bfloat16()
            tril = torch.ones(SMAX, SMAX, dtype=torch.bool, device=device).tril()
            rows = torch.randn(1, PROMPT, (H + 2 * KVH) * HD, device=device, generator=g).bfloat16()
            shapes = {"a": [(0, PROMPT)], "b": [(lo, lo + CHUNK) for lo in range(0, PROMPT, CHUNK)], "c": [(PROMPT, PROMPT + TAIL)]}
            for name, spans in shapes.items():
                ops_ = []
                for lo, hi in spans:
                    q = rows[:, : hi - lo, : H * HD].unflatten(-1, (H, HD)).transpose(1, 2)
                    mask = tril[None, None, torch.arange(lo, hi, device=device)]
                    ops_.append((q, mask))
                fl = 4 * HD * H * sum(pairs(lo, hi) for lo, hi in spans)
                by = sum(2 * KVH * hi * HD * 2 + 2 * (hi - lo) * H * HD * 2 + (hi - lo) * SMAX for lo, hi in spans)
                if has_new:
                    fns[f"d_{name}_mask_fwd"] = (lambda o=ops_: [K.attn_mask_fwd(q, kc, vc, m) for q, m in o])
                    fns[f"d_{name}_mask_flags"] = (lambda o=ops_: [K.attn_mask_flags(m, 1) for _, m in o])
                    meta[f"d_{name}_mask_fwd"] = {"flops": fl, "bytes": by, "calls": len(spans)}
                    meta[f"d_{name}_mask_flags"] = {"bytes": sum((hi - lo) * SMAX for lo, hi in spans), "calls": len(spans)}
                fns[f"d_{name}_dense_fwd"] = (lambda o=ops_: [K.attn_dense_fwd(q, kc, vc, m).transpose(1, 2).reshape(q.shape[2], H * HD) for q, m in o])
                meta[f"d_{name}_dense_fwd"] = {"flops": fl, "bytes": by, "calls": len(spans)}
            qkv = rows.view(1, PROMPT, H + 2 * KVH, HD)
            fns["d_a_causal_attn_fwd"] = lambda: K.attn_fwd(qkv[:, :, :H], qkv[:, :, H : H + KVH], qkv[:, :, H + KVH :])
            meta["d_a_causal_attn_fwd"] = {"flops": 4 * HD * H * pairs(0, PROMPT), "calls": 1}
        ms = {n: [] for n in fns}
        for _ in range(args.rounds):
            for n, fn in fns.items():
                ms[n].append(timed(torch, fn, args.steps, args.warmup))
    out = {"workload": f"Llama-3.1-8B dimensions, {args.layers} layers, KV-cache prefill (batch 1, max_seq_len {SMAX}), random-init weights",
           "label": args.label, "root": os.path.abspath(args.root), "mask_kernel": has_new, "layers": args.layers, "steps": args.steps,
           "warmup": args.warmup, "rounds": args.rounds, "cases": {}}
    for n in fns:
        d = {**stats(ms[n]), **meta[n]}
        if "tokens" in d:
            d["prompt_tokens_per_s"] = round(d["tokens"] / (d["ms"] * 1e-3), 1)
        if "flops" in d:
            d["tflops"] = round(d["flops"] / (d["ms"] * 1e-3) / 1e12, 2)
        if "bytes" in d:
            d["gbs"] = round(d["bytes"] / (d["ms"] * 1e-3) / 1e9, 1)
        out["cases"][n] = d
    c = out["cases"]
    if "d_a_mask_fwd" in c and "d_a_causal_attn_fwd" in c:
        out["mask_fwd_over_causal_fwd_at_4096"] = round(c["d_a_mask_fwd"]["ms"] / c["d_a_causal_attn_fwd"]["ms"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
