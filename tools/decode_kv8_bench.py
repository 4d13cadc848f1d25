"""Decode steps of the 8B model with an FP8 (E4M3) KV cache next to the bf16 cache of the same model, in one process run.

As tools/decode_mxfp4_bench.py: 8B dimensions, random weights, one hipGraph replay per step, device events around the replays.  Per
setting (weights, batch, context) ONE model carries two sets of caches, kv_dtype "bf16" and "fp8"; both steps are captured first and the
timed windows then alternate between the arms, `--rounds` times, so that a drift of the machine hits both alike; the median round is
reported with the min-max spread.  Next to each ratio stands the prediction from byte counts: (weights + fp8 K/V) / (weights + bf16 K/V).
Also timed, alternating in the same way: the attention launch pair alone (attn_decode walking the layers' caches, so that the keys
and values come from HBM as in a step, 20 x `--steps` calls per window) at every setting's shape, and
a 4096-token prefill (what the per-layer transient bf16 image of an fp8 cache costs).  Last, how far the fp8 cache moves the model: a
128-token prompt and 64 teacher-forced decode steps on both caches of the bf16-weight model - the largest max-norm relative deviation of
a step's logits and the share of steps with the same greedy token.  Recorded, not asserted.

    python tools/decode_kv8_bench.py [--settings bf16:1:4096,mxfp4:1:4096,bf16:16:4096,bf16:1:32768] [--steps 50] [--warmup 10] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys

SETTINGS = "bf16:1:4096,mxfp4:1:4096,bf16:16:4096,bf16:1:32768"
ARMS = ("bf16", "fp8")


def build(kind: str, device):
    import torch
    from modelling import Llama, LlamaConfig
    from subclasses import quantize_linear_

    cfg = LlamaConfig(embed_dim=4096, num_layers=32, head_dim=128, num_heads=32, num_kv_heads=8, intermediate_dim=14336, max_seq_len=4096,
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
    if kind == "mxfp4":
        quantize_linear_(model.layers, "mxfp4")
    model.requires_grad_(False)
    return model.eval()


def caches(model, batch: int, seq: int, device) -> dict:
    """arm -> the model's KVCache modules of that kind (rope table and causal mask rebuilt for `seq`), filled with the same N(0, 1) values."""
    import torch
    from llx import kernels as K

    model.config = model.config._replace(max_seq_len=seq)
    out = {}
    g = torch.Generator(device=device)
    for arm in ARMS:
        with torch.device(device):
            model.build_cache(inference=True, batch_size=batch, kv_dtype=arm)
        out[arm] = [layer.attention.kv_cache for layer in model.layers]
    pos = torch.arange(seq, device=device)
    for lb, lf in zip(out["bf16"], out["fp8"]):
        g.manual_seed(99)
        lb.k_cache.normal_(0.0, 1.0, generator=g)
        lb.v_cache.normal_(0.0, 1.0, generator=g)
        K.kv_scatter(lb.k_cache, lb.v_cache, lf.k_cache, lf.v_cache, pos)
    return out


def use(model, arm_caches) -> None:
    for layer, c in zip(model.layers, arm_caches):
        layer.attention.kv_cache = c


def timed(fn, steps: int, warmup: int) -> float:
    import torch

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


def med(xs):
    xs = sorted(xs)
    return {"ms": round(xs[len(xs) // 2], 4), "min_ms": round(xs[0], 4), "max_ms": round(xs[-1], 4)}


def weight_bytes(model, cfg) -> int:
    from subclasses import MXFP4LinearWeight

    total = cfg.embed_dim * 2
    for n, p in model.named_parameters():
        if n.startswith("tok_embeddings"):
            continue
        total += p.packed.numel() + p.scale.numel() if isinstance(p, MXFP4LinearWeight) else p.numel() * p.element_size()
    return total


def fidelity(model, device, prompt_len=128, steps=64) -> dict:
    import torch

    cs = caches(model, 1, 512, device)
    for arm in ARMS:
        for c in cs[arm]:
            c.k_cache.zero_(), c.v_cache.zero_()
    g = torch.Generator(device=device)
    g.manual_seed(7)
    prompt = torch.randint(0, model.config.vocab_size, (1, prompt_len), device=device, generator=g)
    last = {}
    for arm in ARMS:
        use(model, cs[arm])
        last[arm] = model(prompt, input_pos=torch.arange(prompt_len, device=device))[:, -1].float()
    dev_max, same = 0.0, 0
    for s in range(steps):
        dev_max = max(dev_max, ((last["fp8"] - last["bf16"]).abs().max() / last["bf16"].abs().max()).item())
        tok = last["bf16"].argmax(-1)
        same += int((last["fp8"].argmax(-1) == tok).item())
        for arm in ARMS:  # teacher-forced with the bf16 arm's greedy token: the arms stay comparable step by step
            use(model, cs[arm])
            last[arm] = model(tok.view(1, 1), input_pos=torch.tensor([prompt_len + s], device=device))[:, 0].float()
    return {"prompt_tokens": prompt_len, "steps": steps, "max_rel_logit_deviation": round(dev_max, 5), "greedy_agreement": round(same / steps, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default=SETTINGS)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--prefill", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "llama-x_amd")):
        sys.path.insert(0, p)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("decode_kv8_bench: no GPU (there is no CPU path to time)")
    import llx.decode as D
    from llx import kernels as K

    device = torch.device("cuda:0")
    settings = [(w, int(b), int(c)) for w, b, c in (s.split(":") for s in args.settings.split(",") if s)]
    out = {"workload": "Llama-3.1-8B decode step, random-init weights, bf16 against fp8 (E4M3) KV cache, one hipGraph replay per step",
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "settings": []}
    with torch.no_grad():
        for kind in dict.fromkeys(w for w, _, _ in settings):
            model = build(kind, device)
            cfg = model.config
            wb = weight_bytes(model, cfg)
            for _, B, ctx in [s for s in settings if s[0] == kind]:
                cs = caches(model, B, ctx, device)
                tok = torch.randint(0, cfg.vocab_size, (B, 1), device=device)
                pos = torch.full((B, 1) if B > 1 else (1,), ctx - 1, dtype=torch.int64, device=device)
                graphs, fast = {}, {}
                for arm in ARMS:
                    use(model, cs[arm])
                    fast[arm] = bool(D.layer_ok(model.layers[0], model.tok_embeddings(tok), model._inference_mask(B, pos)))
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        for _ in range(2):
                            model(tok, input_pos=pos)
                    torch.cuda.current_stream().wait_stream(side)
                    graphs[arm] = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graphs[arm]):
                        model(tok, input_pos=pos)
                # the attention launch pair alone, walking the 32 layers' caches (20 x steps calls per window: a call is tens of microseconds)
                q = torch.randn(B, cfg.num_heads, 1, 128, device=device, dtype=torch.bfloat16)
                mask = model._inference_mask(B, pos)
                ext = K.mask_extent(mask)
                step_ms, attn_ms = {a: [] for a in ARMS}, {a: [] for a in ARMS}
                for _ in range(args.rounds):
                    for arm in ARMS:
                        step_ms[arm].append(timed(graphs[arm].replay, args.steps, args.warmup))
                    for arm in ARMS:
                        turn = [0]

                        def pair(layers=cs[arm]):  # the layers' caches in turn, as a step reads them: 32 of them exceed the last-level cache
                            c = layers[turn[0] % len(layers)]
                            turn[0] += 1
                            K.attn_decode(q, c.k_cache, c.v_cache, mask, ext)

                        attn_ms[arm].append(timed(pair, 20 * args.steps, 2 * len(cs[arm])))
                kv = cfg.num_layers * 2 * cfg.num_kv_heads * ctx * cfg.head_dim * B
                rec = {"weights": kind, "batch": B, "context": ctx, "weight_bytes": wb, "kv_bytes": {"bf16": 2 * kv, "fp8": kv},
                       "decode_fast_path": fast, "step": {a: med(step_ms[a]) for a in ARMS}, "attention_pair": {a: med(attn_ms[a]) for a in ARMS},
                       "predicted_step_ratio": round((wb + kv) / (wb + 2 * kv), 4), "predicted_attention_ratio": 0.5}
                rec["measured_step_ratio"] = round(rec["step"]["fp8"]["ms"] / rec["step"]["bf16"]["ms"], 4)
                rec["measured_attention_ratio"] = round(rec["attention_pair"]["fp8"]["ms"] / rec["attention_pair"]["bf16"]["ms"], 4)
                out["settings"].append(rec)
                print(json.dumps(rec), flush=True)
                del graphs, cs
                torch.cuda.empty_cache()
            if kind == "bf16":
                cs = caches(model, 1, args.prefill, device)
                prompt = torch.randint(0, cfg.vocab_size, (1, args.prefill), device=device)
                ppos = torch.arange(args.prefill, device=device)
                pre = {a: [] for a in ARMS}
                for _ in range(3):
                    for arm in ARMS:
                        use(model, cs[arm])
                        pre[arm].append(timed(lambda: model(prompt, input_pos=ppos), 2, 1))
                out["prefill"] = {"tokens": args.prefill, **{a: med(pre[a]) for a in ARMS}}
                out["prefill"]["image_cost_ms_per_layer"] = round((out["prefill"]["fp8"]["ms"] - out["prefill"]["bf16"]["ms"]) / cfg.num_layers, 4)
                print(json.dumps(out["prefill"]), flush=True)
                del cs
                torch.cuda.empty_cache()
                out["fidelity"] = fidelity(model, device)
                print(json.dumps(out["fidelity"]), flush=True)
            del model
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
