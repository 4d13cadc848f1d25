"""Text generation at 8B dimensions: generate() (one on-device sampler launch per token, no host read inside a token) next to the loop a
user has to write without it - model(...), then softmax / sort / cumsum / multinomial in torch, then .item() - in one process run.

Setup: Llama-3.1-8B dimensions, random weights, prompt 512, 128 new tokens, temperature 0.8, top_k 0, top_p 0.9.  The two loops
alternate, `--repeats` times each after one untimed pass of both; the median is reported.  Both are timed end to end (prefill + the new
tokens, wall clock between device synchronisations); the prefill alone is timed as well, and ms/token is (total - prefill) / new tokens.
The sampler launch alone (device events, `--sampler-steps` launches back to back on one row of real logits) is timed against the
torch chain it replaces on the same logits (the chain without its .item()).  generate(return_logprobs=True) with and without
top_logprobs=8 alternate in the same repeats: what the one extra launch per token (llx_topk_logprobs_rows) costs in ms/token.

    python tools/generate_bench.py [--prompt 512] [--new 128] [--repeats 3] [--layers 32] [--out profiles/generate_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEMPERATURE, TOP_K, TOP_P, SEED = 0.8, 0, 0.9, 1234


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
    model.build_cache(inference=True)
    return model.to(device), cfg


def torch_chain(logits):
    """Temperature + nucleus sampling of one row of logits in torch, as usually written: the token stays on the device."""
    import torch

    probs = torch.softmax(logits.float() / TEMPERATURE, dim=-1)
    sp, si = torch.sort(probs, descending=True)
    cum = torch.cumsum(sp, dim=-1)
    sp = sp.masked_fill(cum - sp > TOP_P, 0.0)
    sp = sp / sp.sum()
    return si[torch.multinomial(sp, 1)]


def host_loop(model, prompt, n):
    """The loop without generate(): prefill, then per token model(...), the torch chain and .item()."""
    import torch

    dev, P = prompt.device, prompt.shape[1]
    with torch.no_grad():
        logits = model(prompt, input_pos=torch.arange(P, device=dev))[0, -1]
        toks = []
        for k in range(n):
            t = torch_chain(logits).item()
            toks.append(t)
            if k == n - 1:
                break
            logits = model(torch.tensor([[t]], device=dev), input_pos=torch.tensor([P + k], device=dev))[0, -1]
    return toks


def timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--sampler-steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "llama-x_amd")):
        sys.path.insert(0, p)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("generate_bench: no GPU (there is no CPU path to time)")
    from llx import kernels as K
    from llx.generate import generate

    dev = torch.device("cuda:0")
    model, cfg = build(args.layers, args.prompt + args.new, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    prompt = torch.randint(0, cfg.vocab_size, (1, args.prompt), device=dev, generator=g)
    P, n = args.prompt, args.new
    torch.manual_seed(0)

    def run_generate():
        return generate(model, prompt, n, temperature=TEMPERATURE, top_k=TOP_K, top_p=TOP_P, seed=SEED)

    def run_logprobs(k):
        return generate(model, prompt, n, temperature=TEMPERATURE, top_k=TOP_K, top_p=TOP_P, seed=SEED, return_logprobs=True, top_logprobs=k)

    def run_prefill():
        with torch.no_grad():
            return model(prompt, input_pos=torch.arange(P, device=dev))

    run_generate(), host_loop(model, prompt, n), run_prefill(), run_logprobs(0), run_logprobs(8)  # untimed pass of everything
    ms = {"generate": [], "host_loop": [], "prefill": [], "generate_logprobs": [], "generate_top_logprobs_8": []}
    for _ in range(args.repeats):
        ms["generate"].append(timed(run_generate)[0])
        ms["generate_logprobs"].append(timed(lambda: run_logprobs(0))[0])
        ms["generate_top_logprobs_8"].append(timed(lambda: run_logprobs(8))[0])
        ms["host_loop"].append(timed(lambda: host_loop(model, prompt, n))[0])
        ms["prefill"].append(timed(run_prefill)[0])

    # the sampler launch alone against the torch chain, on one row of real logits
    with torch.no_grad():
        row = model(prompt[:, :4], input_pos=torch.arange(4, device=dev))[0, -1:].clone()
    pos = torch.zeros(1, dtype=torch.int64, device=dev)
    out = torch.empty(1, dtype=torch.int64, device=dev)

    def events(fn):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.sampler_steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.sampler_steps

    samp, chain = [], []
    for _ in range(args.repeats):
        samp.append(events(lambda: K.sample(row, temperature=TEMPERATURE, top_k=TOP_K, top_p=TOP_P, seed=SEED, pos=pos, out=out, advance=True)))
        chain.append(events(lambda: torch_chain(row[0])))

    pre = median(ms["prefill"])
    res = {"workload": f"Llama-3.1-8B dimensions ({args.layers} layers), random weights, batch 1, prompt {P}, {n} new tokens, "
                       f"temperature {TEMPERATURE}, top_k {TOP_K}, top_p {TOP_P}; medians of {args.repeats} alternating repeats",
           "prefill_ms": round(pre, 3)}
    for name in ("generate", "host_loop", "generate_logprobs", "generate_top_logprobs_8"):
        tot = median(ms[name])
        res[name] = {"total_ms": round(tot, 3), "ms_per_token": round((tot - pre) / n, 4), "all_total_ms": [round(x, 3) for x in ms[name]]}
    res["top_logprobs_8_extra_ms_per_token"] = round(res["generate_top_logprobs_8"]["ms_per_token"] - res["generate_logprobs"]["ms_per_token"], 4)
    res["sampler_kernel_us"] = round(median(samp) * 1e3, 2)
    res["torch_chain_us"] = round(median(chain) * 1e3, 2)
    res["generate_not_slower_than_host_loop"] = res["generate"]["total_ms"] <= res["host_loop"]["total_ms"]
    res["kernel_not_slower_than_torch_chain"] = res["sampler_kernel_us"] <= res["torch_chain_us"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
