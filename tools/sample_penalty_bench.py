"""What the sampler's penalties and log-probabilities cost: the sampler launch alone on Llama-3 rows (V = 128 256, bf16), R = 1 and 16,
temperature 0.8, top_p 0.9, in four arms that alternate in one process:

    plain     llx_sample_rows, as generate() launches it by default
    counts    llx_sample_rows_ext with an int32 [R, V] count table and all three penalties on
    logprob   llx_sample_rows_ext with a log-probability history and no counts
    both      counts and log-probability

Every arm writes its history column, advances nothing (the same position every launch, so every launch does the same work) and, with
counts, starts each timed window from the same seeded table (about 10 % of the tokens seen, as a long sequence leaves it).  A window is
`--steps` launches back to back between two device events; the arms alternate `--repeats` times after a warm-up of every arm; the median
window per arm is reported in microseconds per launch.

    python tools/sample_penalty_bench.py [--steps 200] [--repeats 7] [--out profiles/sample_penalty_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 128_256
TEMPERATURE, TOP_P, SEED = 0.8, 0.9, 1234
PENALTIES = dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25)
ARMS = ("plain", "counts", "logprob", "both")


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "llama-x_amd")):
        sys.path.insert(0, p)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("sample_penalty_bench: no GPU (there is no CPU path to time)")
    from llx import kernels as K

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    res = {"workload": f"sampler launch alone, V {V} bf16, temperature {TEMPERATURE}, top_p {TOP_P}; penalties {PENALTIES}; "
                       f"us per launch, medians of {args.repeats} alternating windows of {args.steps} launches", "rows": {}}
    for R in (1, 16):
        logits = (torch.randn(R, V, device=dev, generator=g) * 2.0).to(torch.bfloat16)
        seen = torch.rand(R, V, device=dev, generator=g) < 0.1
        seed_table = torch.where(seen, torch.randint(1, 6, (R, V), device=dev, generator=g), torch.zeros((), dtype=torch.int64, device=dev)).to(torch.int32)
        table = seed_table.clone()
        pos = torch.full((R,), 1000, dtype=torch.int64, device=dev)
        out = torch.empty(R, dtype=torch.int64, device=dev)
        history = torch.zeros(R, 1, dtype=torch.int64, device=dev)
        logprobs = torch.zeros(R, 1, dtype=torch.float32, device=dev)
        base = dict(temperature=TEMPERATURE, top_p=TOP_P, seed=SEED, pos=pos, out=out, history=history, hist_base=1000)
        kw = {"plain": base, "counts": dict(base, counts=table, **PENALTIES), "logprob": dict(base, logprob_history=logprobs),
              "both": dict(base, counts=table, logprob_history=logprobs, **PENALTIES)}

        def window(arm, steps):
            table.copy_(seed_table)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                K.sample(logits, **kw[arm])
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / steps

        for arm in ARMS:
            window(arm, 10)  # warm-up: code objects, caches
        us = {arm: [] for arm in ARMS}
        for _ in range(args.repeats):
            for arm in ARMS:
                us[arm].append(window(arm, args.steps))
        res["rows"][str(R)] = {arm: {"us": round(median(us[arm]), 2), "all_us": [round(x, 2) for x in us[arm]]} for arm in ARMS}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
