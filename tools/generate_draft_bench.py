"""Greedy generate() with prompt-lookup drafts at 8B dimensions: what a k + 1-row decode step costs next to the one-row step, and what
the drafting loop gains on the model's own text - all arms alternating in one process run.

Setup: Llama-3.1-8B dimensions, random weights (bf16; --int8 weight-only | dynamic: the layers quantised with quantize_linear_, the head
bf16), batch 1, prompt 512, 256 new tokens, greedy, n-gram 3.  The arms draft_tokens = 0 (the plain loop), 1, 2 and 3 alternate,
`--rounds` times each after one untimed pass of all; medians are reported.  Each arm is timed end to end (wall clock between device
synchronisations); the prefill alone is timed as well.

Two kinds of figures:
  ms_per_step     (total - prefill) / decode steps launched (stats["launched"], the frozen ones behind the end included).  This does not
                  depend on the text: a step costs the same whatever it confirms.  break_even = ms_per_step(k) / ms_per_step(0) - 1 is the
                  number of draft tokens a step must have confirmed on average for the arm to match the plain loop.
  tokens_per_step, ms_per_token, tokens_per_s
                  on the model's own greedy continuation of a random prompt.  That says nothing about real text: random weights
                  either never repeat (8B dimensions, 256 tokens: no draft confirmed, the figures are the pure cost of drafting) or fall
                  into a loop where every draft is confirmed (the tiny test model).

    python tools/generate_draft_bench.py [--int8 weight-only|dynamic] [--prompt 512] [--new 256] [--rounds 3] [--layers 32] [--out profiles/generate_draft_bench.json]

The result of a run is stored under its weight kind in the output file; the other kinds already there are kept.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
NGRAM = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--int8", choices=("weight-only", "dynamic"), default=None)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_draft_bench.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "llama-x_amd")):
        sys.path.insert(0, p)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("generate_draft_bench: no GPU (there is no CPU path to time)")
    from generate_bench import build, median, timed
    from llx.generate import generate

    dev = torch.device("cuda:0")
    P, n = args.prompt, args.new
    model, cfg = build(args.layers, P + n + 3, dev)
    kind = "bf16"
    if args.int8:
        from subclasses import quantize_linear_

        quantize_linear_(model.layers, "int8", dynamic_int8_act=args.int8 == "dynamic")
        kind = f"int8-{args.int8}"
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    prompt = torch.randint(0, cfg.vocab_size, (1, P), device=dev, generator=g)
    arms = (0, 1, 2, 3)

    def run(k):
        stats = {}
        out = generate(model, prompt, n, draft_tokens=k, draft_ngram=NGRAM, stats=stats)
        stats.pop("state", None)
        return out, stats

    def run_prefill():
        with torch.no_grad():
            return model(prompt, input_pos=torch.arange(P, device=dev))

    outs = {k: run(k)[0] for k in arms}  # untimed pass of everything
    run_prefill()
    ms = {k: [] for k in arms}
    stats, pre = {}, []
    for _ in range(args.rounds):
        for k in arms:
            t, (_, stats[k]) = timed(lambda: run(k))
            ms[k].append(t)
        pre.append(timed(run_prefill)[0])
    pre = median(pre)
    same = {k: int((outs[k][0] == outs[0][0]).long().cumprod(0).sum()) for k in arms}  # tokens up to the first difference from the plain loop
    res = {"workload": f"Llama-3.1-8B dimensions ({args.layers} layers), random weights, {kind} layers, batch 1, prompt {P}, {n} new tokens, greedy, "
                       f"n-gram {NGRAM}; medians of {args.rounds} alternating rounds; tokens/step and tokens/s are on the model's own greedy "
                       "text, ms/step does not depend on the text",
           "prefill_ms": round(pre, 3), "arms": {}}
    for k in arms:
        tot, s = median(ms[k]), stats[k]
        dec = tot - pre
        res["arms"][str(k)] = {"draft_tokens_ran": s["draft_tokens"], "total_ms": round(tot, 3), "all_total_ms": [round(x, 3) for x in ms[k]],
                               "steps_launched": s["launched"], "ms_per_step": round(dec / max(1, s["launched"]), 4), "steps": s["steps"],
                               "tokens": s["tokens"], "tokens_per_step": round(s["tokens"] / s["steps"], 3),
                               "ms_per_token": round(dec / s["tokens"], 4), "tokens_per_s": round(1e3 * s["tokens"] / dec, 1),
                               "tokens_equal_to_plain_loop": same[k]}
    base = res["arms"]["0"]["ms_per_step"]
    for k in arms[1:]:
        a = res["arms"][str(k)]
        a["step_cost_over_plain"] = round(a["ms_per_step"] / base, 4)
        a["break_even_accepted_per_step"] = round(a["ms_per_step"] / base - 1, 4)
    print(json.dumps({kind: res}))
    allres = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            allres = json.load(f)
    allres[kind] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(allres, indent=1) + "\n")


if __name__ == "__main__":
    main()
