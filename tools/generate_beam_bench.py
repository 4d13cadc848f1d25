"""Beam search at 8B dimensions: what a decode step of generate(num_beams=W) costs next to the batched greedy step of the same W rows, and
what the three launches of csrc/beam.hip cost alone.

Setup: Llama-3.1-8B dimensions, random weights, max_seq_len 8192, a prompt of `--prompt` tokens, W = 2, 4, 8, 16.  Three windows alternate
in one process, `--rounds` times each after an untimed pass; medians with min-max of ms per step over `--steps` steps between device events:
  (a) the beam step: model(tok [W, 1], input_pos=[pos]) + llx_beam_rows + llx_beam_merge + llx_kv_reorder_rows, the parents being whatever
      the search picks on this model;
  (b) the batched greedy step at B = W: model(tok [W, 1], input_pos=pos[:, None]) + the sampler launch (the loop of _generate_batch);
  (c) the batch-1 greedy step.
`beam_over_batched` = (a) / (b); `reorder_share` = the cache reorder alone at len = prompt, every slot moving, over (a) - (b).
The three launches alone, between device events, at len = 1024 and 4096 (the reorder with parent[b] = (b + 1) % W: every slot moves, and
with identity parents: nothing moves), median of `--kernel-rounds`.

    python tools/generate_beam_bench.py [--prompt 512] [--steps 48] [--rounds 5] [--layers 32] [--out profiles/generate_beam_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEAMS = (2, 4, 8, 16)
LENS = (1024, 4096)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--kernel-rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_beam_bench.json"))
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "llama-x_amd"), os.path.join(ROOT, "tools")):
        sys.path.insert(0, p)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("generate_beam_bench: no GPU (there is no CPU path to time)")
    from generate_batch_bench import build, caches_for, install, stats
    from llx import kernels as K
    from llx.generate import prefill

    dev = torch.device("cuda:0")
    model, cfg = build(args.layers, 8192, dev)
    model.build_cache(inference=True)
    model = model.to(dev)
    P, V = args.prompt, cfg.vocab_size
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    prompt = torch.randint(0, V, (1, P), device=dev, generator=g)
    res = {"workload": f"Llama-3.1-8B dimensions ({args.layers} layers), random weights, max_seq_len 8192, a prompt of {P} tokens; ms per decode "
                       f"step, medians (min-max) of {args.rounds} alternating rounds of {args.steps} steps", "beams": {}, "launches_us": {}}

    def events(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def beam_state(W, n):
        z = lambda *shape, dt: torch.zeros(*shape, device=dev, dtype=dt)  # noqa: E731
        return [z(W, W + 1, dt=torch.float32), z(W, W + 1, dt=torch.int32), z(W, dt=torch.float32), z(W, dt=torch.int32), z(W, 1, dt=torch.int64),
                z(W, n, dt=torch.int64), z(W, n, dt=torch.int64), z(W, dt=torch.int32), z(W, dt=torch.float32), z(3, dt=torch.int32)]

    one = caches_for(model, cfg, 1, dev)
    for W in BEAMS:
        many = caches_for(model, cfg, W, dev)
        table = K.kv_cache_table(c for kv in many for c in (kv.k_cache, kv.v_cache))
        n = 4 * args.steps  # the budget never ends the search inside a window
        rows = prompt.expand(W, -1).contiguous()

        def beam_ms():
            install(model, many)
            st = beam_state(W, n)
            logits = prefill(model, rows)[:, 0]
            K.beam_rows(logits, st[0], st[1])
            K.beam_merge(*st, n=n, init=True)
            pos = torch.arange(P, P + n, device=dev)
            k = [0]

            def step():
                k[0] += 1
                K.beam_rows(model(st[4], input_pos=pos[k[0] - 1 : k[0]])[:, 0], st[0], st[1])
                K.beam_merge(*st, n=n)
                K.kv_reorder_rows(table, st[3], P + k[0])

            step()
            return events(step, args.steps)

        def greedy_ms(B):
            install(model, many if B > 1 else one)
            logits = prefill(model, rows[:B])
            pos = torch.full((B,), P - 1, device=dev, dtype=torch.int64)
            tok = torch.empty(B, 1, device=dev, dtype=torch.int64)
            kw = dict(temperature=0.0, pos=pos, out=tok.view(B), advance=True)
            K.sample(logits[:, 0], **kw)

            def step():
                K.sample(model(tok, input_pos=pos[:, None])[:, 0], **kw)

            step()
            return events(step, args.steps)

        ms = {"beam": [], "batched": [], "single": []}
        with torch.no_grad():
            beam_ms(), greedy_ms(W), greedy_ms(1)  # untimed pass
            for _ in range(args.rounds):
                ms["beam"].append(beam_ms())
                ms["batched"].append(greedy_ms(W))
                ms["single"].append(greedy_ms(1))

        # ---- the three launches alone
        launches = {}
        logits = torch.randn(W, V, device=dev, generator=g).bfloat16()
        st = beam_state(W, 8192)
        K.beam_rows(logits, st[0], st[1])
        K.beam_merge(*st, n=8192, init=True)
        shift = torch.tensor([(b + 1) % W for b in range(W)], device=dev, dtype=torch.int32)
        ident = torch.arange(W, device=dev, dtype=torch.int32)
        fns = {"beam_rows": lambda L: K.beam_rows(logits, st[0], st[1]), "beam_merge": lambda L: K.beam_merge(*st, n=8192),
               "kv_reorder_rows (every slot moves)": lambda L: K.kv_reorder_rows(table, shift, L),
               "kv_reorder_rows (identity)": lambda L: K.kv_reorder_rows(table, ident, L)}
        moved = {}
        for L in LENS + (P,):
            for name, fn in fns.items():
                fn(L)
                t = stats([events(lambda: fn(L), 1) * 1e3 for _ in range(args.kernel_rounds)])
                if L in LENS:
                    launches[f"{name} len={L}"] = t
                if name.startswith("kv_reorder_rows (every"):
                    moved[L] = t["median"]
                    if L in LENS:
                        nbytes = 2 * len(many) * W * cfg.num_kv_heads * L * 128 * 2
                        launches[f"{name} len={L}"]["GBps_read_plus_written"] = round(2 * nbytes / (t["median"] * 1e-6) / 1e9, 1)
        res["launches_us"][str(W)] = launches
        a, b, c = stats(ms["beam"]), stats(ms["batched"]), stats(ms["single"])
        gap = a["median"] - b["median"]
        res["beams"][str(W)] = {"beam_step_ms": a, "batched_greedy_step_ms": b, "single_greedy_step_ms": c,
                                "beam_over_batched": round(a["median"] / b["median"], 3), "beam_minus_batched_ms": round(gap, 4),
                                "reorder_alone_ms_at_prompt_len": round(moved[P] * 1e-3, 4),
                                "reorder_share": round(moved[P] * 1e-3 / gap, 2) if gap > 0 else None}
        print(f"W={W}: {json.dumps(res['beams'][str(W)])} {json.dumps(launches)}", file=sys.stderr, flush=True)
        del many, table
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
