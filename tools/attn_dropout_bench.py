"""What attention dropout costs in the tile loops: forward and backward of the attention call of one layer at 8B heads (H 32, KVH 8,
head_dim 128), S 4096, B 1, causal, with p = 0 (the kernels without dropout) against p = 0.1 (the dropout builds: one 32-bit hash
word per score element in the forward, the dQ and the dK/dV kernel).  Launches alternate between the two in one process; per case
the median of `--rounds` HIP-event times with min and max, forward and backward timed separately.  Writes one JSON record (--out,
default profiles/attn_dropout_bench.json).

    python tools/attn_dropout_bench.py [--rounds 20] [--warmup 3] [--p 0.1] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "llama-x_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--S", type=int, default=4096)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_dropout_bench.json"))
    a = ap.parse_args()
    import torch

    from llx import kernels as K

    dev = torch.device("cuda:0")
    B, S, H, KVH, hd = 1, a.S, 32, 8, 128
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g).bfloat16()  # noqa: E731
    qkv = rn(B, S, (H + 2 * KVH) * hd)  # q, k, v as the views of one row buffer, as the layer passes them
    q = qkv[..., : H * hd].unflatten(-1, (H, hd))
    k = qkv[..., H * hd : (H + KVH) * hd].unflatten(-1, (KVH, hd))
    v = qkv[..., (H + KVH) * hd :].unflatten(-1, (KVH, hd))
    do = rn(B, S, H, hd)
    dqkv = torch.empty_like(qkv)
    dq = dqkv[..., : H * hd].unflatten(-1, (H, hd))
    dk = dqkv[..., H * hd : (H + KVH) * hd].unflatten(-1, (KVH, hd))
    dv = dqkv[..., (H + KVH) * hd :].unflatten(-1, (KVH, hd))
    ticket = torch.tensor([1234, 0], dtype=torch.int64, device=dev)
    cases = {"p0": None, f"p{a.p:g}": (K.attn_dropout_threshold(a.p), ticket, 0)}
    t = {n: {"fwd": [], "bwd": []} for n in cases}
    for it in range(a.warmup + a.rounds):
        for n, drop in cases.items():
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            o, lse = K.attn_fwd(q, k, v, None, dropout=drop)
            e[1].record()
            K.attn_bwd(q, k, v, o, do, lse, dq, dk, dv, None, dropout=drop)
            e[2].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                t[n]["fwd"].append(e[0].elapsed_time(e[1]) * 1e3)
                t[n]["bwd"].append(e[1].elapsed_time(e[2]) * 1e3)
            ticket[1] += 1  # a new mask per round, as a training step draws one
    rec = {"shape": {"B": B, "S": S, "H": H, "KVH": KVH, "head_dim": hd, "mask": "causal"}, "p": a.p, "rounds": a.rounds, "unit": "us",
           "cases": {}}
    for n in cases:
        rec["cases"][n] = {}
        for d in ("fwd", "bwd"):
            rec["cases"][n][d] = {"median": round(statistics.median(t[n][d]), 1), "min": round(min(t[n][d]), 1), "max": round(max(t[n][d]), 1)}
        rec["cases"][n]["fwd_bwd_median"] = round(rec["cases"][n]["fwd"]["median"] + rec["cases"][n]["bwd"]["median"], 1)
    c0, c1 = (rec["cases"][n] for n in cases)
    rec["dropout_over_plain"] = {"fwd": round(c1["fwd"]["median"] / c0["fwd"]["median"], 3), "bwd": round(c1["bwd"]["median"] / c0["bwd"]["median"], 3),
                                 "fwd_bwd": round(c1["fwd_bwd_median"] / c0["fwd_bwd_median"], 3)}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
