"""What a mask-driven attention backward costs: forward + backward of the attention call at 8B heads (H 32, KVH 8), S 4096, B 1 for
  i    MaskSpec()                       the causal rule kernels (index arithmetic only)
  ii   MaskSpec(dense=tril)             the same causal mask given as bytes: the same live tiles, the 64 diagonal tiles per head pay
                                        for the mask bytes (classes 0 and 2 run identical code)
  iii  MaskSpec(dense=window 1024)      a 1024-wide sliding window (causal), which only the dense form can express
Launches alternate between the cases; per case the median of `--rounds` HIP-event times, forward and backward timed separately.  The
yardstick of (ii) is (i) in the same run.  Writes one JSON record (--out, default profiles/attn_mask_bwd_bench.json).

    python tools/attn_mask_bwd_bench.py [--rounds 12] [--warmup 3] [--out FILE]
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
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--S", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_mask_bwd_bench.json"))
    a = ap.parse_args()
    import torch

    from llx import kernels as K

    dev = torch.device("cuda:0")
    B, S, H, KVH, hd, W = 1, a.S, 32, 8, 128, 1024
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
    i = torch.arange(S, device=dev)
    tril = i[:, None] >= i[None, :]
    cases = {
        "rule_causal": K.MaskSpec(),
        "dense_causal": K.MaskSpec(dense=tril),
        "dense_window1024": K.MaskSpec(dense=tril & (i[:, None] - i[None, :] < W)),
    }
    pairs = {"rule_causal": S * (S + 1) // 2, "dense_causal": S * (S + 1) // 2,
             "dense_window1024": int((tril & (i[:, None] - i[None, :] < W)).sum())}
    for ms in cases.values():
        ms.prepared(B, S, dev)  # mask on the device, tile flags built: not part of a step
    t = {n: {"fwd": [], "bwd": []} for n in cases}
    for it in range(a.warmup + a.rounds):
        for n, ms in cases.items():
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            o, lse = K.attn_fwd(q, k, v, ms)
            e[1].record()
            K.attn_bwd(q, k, v, o, do, lse, dq, dk, dv, ms)
            e[2].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                t[n]["fwd"].append(e[0].elapsed_time(e[1]) * 1e3)
                t[n]["bwd"].append(e[1].elapsed_time(e[2]) * 1e3)
    rec = {"shape": {"B": B, "S": S, "H": H, "KVH": KVH, "head_dim": hd}, "rounds": a.rounds, "unit": "us", "cases": {}}
    for n in cases:
        f, b = statistics.median(t[n]["fwd"]), statistics.median(t[n]["bwd"])
        rec["cases"][n] = {"fwd_us": round(f, 1), "bwd_us": round(b, 1), "fwd_bwd_us": round(f + b, 1), "bwd_min_us": round(min(t[n]["bwd"]), 1),
                           "bwd_max_us": round(max(t[n]["bwd"]), 1), "allowed_pairs": pairs[n],
                           "bwd_tflops": round(10.0 * hd * H * pairs[n] / b / 1e6, 1)}  # 5 products of 2 * 128 flops per pair and head
    c = rec["cases"]
    rec["dense_causal_over_rule_causal"] = {"fwd": round(c["dense_causal"]["fwd_us"] / c["rule_causal"]["fwd_us"], 3),
                                            "bwd": round(c["dense_causal"]["bwd_us"] / c["rule_causal"]["bwd_us"], 3),
                                            "fwd_bwd": round(c["dense_causal"]["fwd_bwd_us"] / c["rule_causal"]["fwd_bwd_us"], 3)}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
