"""What the per-token scoring head costs beside the loss head, at 8B head dimensions (T = 4096 rows, D = 4096, V = 128256; a plain
frozen bf16 head), every row labelled and again with 25 % of the rows labelled (a masked prompt):

  (a) logp      ops.head_logprobs under no_grad (norm -> compacted head GEMM -> llx_logprob_rows_fwd)
  (b) loss      ops.HeadLossFn under no_grad (the loss forward)
  (c) torch     head logits through the package (norm, GEMM over all rows), then torch.log_softmax(logits.float(), -1).gather - the
                route a user had before; with its peak memory (torch.cuda.max_memory_allocated over the arm, above the resident set)
  (d) logp_fb / loss_fb   (a) and (b) with their backward for the frozen plain head (d hidden through the norm)
  (e) logp_top8   (a) with top_k=8: one more launch per logits buffer (llx_topk_logprobs_rows) and the [T, 8] map back
      torch_top8  (c)'s logits, then torch.log_softmax(logits.float(), -1).topk(8): the only route to the alternatives before
      k_rows_fwd / k_topk8   the two row kernels alone on one prebuilt [T, V] logits buffer, every row labelled: what the extra pass of
                  (e) costs against a second llx_logprob_rows_fwd launch over the same rows

The arms alternate in one process; a window is `--iters` back-to-back calls between two HIP events; per arm the median, min and max of
`--windows` windows.  The condition recorded: (a) not slower than (b), and (d) logp_fb not slower than loss_fb, by more than the larger
min-max spread of the two.  Writes one JSON record (--out, default profiles/logprob_bench.json).

    python tools/logprob_bench.py [--windows 5] [--iters 5] [--warmup 2] [--out FILE]
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
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--T", type=int, default=4096)
    ap.add_argument("--D", type=int, default=4096)
    ap.add_argument("--V", type=int, default=128256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logprob_bench.json"))
    a = ap.parse_args()
    import torch

    from llx import kernels as K
    from llx import ops
    from modelling.llama import Linear, RMSNorm

    dev = torch.device("cuda:0")
    T, D, V = a.T, a.D, a.V
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    norm, out = RMSNorm(D, eps=1e-5).bfloat16().to(dev), Linear(D, V, bias=False).bfloat16().to(dev)
    with torch.no_grad():
        out.weight.copy_(torch.randn(V, D, device=dev, generator=g) * 0.02)
    out.weight.requires_grad_(False)
    x = torch.randn(T, D, device=dev, generator=g).bfloat16()
    gout = torch.randn(T, device=dev, generator=g)
    norm.weight.requires_grad_(False)  # (a trainable norm weight would make the loss forward write its gradient pass even under no_grad)

    def plan_args():
        plan = ops.LinearPlan(out)
        return norm.eps, plan, *plan.tensors()

    with torch.no_grad():
        kbuf = out(norm(x))  # the kernels' own arms: one [T, V] bf16 logits buffer, built once
    klb = torch.randint(0, V, (T,), device=dev, generator=g)
    klse = K.logprob_rows_fwd(kbuf, klb)[1]

    def arms(lb):
        def logp():
            with torch.no_grad():
                return ops.head_logprobs(x, norm, out, lb)

        def loss():
            with torch.no_grad():
                return ops.HeadLossFn.apply(x, norm.weight, lb, *plan_args())

        def torch_route():
            with torch.no_grad():
                logits = out(norm(x))
                return torch.where(lb != -100, torch.log_softmax(logits.float(), -1).gather(-1, lb.clamp(min=0)[:, None])[:, 0], 0.0)

        def logp_fb():
            xg = x.detach().requires_grad_()
            ops.head_logprobs(xg, norm, out, lb).backward(gout)

        def loss_fb():
            xg = x.detach().requires_grad_()
            ops.HeadLossFn.apply(xg, norm.weight, lb, *plan_args()).backward()

        def logp_top8():
            with torch.no_grad():
                return ops.head_logprobs(x, norm, out, lb, top_k=8)

        def torch_top8():
            with torch.no_grad():
                return torch.log_softmax(out(norm(x)).float(), -1).topk(8)

        def k_rows_fwd():
            return K.logprob_rows_fwd(kbuf, klb)

        def k_topk8():
            return K.topk_logprobs_rows(kbuf, 8, lse=klse, labels=klb)

        return {"logp": logp, "loss": loss, "torch": torch_route, "logp_fb": logp_fb, "loss_fb": loss_fb, "logp_top8": logp_top8,
                "torch_top8": torch_top8, "k_rows_fwd": k_rows_fwd, "k_topk8": k_topk8}

    rec = {"shape": {"T": T, "D": D, "V": V, "head": "plain bf16, frozen"}, "windows": a.windows, "iters_per_window": a.iters, "unit": "ms", "cases": {}}
    for name, frac in (("all_rows_labelled", 1.0), ("quarter_labelled", 0.25)):
        lb = torch.randint(0, V, (T,), device=dev, generator=g)
        lb[: T - int(T * frac)] = -100  # a masked prompt in front
        fns = arms(lb)
        times = {n: [] for n in fns}
        peak = {}
        for w in range(a.warmup + a.windows):
            for n, fn in fns.items():
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                peak[n] = (torch.cuda.max_memory_allocated() - base) / 2**20
                if w >= a.warmup:
                    times[n].append(e0.elapsed_time(e1) / a.iters)
        case = {n: {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3), "peak_MiB": round(peak[n])}
                for n, t in times.items()}
        for new, old in (("logp", "loss"), ("logp_fb", "loss_fb")):
            spread = max(case[new]["max"] - case[new]["min"], case[old]["max"] - case[old]["min"])
            case[f"{new}_minus_{old}"] = {"ms": round(case[new]["median"] - case[old]["median"], 3), "allowed_ms": round(spread, 3),
                                          "holds": case[new]["median"] - case[old]["median"] <= spread}
        # recorded, no bar: the top-k arm against the plain scoring call, and its kernel against a second row-kernel launch
        case["logp_top8_minus_logp"] = {"ms": round(case["logp_top8"]["median"] - case["logp"]["median"], 3)}
        case["k_topk8_minus_k_rows_fwd"] = {"ms": round(case["k_topk8"]["median"] - case["k_rows_fwd"]["median"], 3)}
        rec["cases"][name] = case
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
