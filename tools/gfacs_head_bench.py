"""Times GFACS's log-partition head (csrc/nargnn_logz.hip: rl4co_nargnn_logz_forward + rl4co_nargnn_logz_backward behind one
autograd node) against the same head as torch modules (``Linear(64, 64)``, ``SiLU``, ``Linear(64, Z)``, the reshape and the
mean under autograd) on the same tensors, forward and backward, at the edge-row counts of TSP-100 and TSP-500 with the default
``k_sparse`` and B = 20. Writes profiles/gfacs_head_bench.json.

Both sides are warmed up, then timed alternately (kernel, torch, kernel, ...) with device events around a window of forward +
backward passes, ``--reps`` times; the median, the least and the largest are kept. A window is as many passes as fill
``--window-ms`` (default half a second) at the pace of a first short probe, per side and shape. The times are those of the
whole call under autograd -- four launches, the host's bookkeeping and the allocations included -- not kernel times from a
trace; ``call_share_of_hbm_peak`` is the least traffic (read w, write grad_w, from the shapes; the kernel's backward reads w
twice more: the recompute and the weight gradient) at the HBM peak over that call time. Needs the MI355X: there is no
fall-back.

    python tools/gfacs_head_bench.py [--reps 7] [--window-ms 500] [--out profiles/gfacs_head_bench.json]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = {"tsp100": (20, 100), "tsp500": (20, 500)}  # name -> (B, N); K = max(N // 5, 10)
HBM_PEAK = 8.0e12


def timed(step, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        step()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def summary(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "runs": len(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=500.0)
    ap.add_argument("--z", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gfacs_head_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gfacs_head_bench needs the MI355X")
    from rl4co_amd.nargnn import _LogZHead

    result = {"z_out_dim": args.z, "reps": args.reps, "window_ms": args.window_ms, "pooling": "reference",
              "hbm_peak_bytes_per_s": HBM_PEAK, "shapes": []}
    for name, (b, n) in SHAPES.items():
        k = max(n // 5, 10)
        rows = b * n * k
        gen = torch.Generator().manual_seed(1)
        w = torch.randn(b, n, k, 64, generator=gen).cuda().requires_grad_()
        net = torch.nn.Sequential(torch.nn.Linear(64, 64), torch.nn.SiLU(), torch.nn.Linear(64, args.z)).cuda()
        upstream = (torch.rand(b, args.z, generator=gen) * 2 - 1).cuda()
        params = [net[0].weight, net[0].bias, net[2].weight, net[2].bias]

        def clear():
            for t in [w] + params:
                t.grad = None

        def kernel_step():
            clear()
            _LogZHead.apply(w, *params, b, "reference").backward(upstream)

        def torch_step():
            clear()
            net(w).reshape(-1, b, args.z).mean(0).backward(upstream)

        # the two sides agree before anything is timed
        kernel_step()
        got = [w.grad.clone()] + [p.grad.clone() for p in params]
        torch_step()
        want = [w.grad.clone()] + [p.grad.clone() for p in params]
        gap = max(float((g - t).abs().max() / t.abs().max().clamp_min(1e-30)) for g, t in zip(got, want))
        for _ in range(3):
            kernel_step()
            torch_step()
        torch.cuda.synchronize()
        steps = {"kernel": kernel_step, "torch": torch_step}
        iters = {side: max(20, int(args.window_ms / timed(step, 20)) + 1) for side, step in steps.items()}
        times = {"kernel": [], "torch": []}
        for _ in range(args.reps):
            for side, step in steps.items():
                times[side].append(timed(step, iters[side]))
        least_bytes = 2 * rows * 64 * 4  # read w, write grad_w
        entry = {"name": name, "batch": b, "nodes": n, "k": k, "rows": rows, "kernel": summary(times["kernel"]),
                 "torch": summary(times["torch"]), "passes_per_window": iters, "worst_relative_gap_of_the_gradients": gap,
                 "least_bytes": least_bytes}
        entry["torch_over_kernel"] = entry["torch"]["median_ms"] / entry["kernel"]["median_ms"]
        entry["call_share_of_hbm_peak"] = least_bytes / (entry["kernel"]["median_ms"] * 1e-3) / HBM_PEAK
        result["shapes"].append(entry)
        print(json.dumps(entry))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
