"""Time of DeepACO's heatmap encoder for the depot graphs (rl4co_amd.NARGNNDepotEncoder on csrc/nargnn_depot.hip) at the
reference's depth (15 GNN layers, 5 heatmap-MLP layers, width 64) on CVRP-50 x 4096 (N = 51, K = 10) and CVRP-100 x 1024
(N = 101, K = 20). Two legs per shape, alternating round by round after one warm-up round, each timed with HIP events
around the whole call and synchronised:
  kernel   NARGNNDepotEncoder.forward: graph construction by torch ops, then ONE rl4co_nargnn_depot_heatmap launch
  torch    the fp32 edge-list restatement of tests/nargnn_depot_ref.py from torch ops on the same card (graph
           construction included). This flatters the reference, which builds its graphs one instance at a time in Python.
Per shape: median / min / max of each leg, the ratio of the medians, the FLOP count (2 D D (4 N + R) per GNN layer,
2 D D R per MLP layer, R = (N - 1)(K + 2) edge rows) as a share of the card's fp32 MFMA peak, and the TSP kernel's time at
the same customers and K from profiles/nargnn_bench.json scaled by the row count R / (N_tsp K): what the irregular layout
costs. One more line: the whole DeepACOPolicy call (48 ants, 10 iterations) at CVRP-100 x 256 with the encoder's share.

    python tools/nargnn_depot_bench.py [--reps 5] [--out profiles/nargnn_depot_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rl4co_amd import DeepACOPolicy, NARGNNDepotEncoder  # noqa: E402
from rl4co_amd import kernels as K  # noqa: E402
from rl4co_amd.envs import get_env  # noqa: E402
from tests import nargnn_depot_ref as R  # noqa: E402

FP32_MFMA_PEAK = 157.3e12  # MI355X, fp32 matrix, FLOP/s (vendor figure)
SHAPES = [(50, 4096), (100, 1024)]  # (customers, batch)
LAYERS, MLP_LAYERS, D = 15, 5, 64


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end)


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": len(ms)}


def tsp_yardstick(customers, batch, k, rows):
    """The TSP kernel's recorded median at (num_loc, batch, k), scaled by the row count; None when not recorded."""
    path = os.path.join(ROOT, "profiles", "nargnn_bench.json")
    if not os.path.exists(path):
        return None
    for row in json.load(open(path))["shapes"]:
        if (row["num_loc"], row["batch"], row["k"]) == (customers, batch, k):
            return {"tsp_median_ms": row["kernel"]["median_ms"], "row_ratio": rows / (customers * k),
                    "scaled_ms": row["kernel"]["median_ms"] * rows / (customers * k)}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/nargnn_depot_bench.json")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sd = R.make_state_dict("cvrp", 1, LAYERS, MLP_LAYERS)
    enc = NARGNNDepotEncoder(env_name="cvrp").eval()
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    result = {"env": "cvrp", "layers": LAYERS, "mlp_layers": MLP_LAYERS, "reps": args.reps,
              "fp32_mfma_peak_flops": FP32_MFMA_PEAK, "shapes": []}
    for customers, b in SHAPES:
        n = customers + 1
        k = R.num_neighbors(n)
        rows = customers * (k + 2)
        locs, feats = (t.to(dev) for t in R.make_instance("cvrp", b, n, n + b))
        td = {"locs": locs, "demand": feats[..., 0].contiguous()}
        legs = {"kernel": lambda: enc(td), "torch": lambda: R.encode(sd_dev, locs, feats, dtype=torch.float32)}
        with torch.no_grad():
            for fn in legs.values():  # warm-up round
                fn()
            times = {name: [] for name in legs}
            for _ in range(args.reps):
                for name, fn in legs.items():
                    times[name].append(timed(fn))
            diff = float((enc(td)[0] - R.encode(sd_dev, locs, feats, dtype=torch.float32)[0]).abs().max())
        flop = b * (LAYERS * 2 * D * D * (4 * n + rows) + (MLP_LAYERS - 1) * 2 * D * D * rows + 2 * D * rows)
        row = {"num_loc": customers, "nodes": n, "batch": b, "k": k, "edge_rows": rows,
               "tier": "lds" if n <= K.nargnn_depot_lds_nodes(k) else "scratch", "kernel": spread(times["kernel"]),
               "torch": spread(times["torch"]), "flop": flop, "max_abs_diff_vs_torch": diff,
               "tsp_kernel_scaled_by_rows": tsp_yardstick(customers, b, k, rows)}
        row["speedup"] = row["torch"]["median_ms"] / row["kernel"]["median_ms"]
        row["share_of_fp32_mfma_peak"] = flop / (row["kernel"]["median_ms"] * 1e-3) / FP32_MFMA_PEAK
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
        del locs, feats, td, legs
        torch.cuda.empty_cache()
    # the whole policy call
    torch.manual_seed(0)
    env = get_env("cvrp", generator_params=dict(num_loc=100))
    td = env.reset(batch_size=[256])
    pol = DeepACOPolicy(env_name="cvrp").eval()
    pol.encoder.load_state_dict(sd, strict=True)
    pol = pol.to(dev)
    pol(td, env, phase="test")
    whole = [timed(lambda: pol(td, env, phase="test")) for _ in range(args.reps)]
    alone = [timed(lambda: pol.encoder(td)) for _ in range(args.reps)]
    row = {"num_loc": 100, "batch": 256, "n_ants": 48, "n_iterations": 10, "policy": spread(whole), "encoder": spread(alone)}
    row["encoder_share"] = row["encoder"]["median_ms"] / row["policy"]["median_ms"]
    result["policy"] = row
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
