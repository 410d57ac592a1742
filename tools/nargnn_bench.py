"""Time of DeepACO's heatmap encoder (rl4co_amd.NARGNNEncoder on csrc/nargnn.hip) at the reference's depth (15 GNN layers,
5 heatmap-MLP layers, width 64) on TSP-50 x 4096 (K = 10), TSP-100 x 1024 and TSP-100 x 4096 (K = 20). Two legs per shape,
alternating round by round after one warm-up round, each timed with HIP events around the whole call and synchronised:
  kernel   NARGNNEncoder.forward: neighbour selection by torch ops, then ONE rl4co_nargnn_heatmap launch
  torch    the dense fp32 restatement of tests/nargnn_ref.py from torch ops on the same card (neighbour selection
           included). This flatters the reference, which also builds its graphs one instance at a time in Python.
Per shape: median / min / max of each leg, the ratio of the medians, the FLOP count (2 D D (4 N + N K) per GNN layer,
2 D D N K per MLP layer) as a share of the card's fp32 MFMA peak, and the bytes that must move (inputs and outputs).
One more line: the whole DeepACOPolicy call (48 ants, 10 iterations) at TSP-100 x 256 with the encoder's share of it.

    python tools/nargnn_bench.py [--reps 5] [--out profiles/nargnn_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rl4co_amd import DeepACOPolicy, NARGNNEncoder  # noqa: E402
from rl4co_amd import kernels as K  # noqa: E402
from rl4co_amd.envs import TSPEnv  # noqa: E402
from tests import nargnn_ref as R  # noqa: E402

FP32_MFMA_PEAK = 157.3e12  # MI355X, fp32 matrix, FLOP/s (vendor figure)
SHAPES = [(50, 4096), (100, 1024), (100, 4096)]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/nargnn_bench.json")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sd = R.make_state_dict(1, LAYERS, MLP_LAYERS)
    enc = NARGNNEncoder().eval()
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    result = {"layers": LAYERS, "mlp_layers": MLP_LAYERS, "reps": args.reps, "fp32_mfma_peak_flops": FP32_MFMA_PEAK, "shapes": []}
    for n, b in SHAPES:
        k = R.num_neighbors(n)
        locs = torch.rand(b, n, 2, generator=torch.Generator().manual_seed(n + b)).to(dev)
        td = {"locs": locs}
        legs = {"kernel": lambda: enc(td), "torch": lambda: R.encode(sd_dev, locs, dtype=torch.float32)}
        with torch.no_grad():
            for fn in legs.values():  # warm-up round
                fn()
            times = {name: [] for name in legs}
            for _ in range(args.reps):
                for name, fn in legs.items():
                    times[name].append(timed(fn))
            diff = float((enc(td)[0] - R.encode(sd_dev, locs, dtype=torch.float32)[0]).abs().max())
        flop = b * (LAYERS * 2 * D * D * (4 * n + n * k) + (MLP_LAYERS - 1) * 2 * D * D * n * k + 2 * D * n * k)
        moved = b * (n * 2 * 4 + n * k * 8 + n * n * 4 + n * D * 4)
        row = {"num_loc": n, "batch": b, "k": k, "tier": "lds" if n <= K.nargnn_lds_nodes(k) else "scratch",
               "kernel": spread(times["kernel"]), "torch": spread(times["torch"]), "flop": flop, "bytes_that_must_move": moved,
               "max_abs_diff_vs_torch": diff}
        row["speedup"] = row["torch"]["median_ms"] / row["kernel"]["median_ms"]
        row["share_of_fp32_mfma_peak"] = flop / (row["kernel"]["median_ms"] * 1e-3) / FP32_MFMA_PEAK
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
        del locs, td, legs
        torch.cuda.empty_cache()
    # the whole policy call
    torch.manual_seed(0)
    env = TSPEnv(generator_params=dict(num_loc=100))
    td = env.reset(batch_size=[256])
    pol = DeepACOPolicy().eval()
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
