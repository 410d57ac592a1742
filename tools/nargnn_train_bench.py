"""Time of one training forward + backward of DeepACO's heatmap encoder (rl4co_amd.TrainableNARGNNEncoder on
csrc/nargnn_train.hip) at the reference's depth (15 GNN layers, 5 heatmap-MLP layers, width 64) on TSP-100 x 128 (K = 20)
and TSP-50 x 512 (K = 10). Legs per shape, alternating round by round after a warm-up round, each timed with HIP events
around the whole call and synchronised:
  kernel   TrainableNARGNNEncoder in .train(): forward, then backward under a fixed gradient of the heatmap
  torch    the dense fp32 train-mode restatement of tests/nargnn_train_ref.py with autograd on the same card (this flatters
           the reference, which also builds its graphs one instance at a time in Python)
  ends     the kernel leg's torch ends alone (embeddings, heatmap MLP, scatter, log; an encoder without GNN layers)
  stack    rl4co_nargnn_train_forward alone, for the time per layer against the bytes its passes move
Per shape: median / min / max of each leg, the ratio of the medians, the share of the torch ends, the workspace, and the
forward's edge-tensor passes per layer as a time at the card's 8 TB/s. One more line: the whole DeepACOPolicy train step
(encoder, 30 ants' rollout, loss, backward) at the first shape with either encoder.

    python tools/nargnn_train_bench.py [--reps 5] [--out profiles/nargnn_train_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rl4co_amd import DeepACOPolicy, TrainableNARGNNEncoder  # noqa: E402
from rl4co_amd import kernels as K  # noqa: E402
from rl4co_amd.aco import deepaco_loss  # noqa: E402
from rl4co_amd.envs import TSPEnv  # noqa: E402
from tests import nargnn_ref as R  # noqa: E402
from tests import nargnn_train_ref as T  # noqa: E402

HBM_PEAK = 8.0e12  # MI355X, bytes / s (vendor figure)
SHAPES = [(100, 128), (50, 512)]
LAYERS, MLP_LAYERS, D = 15, 5, 64
# edge-tensor passes of one layer's forward: vert_pre reads w0; lin_fwd reads w0, writes pre_e; row_stats reads pre_e (its
# second sweep is meant to hit the cache); apply reads pre_e and w0, writes w
FORWARD_EDGE_PASSES = 7


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


def alternate(legs, reps):
    for fn in legs.values():  # warm-up round
        fn()
    times = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            times[name].append(timed(fn))
    return {name: spread(ms) for name, ms in times.items()}


def step(enc, td, grad):
    def run():
        for p in enc.parameters():
            p.grad = None
        logits, _ = enc(td)
        logits.backward(grad)

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/nargnn_train_bench.json")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sd = R.make_state_dict(1, LAYERS, MLP_LAYERS)
    enc = TrainableNARGNNEncoder()
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dev).train()
    ends = TrainableNARGNNEncoder(num_layers_graph_encoder=0)
    ends.load_state_dict(R.make_state_dict(1, 0, MLP_LAYERS), strict=True)
    ends = ends.to(dev).train()
    ref = T.ModuleAsEncoder(sd).to(dev)
    result = {"layers": LAYERS, "mlp_layers": MLP_LAYERS, "reps": args.reps, "hbm_peak_bytes_per_s": HBM_PEAK, "shapes": []}
    for n, b in SHAPES:
        k = R.num_neighbors(n)
        locs = torch.rand(b, n, 2, generator=torch.Generator().manual_seed(n + b)).to(dev)
        td = {"locs": locs}
        grad = torch.rand(b, n, n, generator=torch.Generator().manual_seed(5)).to(dev) * 2 - 1
        nbr, _ = enc.neighbors(locs)
        ptr, src = K.incoming_csr(nbr)
        p = enc.packed_parameters(dev)
        bns = [bn.module for layer in enc.graph_network.layers for bn in (layer.v_bn, layer.e_bn)]
        bn_w = torch.stack([m.weight for m in bns]).detach().view(LAYERS, 2, D).contiguous()
        bn_b = torch.stack([m.bias for m in bns]).detach().view(LAYERS, 2, D).contiguous()
        x = torch.randn(b, n, D, device=dev)
        w = torch.randn(b, n, k, D, device=dev)
        legs = {"kernel": step(enc, td, grad), "torch": step(ref, td, grad), "ends": step(ends, td, grad),
                "stack": lambda: K.nargnn_train_forward(nbr, ptr, src, x, w, lin_w=p["lin_w"], lin_b=p["lin_b"], bn_w=bn_w,
                                                        bn_b=bn_b)}
        row = {"num_loc": n, "batch": b, "k": k, **alternate(legs, args.reps)}
        row["speedup"] = row["torch"]["median_ms"] / row["kernel"]["median_ms"]
        row["torch_ends_share"] = row["ends"]["median_ms"] / row["kernel"]["median_ms"]
        row["workspace_bytes"] = K.nargnn_train_workspace_bytes(b, n, k, LAYERS)
        edge_bytes = b * n * k * D * 4
        row["forward_us_per_layer"] = 1e3 * row["stack"]["median_ms"] / LAYERS
        row["forward_edge_passes_per_layer"] = FORWARD_EDGE_PASSES
        row["forward_us_per_layer_at_hbm_peak"] = 1e6 * FORWARD_EDGE_PASSES * edge_bytes / HBM_PEAK
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
        del legs, x, w, grad
        torch.cuda.empty_cache()
    # the whole policy train step at the first shape
    n, b = SHAPES[0]
    torch.manual_seed(0)
    env = TSPEnv(generator_params=dict(num_loc=n))
    td = env.reset(batch_size=[b])

    def train_step(pol):
        def run():
            for p in pol.parameters():
                p.grad = None
            deepaco_loss(pol(td, env, phase="train")).backward()

        return run

    pols = {"kernel": DeepACOPolicy(encoder=enc).to(dev).train(), "torch": DeepACOPolicy(encoder=ref).to(dev).train()}
    row = {"num_loc": n, "batch": b, "n_ants": 30, **alternate({name: train_step(pol) for name, pol in pols.items()}, args.reps)}
    row["speedup"] = row["torch"]["median_ms"] / row["kernel"]["median_ms"]
    result["policy_train_step"] = row
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
