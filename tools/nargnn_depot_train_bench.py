"""Time of one training forward + backward of DeepACO's depot-graph heatmap encoder (rl4co_amd.TrainableNARGNNDepotEncoder
on csrc/nargnn_train.hip's depot instantiation) at the reference's depth (15 GNN layers, 5 heatmap-MLP layers, width 64) on
CVRP-100 x 128 (N = 101, K = 20) and CVRP-50 x 512 (N = 51, K = 10). The protocol, the timer and the legs are
tools/nargnn_train_bench.py's: HIP events around the whole call, a warm-up round, then alternating rounds, medians.
  kernel   TrainableNARGNNDepotEncoder in .train(): forward, then backward under a fixed gradient of the heatmap
  torch    the fp32 edge-list train-mode restatement of tests/nargnn_depot_train_ref.py with autograd on the same card
  ends     the kernel leg's torch ends alone (embeddings, heatmap MLP, scatter, log; an encoder without GNN layers)
  stack    rl4co_nargnn_depot_train_forward alone, for the time per layer against the bytes its passes move
One more line: the whole NonAutoregressivePolicy train step (encoder, 30 ants' rollout, loss, backward) at the first shape
with either encoder.

    python tools/nargnn_depot_train_bench.py [--reps 5] [--out profiles/nargnn_depot_train_bench.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nargnn_train_bench import D, FORWARD_EDGE_PASSES, HBM_PEAK, LAYERS, MLP_LAYERS, alternate, step  # noqa: E402
from rl4co_amd import NonAutoregressivePolicy, TrainableNARGNNDepotEncoder  # noqa: E402
from rl4co_amd import kernels as K  # noqa: E402
from rl4co_amd.aco import deepaco_loss  # noqa: E402
from tests import aco_depot_grad_ref as G  # noqa: E402
from tests import nargnn_depot_ref as R  # noqa: E402
from tests import nargnn_depot_train_ref as T  # noqa: E402

ENV = "cvrp"
SHAPES = [(101, 128), (51, 512)]  # (N with the depot, batch)
ANTS = 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/nargnn_depot_train_bench.json")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sd = R.make_state_dict(ENV, 1, LAYERS, MLP_LAYERS)
    enc = TrainableNARGNNDepotEncoder(env_name=ENV)
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dev).train()
    ends = TrainableNARGNNDepotEncoder(env_name=ENV, num_layers_graph_encoder=0)
    ends.load_state_dict(R.make_state_dict(ENV, 1, 0, MLP_LAYERS), strict=True)
    ends = ends.to(dev).train()
    ref = T.ModuleAsEncoder(sd, ENV).to(dev)
    result = {"env": ENV, "layers": LAYERS, "mlp_layers": MLP_LAYERS, "reps": args.reps, "hbm_peak_bytes_per_s": HBM_PEAK,
              "shapes": []}
    for n, b in SHAPES:
        k = R.num_neighbors(n)
        e = (n - 1) * (k + 2)
        data = G.random_data(ENV, b, n, n + b)
        td = G.as_td(ENV, data, dev)
        grad = torch.rand(b, n, n, generator=torch.Generator().manual_seed(5)).to(dev) * 2 - 1
        nbr, _, _ = enc.neighbors(td["locs"])
        ptr, src = K.depot_incoming_csr(nbr)
        p = enc.packed_parameters(dev)
        bns = [bn.module for layer in enc.graph_network.layers for bn in (layer.v_bn, layer.e_bn)]
        bn_w = torch.stack([m.weight for m in bns]).detach().view(LAYERS, 2, D).contiguous()
        bn_b = torch.stack([m.bias for m in bns]).detach().view(LAYERS, 2, D).contiguous()
        x = torch.randn(b, n, D, device=dev)
        w = torch.randn(b, e, D, device=dev)
        legs = {"kernel": step(enc, td, grad), "torch": step(ref, td, grad), "ends": step(ends, td, grad),
                "stack": lambda: K.nargnn_depot_train_forward(nbr, ptr, src, x, w, lin_w=p["lin_w"], lin_b=p["lin_b"], bn_w=bn_w,
                                                              bn_b=bn_b)}
        row = {"nodes": n, "batch": b, "k": k, "edge_rows": b * e, **alternate(legs, args.reps)}
        row["speedup"] = row["torch"]["median_ms"] / row["kernel"]["median_ms"]
        row["torch_ends_share"] = row["ends"]["median_ms"] / row["kernel"]["median_ms"]
        row["workspace_bytes"] = K.nargnn_depot_train_workspace_bytes(b, n, k, LAYERS)
        row["forward_us_per_layer"] = 1e3 * row["stack"]["median_ms"] / LAYERS
        row["forward_edge_passes_per_layer"] = FORWARD_EDGE_PASSES
        row["forward_us_per_layer_at_hbm_peak"] = 1e6 * FORWARD_EDGE_PASSES * b * e * D * 4 / HBM_PEAK
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
        del legs, x, w, grad
        torch.cuda.empty_cache()
    # the whole policy train step at the first shape
    n, b = SHAPES[0]
    td = G.as_td(ENV, G.random_data(ENV, b, n, 0), dev)

    def train_step(pol):
        def run():
            for q in pol.parameters():
                q.grad = None
            torch.manual_seed(0)
            out = pol(td, ENV, phase="train", multisample=True, num_samples=ANTS)
            deepaco_loss({key: out[key].view(ANTS, b).t() for key in ("reward", "log_likelihood")}).backward()

        return run

    pols = {"kernel": NonAutoregressivePolicy(encoder=enc, env_name=ENV).to(dev).train(),
            "torch": NonAutoregressivePolicy(encoder=ref, env_name=ENV).to(dev).train()}
    row = {"nodes": n, "batch": b, "n_ants": ANTS, **alternate({name: train_step(pol) for name, pol in pols.items()}, args.reps)}
    row["speedup"] = row["torch"]["median_ms"] / row["kernel"]["median_ms"]
    result["policy_train_step"] = row
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
