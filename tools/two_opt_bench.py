"""Time of the TSP 2-opt kernel (tsp_two_opt.hip) on the two inputs a user would hand it: 4096 x TSP-100 seeded random
permutations, and the greedy tours of a random-init policy on the same instances. Each launch is timed with HIP events
after two warm-up launches per input, the inputs alternating round by round; next to the time, the mean number of scans
per tour and the tour-length improvement in float64. The reference's numba path runs on neither machine, so the figure is
recorded, not compared.

    python tools/two_opt_bench.py [--reps 10] [--batch 4096] [--num-loc 100] [--out profiles/two_opt_bench.json]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rl4co_amd import kernels as K  # noqa: E402
from rl4co_amd.envs import get_env  # noqa: E402
from rl4co_amd.policy import AttentionModelPolicy  # noqa: E402
from rl4co_amd.tensordict import TensorDict  # noqa: E402


def length64(locs, tours):
    p = locs.double().gather(1, tours[..., None].expand(-1, -1, 2))
    return (p - p.roll(-1, dims=1)).norm(dim=-1).sum(1)


class Leg:
    def __init__(self, kind, locs, tours, max_iterations):
        self.kind, self.locs, self.tours, self.max_iterations = kind, locs, tours.contiguous(), max_iterations
        self.err = K.new_error_word(locs.device)
        self.times, self.out, self.iters = [], None, None

    def launch(self, keep: bool):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.out, self.iters = K.tsp_two_opt(self.tours, locs=self.locs, max_iterations=self.max_iterations, err=self.err,
                                             return_iterations=True)
        e1.record()
        torch.cuda.synchronize()
        if keep:
            self.times.append(e0.elapsed_time(e1))

    def result(self):
        assert int(self.err.item()) == 0
        t = sorted(self.times)
        before, after = length64(self.locs, self.tours), length64(self.locs, self.out)
        b, n = self.tours.shape
        return dict(case=f"tsp{n}x{b}", input=self.kind, max_iterations=self.max_iterations, reps=len(t),
                    median_ms=t[len(t) // 2], min_ms=t[0], max_ms=t[-1],
                    mean_iterations=float(self.iters.double().mean()), max_iterations_seen=int(self.iters.max()),
                    mean_length_before_f64=float(before.mean()), mean_length_after_f64=float(after.mean()),
                    mean_improvement_f64=float((before - after).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--num-loc", type=int, default=100)
    ap.add_argument("--max-iterations", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("two_opt_bench needs the MI355X: a time taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1234)
    locs = torch.rand(a.batch, a.num_loc, 2, generator=g).to(dev)
    random_tours = torch.stack([torch.randperm(a.num_loc, generator=g) for _ in range(a.batch)]).to(dev)
    torch.manual_seed(0)
    pol = AttentionModelPolicy("tsp").eval().to(dev)
    env = get_env("tsp", generator_params=dict(num_loc=a.num_loc, device=dev), device=dev)
    td = env.reset(TensorDict({"locs": locs}, batch_size=[a.batch]))
    with torch.inference_mode():
        greedy_tours = pol(td, env, phase="test", decode_type="greedy")["actions"].clone()
    legs = [Leg("random_permutation", locs, random_tours, a.max_iterations),
            Leg("greedy_random_init_policy", locs, greedy_tours, a.max_iterations)]
    for it in range(a.reps + 2):  # two warm-up rounds; the legs alternate inside every round
        for leg in legs:
            leg.launch(keep=it >= 2)
    rows = [leg.result() for leg in legs]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), when=time.strftime("%Y-%m-%d"),
                           what="rl4co_tsp_two_opt, one launch over the batch, HIP events around the launch", rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
