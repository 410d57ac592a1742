"""Cost of the multi-agent TSP (min-max) in the fused decode launch (am_decode.hip): the mTSP-100 x 4096 bf16 decode launch
beside the TSP-100 and CVRP-100 launches of the same build with the row cache off (mTSP has none), each timed alone with HIP
events, the legs alternating round by round, with the in-kernel counter of cache rows streamed from HBM; once with the
one-wave kernel pinned and once with the variant the library picks.

    python tools/mtsp_bench.py [--reps 9] [--out profiles/mtsp_bench.json]

The three environments list different numbers of rows per tour (mTSP adds depot visits between subtours, CVRP more), so the
comparable figure is the time per million listed rows."""
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


class Leg:
    """One decode launch, prepared once (policy, instances, folded cache) and timed launch by launch."""

    def __init__(self, env_name, num_loc, batch, variant):
        torch.manual_seed(0)
        self.pol = AttentionModelPolicy(env_name, cache_dtype=torch.bfloat16, encoder_autocast=torch.bfloat16).cuda().eval()
        gen = dict(num_loc=num_loc, device="cuda")
        if env_name == "mtsp":
            gen.update(min_num_agents=5, max_num_agents=5)  # the reference generator's default
        env = get_env(env_name, generator_params=gen, device="cuda")
        torch.manual_seed(1)
        self.td = env.reset(batch_size=[batch])
        self.env_name, self.num_loc, self.batch, self.variant = env_name, num_loc, batch, variant
        with torch.inference_mode():
            hidden, _ = self.pol._encode(self.td)
            self.cache = self.pol.decoder.precompute_cache(hidden, torch.bfloat16, torch.float32, fold=True)
        self.n = self.td["action_mask"].shape[-1]
        self.tmax = self.pol._max_horizon(env_name, self.n)
        self.ran = K.decode_variant(self.n, torch.bfloat16, self.tmax, batch, batch, env_name=env_name) if variant == "auto" else None
        self.times, self.rows, self.steps, self.longest = [], 0, 0, 0

    def launch(self, keep: bool):
        with torch.inference_mode():
            st = self.pol._initial_state(self.td, 0)
            actions = torch.zeros(self.batch, self.tmax, dtype=torch.int64, device="cuda")
            logps = torch.zeros(self.batch, self.tmax, device="cuda")
            status = torch.zeros(6, dtype=torch.int32, device="cuda")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            K.am_decode(self.cache, st, mode="sampling", max_steps=self.tmax, actions=actions, logps=logps, err=status[:1],
                        variant=self.variant, philox_seed=1234, steps_summary=status[2:6])  # one seed: the same tours every launch
            e1.record()
            torch.cuda.synchronize()
        err, _, self.longest, self.steps, lo, hi = status.tolist()
        assert err == 0, err
        self.rows = (hi << 32) | (lo & 0xFFFFFFFF)
        if keep:
            self.times.append(e0.elapsed_time(e1))

    def result(self):
        t = sorted(self.times)
        med = t[len(t) // 2]
        names = {1: "stream", 2: "lds", 3: "wide", 4: "ms"}
        r = dict(case=f"{self.env_name}{self.num_loc}x{self.batch}", variant=self.variant, planes="bf16", mode="sampling",
                 reps=len(t), median_ms=med, min_ms=t[0], max_ms=t[-1], longest_tour=self.longest,
                 trajectory_steps=self.steps, us_per_trajectory_step=1e3 * med / self.steps)
        if self.ran is not None:
            r["variant_run"] = names.get(self.ran, str(self.ran))
        if self.rows:  # (0: the planes were LDS-resident, read once per rollout)
            r.update(listed_rows=self.rows, ms_per_million_rows=med / (self.rows / 1e6))
        return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["RL4CO_DECODE_ROW_CACHE"] = "0"  # read at every launch: TSP / CVRP stream every listed row, as mTSP does
    # mTSP's num_loc counts the depot: 100 nodes; TSP-100 has 100 nodes, CVRP-100 has 101
    legs = [Leg(env, 100, a.batch, variant) for variant in ("stream", "auto") for env in ("mtsp", "tsp", "cvrp")]
    for it in range(a.reps + 2):  # two warm-up rounds; the legs alternate inside every round
        for leg in legs:
            leg.launch(keep=it >= 2)
    rows = [leg.result() for leg in legs]
    for r in rows:
        print(json.dumps(r), flush=True)
    ratio_tsp = rows[0]["ms_per_million_rows"] / rows[1]["ms_per_million_rows"]
    ratio_cvrp = rows[0]["ms_per_million_rows"] / rows[2]["ms_per_million_rows"]
    print(f"mtsp / tsp, stream, ms per million listed rows: {ratio_tsp:.3f}; mtsp / cvrp: {ratio_cvrp:.3f}")
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), when=time.strftime("%Y-%m-%d"), row_cache="off",
                           per_row_ratio_mtsp_over_tsp_stream=ratio_tsp, per_row_ratio_mtsp_over_cvrp_stream=ratio_cvrp,
                           rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
