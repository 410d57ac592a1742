"""Cost of beam search (am_decode_beam.hip) beside the closest existing workload: the beam launch at TSP-100 x B x W in bf16
planes and the multistart greedy decode launch with the same number of rows (W starts per instance, the variant the library
picks), each timed alone with HIP events, the legs alternating round by round.

    python tools/beam_bench.py [--reps 7] [--batch 1024] [--widths 16 100] [--out profiles/beam_bench.json]
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


class Leg:
    """One decode launch over W rows per instance — beam search or multistart greedy — prepared once, timed launch by launch."""

    def __init__(self, kind, num_loc, batch, width):
        torch.manual_seed(0)
        self.pol = AttentionModelPolicy("tsp", cache_dtype=torch.bfloat16, encoder_autocast=torch.bfloat16).cuda().eval()
        self.env = get_env("tsp", generator_params=dict(num_loc=num_loc, device="cuda"), device="cuda")
        torch.manual_seed(1)
        self.td = self.env.reset(batch_size=[batch])
        self.kind, self.num_loc, self.batch, self.width = kind, num_loc, batch, width
        with torch.inference_mode():
            hidden, _ = self.pol._encode(self.td)
            self.cache = self.pol.decoder.precompute_cache(hidden, torch.bfloat16, torch.float32, fold=True)
        self.n = self.td["action_mask"].shape[-1]
        self.times = []

    def launch(self, keep: bool):
        rows, t_len = self.width * self.batch, self.n
        with torch.inference_mode():
            st = self.pol._initial_state(self.td, self.width)
            status = torch.zeros(6, dtype=torch.int32, device="cuda")
            first = self.env.select_start_nodes(self.td, num_starts=self.width)
            K.env_step("tsp", st, first, status[:1])
            actions = torch.zeros(rows, t_len, dtype=torch.int64, device="cuda")
            logps = torch.zeros(rows, t_len, device="cuda")
            raw = {k: torch.zeros(rows, t_len, dtype=dt, device="cuda")
                   for k, dt in (("step_nodes", torch.int32), ("step_logps", torch.float32), ("parents", torch.int32),
                                 ("cum_logp", torch.float32))} if self.kind == "beam_search" else {}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if self.kind == "beam_search":
                K.am_decode_beam(self.cache, st, self.width, t_len - 1, actions=actions, logps=logps, err=status[:1],
                                 steps_summary=status[2:4], **raw)
            else:
                K.am_decode(self.cache, st, mode="greedy", max_steps=t_len - 1, t0=1, actions=actions, logps=logps,
                            err=status[:1], steps_summary=status[2:6])
            e1.record()
            torch.cuda.synchronize()
        assert status[0].item() == 0, status[0].item()
        if keep:
            self.times.append(e0.elapsed_time(e1))

    def result(self):
        t = sorted(self.times)
        return dict(case=f"tsp{self.num_loc}x{self.batch}xW{self.width}", kind=self.kind, planes="bf16", reps=len(t),
                    median_ms=t[len(t) // 2], min_ms=t[0], max_ms=t[-1], rows=self.width * self.batch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--widths", type=int, nargs="+", default=[16, 100])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    legs = [Leg(kind, 100, a.batch, w) for w in a.widths for kind in ("beam_search", "multistart_greedy")]
    for it in range(a.reps + 2):  # two warm-up rounds; the legs alternate inside every round
        for leg in legs:
            leg.launch(keep=it >= 2)
    rows = [leg.result() for leg in legs]
    for r in rows:
        print(json.dumps(r), flush=True)
    ratios = {f"W{rows[i]['rows'] // a.batch}": rows[i]["median_ms"] / rows[i + 1]["median_ms"] for i in range(0, len(rows), 2)}
    print("beam search / multistart greedy, median ms per rollout:", json.dumps(ratios))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), when=time.strftime("%Y-%m-%d"),
                           ratio_beam_over_multistart_greedy=ratios, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
