"""Cost of the top-k / top-p filter in the fused decode launch (am_decode.hip, csrc/topkp.h): the decode kernel alone, timed
with HIP events, without a filter, with top_k = 10, top_p = 0.9 and both.

    python tools/topkp_bench.py [--reps 7] [--out profiles/topkp_bench.json]

Cases: TSP-100 x 4096 bf16 sampling (stream variant), CVRP-500 x 1024 bf16 sampling (wide variant), and the multistart
fallback: TSP-100 x 512 instances x 8 starts bf16 sampling, auto variant (MS without a filter, not MS with one)."""
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

FILTERS = [("none", 0, 0.0), ("top_k=10", 10, 0.0), ("top_p=0.9", 0, 0.9), ("both", 10, 0.9)]


def bench(env_name, num_loc, batch, variant, starts, reps):
    torch.manual_seed(0)
    pol = AttentionModelPolicy(env_name, cache_dtype=torch.bfloat16, encoder_autocast=torch.bfloat16).cuda().eval()
    env = get_env(env_name, generator_params=dict(num_loc=num_loc, device="cuda"), device="cuda")
    td = env.reset(batch_size=[batch])
    rows = []
    with torch.inference_mode():
        hidden, _ = pol._encode(td)
        cache = pol.decoder.precompute_cache(hidden, torch.bfloat16, torch.float32, fold=True)
        n = td["action_mask"].shape[-1]
        b = batch * max(starts, 1)
        tmax = n if env_name == "tsp" else 2 * n
        for name, k, p in FILTERS:
            times = []
            for it in range(reps):
                st = pol._initial_state(td, starts)
                actions = torch.zeros(b, tmax, dtype=torch.int64, device="cuda")
                logps = torch.zeros(b, tmax, device="cuda")
                err = K.new_error_word("cuda")
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                K.am_decode(cache, st, mode="sampling", max_steps=tmax, actions=actions, logps=logps, err=err,
                            variant=variant, philox_seed=1234 + it, top_k=k, top_p=p)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
                assert int(err.item()) == 0
            t = sorted(times[1:])
            rows.append(dict(case=f"{env_name}{num_loc}x{batch}" + (f"x{starts}starts" if starts else ""), variant=variant,
                             filter=name, median_ms=t[len(t) // 2], min_ms=t[0], max_ms=t[-1]))
            print(json.dumps(rows[-1]), flush=True)
    base = rows[0]["median_ms"]
    for r in rows:
        r["ratio"] = r["median_ms"] / base
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    rows += bench("tsp", 100, 4096, "stream", 0, a.reps)
    rows += bench("cvrp", 500, 1024, "wide", 0, a.reps)
    rows += bench("tsp", 100, 512, "auto", 8, a.reps)
    for r in rows:
        print(f"{r['case']:24s} {r['variant']:7s} {r['filter']:10s} {r['median_ms']:8.3f} ms  x{r['ratio']:.3f}")
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), when=time.strftime("%Y-%m-%d"), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
