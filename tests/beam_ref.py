"""Beam search: a plain-torch restatement of the reference's BeamSearch bookkeeping (utils/decoding.py:527-600 —
``_make_beam_step``, ``_backtrack``, ``_select_best_beam``) with the tie rule the kernel states (equal candidates: the lower
flat index ``parent * N + node``), and CPU restatements of the two environments' transitions on the flat state of
``envspec`` (tsp/env.py:60-86, cvrp/env.py:66-96,126-136). Helper of tests/test_beam_cpu.py and tests/test_gpu_beam.py; not
collected."""
import torch


def make_beam_step(logprobs, parent_cum, beam_width: int):
    """``_make_beam_step``: ``logprobs`` [W*B, N] (beam-major rows), ``parent_cum`` [W*B] -> (selected node, parent beam,
    kept cumulative value), each [W*B] beam-major, the W kept candidates of an instance in descending order. The stable
    descending sort keeps equal values in ascending flat index: the kernel's tie rule (torch.topk leaves it open)."""
    rows, n = logprobs.shape
    b = rows // beam_width
    cand = logprobs + parent_cum[:, None]
    stacked = torch.cat(cand.split(b), dim=1)  # [B, W*N], column = parent * N + node
    val, ind = torch.sort(stacked, dim=1, descending=True, stable=True)
    val, ind = val[:, :beam_width], ind[:, :beam_width]
    flat = lambda x: torch.hstack(torch.unbind(x, 1))  # noqa: E731  [B, W] -> [W*B] beam-major
    ind = flat(ind)
    return ind % n, (ind // n).to(torch.int32), flat(val)


def backtrack(step_nodes, step_logps, parents, beam_width: int):
    """``_backtrack``: per-step selections [W*B, T] (column 0 = the start node) -> aligned (actions, logps) [W*B, T]."""
    rows, t = step_nodes.shape
    b = rows // beam_width
    inst = torch.arange(b, device=step_nodes.device).repeat(beam_width)
    cur = parents[:, -1].long()
    acts, lps = [step_nodes[:, -1]], [step_logps[:, -1]]
    for k in reversed(range(t - 1)):
        idx = inst + cur * b
        acts.append(step_nodes[idx, k])
        lps.append(step_logps[idx, k])
        cur = parents[idx, k].long()
    return torch.stack(acts[::-1], 1), torch.stack(lps[::-1], 1)


def select_best_beam(rewards, beam_width: int):
    """``_select_best_beam``: rows [B] of the beam of largest reward per instance, the lowest beam index on equal rewards."""
    b = rewards.shape[0] // beam_width
    per = rewards.view(beam_width, b)
    beams = torch.arange(beam_width, device=rewards.device).view(-1, 1).expand(beam_width, b)
    best = torch.where(per == per.max(0).values, beams, beam_width).min(0).values
    return best * b + torch.arange(b, device=rewards.device)


# ---- the two environments on the flat state (CPU tensors; rows beam-major over B_inst instances) ------------------------
def tsp_state(b: int, n: int, width: int, start=None):
    """The state after the imposed start step; ``start`` [W*B]: given start nodes instead of select_start_nodes'."""
    rows = width * b
    start = torch.arange(width).repeat_interleave(b) % n if start is None else start  # select_start_nodes, ops.py:128-161
    st = {"action_mask": torch.ones(rows, n, dtype=torch.bool), "first_node": torch.zeros(rows, dtype=torch.int64),
          "current_node": torch.zeros(rows, dtype=torch.int64), "i": torch.zeros(rows, dtype=torch.int64),
          "done": torch.zeros(rows, dtype=torch.bool)}
    env_step("tsp", st, start)
    return st, start


def cvrp_state(demand, width: int, start=None):
    b, n1 = demand.shape
    rows, n = width * b, n1 + 1
    start = torch.arange(width).repeat_interleave(b) % n1 + 1 if start is None else start
    mask = torch.ones(rows, n, dtype=torch.bool)
    mask[:, 0] = False
    st = {"demand": demand.contiguous(), "used_capacity": torch.zeros(rows), "vehicle_capacity": torch.ones(rows),
          "visited": torch.zeros(rows, n, dtype=torch.bool), "current_node": torch.zeros(rows, dtype=torch.int64),
          "action_mask": mask, "done": torch.zeros(rows, dtype=torch.bool)}
    env_step("cvrp", st, start)
    return st, start


def env_step(env: str, st: dict, action) -> None:
    """In place, every op one IEEE fp32 rounding as in the kernels."""
    rows = torch.arange(action.shape[0])
    a = action.long()
    if env == "tsp":
        st["first_node"].copy_(torch.where(st["i"] == 0, a, st["first_node"]))
        st["current_node"].copy_(a)
        st["action_mask"][rows, a] = False
        st["i"] += 1
        st["done"].copy_(~st["action_mask"].any(1))
        return
    demand = st["demand"]
    b, n1 = demand.shape
    dem = demand[rows % b]  # [rows, N-1]
    di = (a - 1).clamp(0, n1 - 1)
    used = (st["used_capacity"] + dem[rows, di]) * (a != 0).float()
    st["used_capacity"].copy_(used)
    st["current_node"].copy_(a)
    st["visited"][rows, a] = True
    masked = st["visited"][:, 1:] | (dem + used[:, None] > (st["vehicle_capacity"] + 1e-5)[:, None])
    st["action_mask"][:, 1:] = ~masked
    st["action_mask"][:, 0] = ~((a == 0) & (~masked).any(1))
    st["done"].copy_(st["visited"].all(1))


# ---- the recorder (needs the reference checkout) ---------------------------------------------------------------------------
# case -> (environment, num_loc, beam width, data seed). Batch 32. Next to each: instances (of 32) whose SET of final beams
# differs between the reference run in fp32 (the record) and the same reference run in float64 on the CPU — the noise floor
# the GPU parity test's budget of 1/4 has to cover (printed by ``python -m tests.beam_ref``).
CASES = {"tsp20_w5": ("tsp", 20, 5, 1234),    # fp32 vs float64: 0 of 32
         "tsp20_w20": ("tsp", 20, 20, 1234),  # fp32 vs float64: 1 of 32
         "cvrp20_w8": ("cvrp", 20, 8, 1234)}  # fp32 vs float64: 0 of 32
BATCH = 32
FULL = 2  # instances whose full per-step log-prob rows (every parent, every node) a record keeps


def _reference_run(case: str, dtype, select_best: bool):
    """The reference's own AttentionModelPolicy and environment with decode_type="beam_search" on the CPU."""
    import importlib

    from oracle import ref_import
    from tests.helpers import WEIGHT_SEED

    ref = ref_import.load()
    env_name, num_loc, width, data_seed = CASES[case]
    ref_env = (ref.TSPEnv if env_name == "tsp" else ref.CVRPEnv)(generator_params=dict(num_loc=num_loc), seed=0)
    torch.manual_seed(WEIGHT_SEED)
    pol = ref.AttentionModelPolicy(env_name=env_name).eval().to(dtype)
    torch.manual_seed(data_seed)
    data = ref_env.generator(batch_size=[BATCH])
    td0 = ref_env.reset(data.clone())
    if dtype != torch.float32:
        for k in list(td0.keys()):
            if td0[k].dtype == torch.float32:
                td0.set(k, td0[k].to(dtype))
    dec = importlib.import_module("rl4co.utils.decoding")
    seen = {"rows": [], "cum_in": [], "node": [], "parent": [], "cum": []}
    orig = dec.BeamSearch._make_beam_step

    def grab(self, logprobs):
        if not seen["node"]:
            seen["start"] = self.actions[0].clone()
        seen["rows"].append(logprobs.clone())
        seen["cum_in"].append(self.parent_beam_logprobs.view(-1).clone())
        selected, idx = orig(self, logprobs)
        seen["node"].append(selected.clone())
        seen["parent"].append(self.beam_path[-1].clone())
        seen["cum"].append(self.parent_beam_logprobs.view(-1).clone())
        return selected, idx

    dec.BeamSearch._make_beam_step = grab
    try:
        with torch.inference_mode():
            out = pol(td0.clone(), ref_env, phase="test", decode_type="beam_search", beam_width=width, select_best=select_best,
                      return_sum_log_likelihood=False)
    finally:
        dec.BeamSearch._make_beam_step = orig
    return data, out, seen


def beam_sets(actions, width: int):
    """Per instance, the set of final beams (rows of ``actions`` [W*B, T], trailing depot padding stripped)."""
    b = actions.shape[0] // width
    strip = lambda r: tuple(r[: max(i for i, a in enumerate(r) if a != 0 or i == 0) + 1])  # noqa: E731
    return [frozenset(strip(actions[j * b + i].tolist()) for j in range(width)) for i in range(b)]


def reference_rollout(case: str) -> dict:
    env_name, num_loc, width, _ = CASES[case]
    data, out, seen = _reference_run(case, torch.float32, select_best=False)
    _, best, _ = _reference_run(case, torch.float32, select_best=True)
    steps = len(seen["node"])
    rows = torch.arange(width).repeat_interleave(FULL) * BATCH + torch.arange(FULL).repeat(width)  # beam-major over FULL
    rec = {f"in_{k}": v for k, v in data.items()}
    rec.update(
        actions=out["actions"].to(torch.uint8), log_likelihood=out["log_likelihood"].float(), reward=out["reward"],
        best_actions=best["actions"].to(torch.uint8), best_reward=best["reward"],
        # per step (column 0 = the start): chosen node and parent of every beam, the smallest kept cumulative log-prob
        step_nodes=torch.stack([out["actions"][:, 0] * 0] + seen["node"], 1).to(torch.uint8),
        parents=torch.stack([seen["parent"][0] * 0] + seen["parent"], 1).to(torch.uint8),
        kept_min=torch.stack([c.view(width, BATCH)[-1] for c in seen["cum"]], 1),
        # the first FULL instances: every parent's full log-prob row, the cumulative values going in and coming out
        full_rows=torch.stack([r[rows] for r in seen["rows"]], 0),
        full_cum_in=torch.stack([c[rows] for c in seen["cum_in"]], 0),
        full_cum=torch.stack([c[rows] for c in seen["cum"]], 0),
    )
    rec["step_nodes"][:, 0] = seen["start"].to(torch.uint8)  # the start node of every beam row (select_start_nodes)
    assert rec["step_nodes"].shape[1] == steps + 1 == out["actions"].shape[1]
    return rec


def record(case: str) -> dict:
    from tests.helpers import reference_record

    return reference_record(f"beam_{case}", lambda: reference_rollout(case))


if __name__ == "__main__":  # RL4CO_RECORD_REFERENCE=1 python -m tests.beam_ref
    for name, (_, _, w, _) in CASES.items():
        r = record(name)
        _, out64, _ = _reference_run(name, torch.float64, select_best=False)
        a, b = beam_sets(r["actions"].long(), w), beam_sets(out64["actions"], w)
        print(name, {k: tuple(v.shape) for k, v in r.items()}, "fp32 vs float64 differing instances:",
              sum(x != y for x, y in zip(a, b)), "of", BATCH)


def reparent(st: dict, env: str, parents, width: int) -> dict:
    """``td[batch_beam_idx]``: every beam row takes its parent's per-trajectory state."""
    rows = parents.shape[0]
    b = rows // width
    idx = torch.arange(b).repeat(width) + parents.long() * b
    return {k: (v if (env == "cvrp" and k == "demand") else v[idx].clone()) for k, v in st.items()}
