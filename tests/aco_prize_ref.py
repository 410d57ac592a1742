"""Ant System on a heatmap (OP and PCTSP): a plain-torch fp32 restatement of one iteration (the environment's state and mask
in its own expressions, heatmap logits -> masked log-softmax -> key = lp - ln_noise -> lowest-index argmax, rows W = n wide
and zero-filled after done; the reward of the W-wide row in the kernel's stated order, which is ATen's row sum; reward map;
best-row record as the reference's ragged list; pheromone deposit with the ants added in order) and the recorder of the
reference's own ``AntSystem`` runs with its ``OPEnv`` / ``PCTSPEnv`` under injected noise
(tests/golden/reference/aco_op_*.npz, aco_pctsp_*.npz). tests/test_aco_prize_cpu.py pins the restatement to the records; the
GPU tests compare the kernel with both. The pieces shared with TSP and CVRP (logits, log-softmax, reward map, noise, update,
the ragged record) are tests/aco_ref.py's and tests/aco_cvrp_ref.py's. Node 0 is the depot, ``n`` counts it, rows are
ant-major: row ``j * B + b`` is ant ``j`` of instance ``b``.

``data`` is a dict of per-instance tensors: ``locs`` [B, n, 2], ``prize`` [B, n] (0 at the depot; PCTSP: ``real_prize``) and
``max_length`` [B, n] (OP, the environment's per-node table) or ``penalty`` [B, n] (PCTSP, 0 at the depot)."""
import torch

from tests.aco_cvrp_ref import final_matrix, fresh_state, pad, record_finals, update  # noqa: F401
from tests.aco_ref import f32, heuristic, ln_exp1, logits, step_logps  # noqa: F401

ENVS = ("op", "pctsp")
# case -> (customers, ants, B, iterations, alpha, beta, decay, initial pheromone (None: ones), data seed per environment)
CASES = {"c10_a5": (10, 5, 4, 3, 1.0, 1.0, 0.95, None, {"op": 3234, "pctsp": 4234}),
         "c10_a5_ab": (10, 5, 4, 3, 0.7, 2.0, 0.8, 2, {"op": 3236, "pctsp": 4236}),
         "c20_a20": (20, 20, 4, 3, 1.0, 1.0, 0.95, None, {"op": 3235, "pctsp": 4235})}
# Per-step tolerance of a kernel log-prob against the recorded reference or this restatement (fp32 both sides, another
# operation order and another exp / log): 4 x the largest deviation of the reference's OWN fp32 per-step log-probs from the
# same steps evaluated in float64, over the six records (the key "noise_floor" of each record; measured on the CPU).
NOISE_FLOORS = {"op_c10_a5": 2.602e-07, "op_c10_a5_ab": 3.596e-07, "op_c20_a20": 3.445e-07,  # (each rounded up)
                "pctsp_c10_a5": 2.807e-07, "pctsp_c10_a5_ab": 3.845e-07, "pctsp_c20_a20": 3.696e-07}
MEASURED_NOISE_FLOOR = max(NOISE_FLOORS.values())
STEP_TOL = 4 * MEASURED_NOISE_FLOOR
# reward_w (the W-wide row) against the recorded reward (the row trimmed to its iteration's longest): both sum the same
# terms, the trailing ones exactly 0, in another association of ATen's 8-lane / 4-accumulator cascade. In ulps of
# reward_scale (OP: the reward itself; PCTSP: length + total penalty, the largest term of S - (len + P)), measured on the
# six records (the key "reward_ulps" of each record; python -m tests.aco_prize_ref prints them). The asserted bound is the
# largest measured one.
REWARD_ULPS_BY_RECORD = {"op_c10_a5": 1.0, "op_c10_a5_ab": 1.0, "op_c20_a20": 0.0,
                         "pctsp_c10_a5": 0.0, "pctsp_c10_a5_ab": 0.0, "pctsp_c20_a20": 0.0}
MEASURED_REWARD_ULPS = max(REWARD_ULPS_BY_RECORD.values())
REWARD_ULPS = MEASURED_REWARD_ULPS


def width(n):
    """W = n: at most n - 1 customers, then the depot."""
    return n


# ---- the environments' state (op/env.py:67-154, pctsp/env.py:62-144), all rows at once ------------------------------------------
def mask(env, data, inst, cur, visited, acc):
    """[rows, n] bool, True = INFEASIBLE (the complement of get_action_mask). ``acc``: OP tour_length, PCTSP cur_total_prize."""
    m = visited | visited[:, 0:1]
    if env == "op":
        locs = data["locs"][inst]
        cur_loc = locs[torch.arange(cur.shape[0]), cur][:, None, :]
        exceeds = acc[:, None] + (locs - cur_loc).norm(p=2, dim=-1) > data["max_length"][inst]
        m = m | exceeds
        m[:, 0] = False
    else:
        m[:, 0] = (acc < 1.0) & (visited[:, 1:].int().sum(-1) < visited.shape[1] - 1)
    return m


def advance(env, data, inst, cur, acc, action):
    """The accumulator after ``action``."""
    if env == "op":
        locs = data["locs"][inst]
        ar = torch.arange(cur.shape[0])
        return acc + (locs[ar, action] - locs[ar, cur]).norm(p=2, dim=-1)
    return acc + data["prize"][inst].gather(1, action[:, None]).squeeze(1)


def select_rows(lp, ln_noise, infeasible):
    """Lowest-index argmax over the feasible nodes of lp - ln_noise, every row (a NaN key counts as -inf)."""
    key = (lp - ln_noise).masked_fill(infeasible, float("-inf"))
    key = torch.where(key != key, torch.full_like(key, float("-inf")), key)
    n = key.shape[1]
    best = key.max(-1, keepdim=True).values
    return torch.where((key == best) & ~infeasible, torch.arange(n)[None, :], n).min(-1).values


# ---- sampling ---------------------------------------------------------------------------------------------------------------
def sample(env, pheromone, log_heu, data, ln_noise, alpha=1.0, beta=1.0, temperature=1.0, forced=None, rows=None):
    """One iteration's rows. ln_noise [W, rows, n] (None with ``forced`` [rows, W]).
    Returns actions [rows, W], lengths [rows], logps [rows, W], all_logps [rows, W, n], masks [rows, W, n] (True = infeasible;
    rows of steps not taken are all False)."""
    b, n, _ = pheromone.shape
    w = width(n)
    if rows is None:
        rows = forced.shape[0] if forced is not None else ln_noise.shape[1]
    ar = torch.arange(rows)
    inst = ar % b
    lg = logits(pheromone, log_heu, alpha, beta)
    actions = torch.zeros(rows, w, dtype=torch.int64)
    lengths = torch.zeros(rows, dtype=torch.int32)
    logps = torch.zeros(rows, w)
    full = torch.zeros(rows, w, n)
    masks = torch.zeros(rows, w, n, dtype=torch.bool)
    cur = torch.zeros(rows, dtype=torch.int64)
    visited = torch.zeros(rows, n, dtype=torch.bool)
    acc = torch.zeros(rows)
    done = torch.zeros(rows, dtype=torch.bool)
    for t in range(w):
        live = ~done
        if not bool(live.any()):
            break
        m = mask(env, data, inst, cur, visited, acc)
        lp = step_logps(lg[inst, cur], m, temperature)
        nxt = forced[:, t] if forced is not None else select_rows(lp, ln_noise[t], m)
        nxt = torch.where(live, nxt, torch.zeros_like(nxt))
        actions[:, t] = nxt
        logps[:, t] = torch.where(live, lp[ar, nxt], torch.zeros(rows))
        full[:, t] = torch.where(live[:, None], lp, torch.zeros(rows, n))
        masks[:, t] = m & live[:, None]
        acc = torch.where(live, advance(env, data, inst, cur, acc, nxt), acc)
        visited[ar[live], nxt[live]] = True
        cur = torch.where(live, nxt, cur)
        lengths += live.to(torch.int32)
        done = done | (live & (nxt == 0) & (t > 0))
    return actions, lengths, logps, full, masks


def tour_length_w(locs, inst, actions):
    """The closed length of [depot, actions] (get_tour_length's expression, ATen's arithmetic)."""
    rows = actions.shape[0]
    idx = torch.cat((torch.zeros(rows, 1, dtype=torch.int64), actions), 1)
    pts = locs[inst][torch.arange(rows)[:, None], idx]
    return (pts.roll(-1, 1) - pts).norm(p=2, dim=-1).sum(1)


def reward_w(env, data, actions):
    """The environment's get_reward on the CPU on the row as given (ATen's arithmetic, the reference's own expressions)."""
    inst = torch.arange(actions.shape[0]) % data["locs"].shape[0]
    if env == "op":
        return data["prize"][inst].gather(1, actions).sum(-1)
    penalty = data["penalty"][inst]
    return penalty.gather(1, actions).sum(-1) - (tour_length_w(data["locs"], inst, actions) + penalty[..., 1:].sum(-1))


def reward_scale(env, data, actions):
    """The magnitude the reward's ulps are counted in: OP the reward, PCTSP length + total penalty."""
    if env == "op":
        return reward_w(env, data, actions)
    inst = torch.arange(actions.shape[0]) % data["locs"].shape[0]
    return tour_length_w(data["locs"], inst, actions) + data["penalty"][inst][..., 1:].sum(-1)


def ulps(got, want, scale):
    """|got - want| in ulps of ``scale`` (fp32), 0 where they are equal."""
    unit = torch.finfo(torch.float32).eps * 2.0 ** torch.floor(torch.log2(scale.abs().double()))
    diff = (got.double() - want.double()).abs()
    return torch.where(diff == 0, torch.zeros_like(diff), diff / unit)


def record_data(env, rec):
    keys = ("locs", "prize", "max_length") if env == "op" else ("locs", "prize", "penalty")
    return {k: rec[k] for k in keys}


def random_data(env, b, n, seed, budget=1.2, prize_scale=None):
    """A seeded instance set in the generators' spirit: uniform locs; OP prizes by distance to the depot and the per-node table
    of budget ``budget``; PCTSP prizes U(0, prize_scale / C) (default 4) and penalties U(0, 3 / C)."""
    g = torch.Generator().manual_seed(seed)
    locs = torch.rand(b, n, 2, generator=g)
    to_depot = (locs[:, 0:1] - locs).norm(p=2, dim=-1)
    if env == "op":
        prize = (1 + (to_depot / to_depot.max(-1, keepdim=True).values * 99).int()).float() / 100
        prize[:, 0] = 0
        return {"locs": locs, "prize": prize, "max_length": torch.full((b, 1), budget) - to_depot - 1e-6}
    c = n - 1
    prize = torch.rand(b, n, generator=g) * ((4.0 if prize_scale is None else prize_scale) / c)
    penalty = torch.rand(b, n, generator=g) * (3.0 / c)
    prize[:, 0] = 0
    penalty[:, 0] = 0
    return {"locs": locs, "prize": prize, "penalty": penalty}


# ---- the recorder (needs the reference checkout) ------------------------------------------------------------------------------
def reference_run(env_name: str, case: str, seed=None) -> dict:
    """The reference's own AntSystem with its OPEnv / PCTSPEnv on the CPU in fp32, iteration by iteration as its ``run`` drives
    it, the sampler's multinomial replaced by the argmax of lp - ln_noise over recorded noise (the same distribution).
    Per iteration i: actions_i / logps_i / logps64_i [rows, T_i] (T_i the reference's own width, its longest row),
    masks_i [rows, T_i, n] (True = infeasible, the reference's action masks replayed along its actions), lengths [iters, rows],
    reward, final_reward, final_actions (zero-padded to W) with final_widths, pheromone; ln_noise [iters, W, rows, n]."""
    import importlib.util

    from oracle import ref_import

    ref = ref_import.load()
    spec = importlib.util.spec_from_file_location(
        "rl4co.models.zoo.deepaco.antsystem", ref_import.REFERENCE_ROOT / "rl4co/models/zoo/deepaco/antsystem.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    c, ants, b, iters, alpha, beta, decay, phe0, seeds = CASES[case]
    seed = seeds[env_name] if seed is None else seed
    n, rows = c + 1, ants * b
    w = width(n)
    torch.manual_seed(seed)
    if env_name == "op":  # (prize_distribution: as in oracle/gen_golden.py, the generator's default bounds are degenerate)
        env = ref.OPEnv(generator_params=dict(num_loc=c, prize_distribution="dist"))
    else:
        env = ref.PCTSPEnv(generator_params=dict(num_loc=c))
    td0 = env.reset(env.generator(batch_size=[b]))
    locs = td0["locs"].clone()
    heu = heuristic(locs)
    noise = ln_exp1((iters, w, rows, n), seed + 1)
    seen = {"it": 0}

    class Recording(mod.Sampling):
        def _step(self, logprobs, mask, td, **kwargs):
            t = seen.setdefault("t", 0)
            seen["t"] = t + 1
            return logprobs, select_rows(logprobs, noise[seen["it"], t], ~mask), td

        def post_decoder_hook(self, td, env_):
            seen["logps"] = torch.stack(self.logprobs, 1).clone()
            return super().post_decoder_hook(td, env_)

    mod.Sampling = Recording
    aco = mod.AntSystem(heu.clone(), n_ants=ants, alpha=alpha, beta=beta, decay=decay, pheromone=phe0)
    kwargs = dict(multisample=True, num_samples=ants, select_best=False)
    rec = {"locs": locs, "log_heuristic": heu, "pheromone0": aco.pheromone.clone(), "Q": f32(aco.Q), "ln_noise": noise}
    if env_name == "op":
        rec.update(prize=td0["prize"].clone(), max_length=td0["max_length"].clone())
    else:
        rec.update(prize=td0["real_prize"].clone(), penalty=td0["penalty"].clone())
    data = record_data(env_name, rec)
    keys = ("lengths", "reward", "final_reward", "final_actions", "final_widths", "pheromone")
    tab = {k: [] for k in keys}
    floor, worst = 0.0, 0.0
    idx = torch.arange(rows)
    for i in range(iters):
        before = aco.pheromone.clone()
        seen["it"], seen["t"] = i, 0
        actions, reward = aco._one_step(td0.clone(), env, kwargs)  # [B, ants, T], [B, ants]
        t_i = actions.shape[-1]
        actions = actions.transpose(0, 1).reshape(rows, t_i).contiguous()
        reward = reward.t().reshape(rows).contiguous()
        # the same steps replayed through the reference's env: its masks, its done flags, float64 through its process_logits
        lg64 = alpha * torch.log(before.double()) + beta * heu.double()
        lp64 = torch.zeros(rows, t_i, dtype=torch.float64)
        masks = torch.zeros(rows, t_i, n, dtype=torch.bool)
        lengths = torch.zeros(rows, dtype=torch.int32)
        td = ref.ops.batchify(td0.clone(), ants)
        was_done = torch.zeros(rows, dtype=torch.bool)
        for t in range(t_i):
            feasible = td["action_mask"].clone()
            masks[:, t] = ~feasible
            lp = ref.decoding.process_logits(lg64[idx % b, td["current_node"].reshape(-1)].clone(), feasible)
            lp64[:, t] = lp[idx, actions[:, t]]
            lengths += (~was_done).to(torch.int32)
            td.set("action", actions[:, t])
            td = env.step(td)["next"]
            was_done = td["done"].reshape(-1).clone()
        assert bool(was_done.all()) and int(lengths.max()) == t_i
        floor = max(floor, float((seen["logps"].double() - lp64).abs().max()))
        wide = pad(actions, w)
        worst = max(worst, float(ulps(reward_w(env_name, data, wide), reward, reward_scale(env_name, data, wide)).max()))
        rec[f"actions_{i}"], rec[f"logps_{i}"], rec[f"logps64_{i}"], rec[f"masks_{i}"] = actions, seen["logps"], lp64, masks
        finals = [t.clone() for t in aco.final_actions]
        for k, v in zip(keys, (lengths, reward, aco.final_reward.clone(), final_matrix(finals, w),
                               torch.tensor([len(t) for t in finals]), aco.pheromone.clone())):
            tab[k].append(v)
    rec.update({k: torch.stack(v, 0) for k, v in tab.items()})
    rec["noise_floor"] = torch.tensor(floor, dtype=torch.float64)
    rec["reward_ulps"] = torch.tensor(worst, dtype=torch.float64)
    return rec


def record(env_name: str, case: str) -> dict:
    from tests.helpers import reference_record

    return reference_record(f"aco_{env_name}_{case}", lambda: reference_run(env_name, case))


def coverage(env_name, rec, case):
    """What the data seeds are chosen for. OP: the rows that end early on budget (an unvisited customer was masked by the
    length test alone at the row's last step). PCTSP: per instance, whether some row returned before every customer was
    visited and whether some row visited all of them."""
    c, ants, b, iters = CASES[case][:4]
    if env_name == "op":
        early = 0
        for i in range(iters):
            actions, lengths, masks = rec[f"actions_{i}"], rec["lengths"][i].long(), rec[f"masks_{i}"]
            for r in range(actions.shape[0]):
                last = int(lengths[r]) - 1
                customers = set(actions[r, :last].tolist())
                early += int(0 not in customers and len(customers) < c and bool(masks[r, last, 1:].all()))
        return {"early": early}
    short, full = torch.zeros(b, dtype=torch.bool), torch.zeros(b, dtype=torch.bool)
    for i in range(iters):
        customers = rec["lengths"][i].long() - 1
        for r in range(customers.shape[0]):
            short[r % b] |= bool(customers[r] < c)
            full[r % b] |= bool(customers[r] == c)
    return {"short": short, "full": full}


if __name__ == "__main__":  # RL4CO_RECORD_REFERENCE=1 python -m tests.aco_prize_ref
    for env_name in ENVS:
        for name in CASES:
            r = record(env_name, name)
            iters = CASES[name][3]
            print(env_name, name, "noise_floor", float(r["noise_floor"]), "reward_w ulps", float(r["reward_ulps"]),
                  "widths", [r[f"actions_{i}"].shape[1] for i in range(iters)], "lengths", int(r["lengths"].min()),
                  int(r["lengths"].max()), coverage(env_name, r, name))
