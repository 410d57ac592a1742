"""Ant System on a heatmap (CVRP): a plain-torch fp32 restatement of one iteration (CVRPEnv's state and mask, heatmap logits
-> masked log-softmax -> key = lp - ln_noise -> lowest-index argmax, rows W wide and zero-filled after done; the reward of
the W-wide row; reward map; best-row record as the reference's ragged list; pheromone deposit with the ants added in order)
and the recorder of the reference's own ``AntSystem`` runs with its ``CVRPEnv`` (tests/golden/reference/aco_cvrp_*.npz).
tests/test_aco_cvrp_cpu.py pins the restatement to the records; the GPU tests compare the kernel with both. The pieces CVRP
shares with TSP (logits, log-softmax, selection, reward map, noise) are tests/aco_ref.py's. Node 0 is the depot, ``n`` counts
it, rows are ant-major: row ``j * B + b`` is ant ``j`` of instance ``b``."""
import torch

from tests.aco_ref import f32, heuristic, ln_exp1, logits, reward_map, select, step_logps  # noqa: F401

# case -> (customers, ants, B, iterations, alpha, beta, decay, initial pheromone (None: ones), data seed, entry mode)
CASES = {"c10_a5": (10, 5, 4, 3, 1.0, 1.0, 0.95, None, 2234, "multisample"),
         "c20_a20": (20, 20, 4, 3, 1.0, 1.0, 0.95, None, 2235, "multistart"),
         "c10_a5_ab": (10, 5, 4, 3, 0.7, 2.0, 0.8, 2, 2236, "multisample")}
# Per-step tolerance of a kernel log-prob against the recorded reference or this restatement (fp32 both sides, another
# operation order and another exp / log): 4 x the largest deviation of the reference's OWN fp32 per-step log-probs from the
# same steps evaluated in float64, over the three records (the key "noise_floor" of each record; measured on the CPU).
MEASURED_NOISE_FLOOR = 3.598e-07  # c10_a5_ab (3.5975e-07 rounded up); c10_a5 2.661e-07, c20_a20 3.573e-07
STEP_TOL = 4 * MEASURED_NOISE_FLOOR
# reward_w (the W-wide row) against the recorded reward (the row trimmed to its iteration's longest): both sum the same
# non-negative segments, the trailing ones exactly 0, in another association of ATen's 8-lane / 4-ILP cascade. Measured on
# the three records, in ulps of the tour length: c20_a20 2.0, c10_a5 0.0, c10_a5_ab 0.0 (python -m tests.aco_cvrp_ref prints
# them). The asserted bound is the largest measured one.
MEASURED_REWARD_ULPS = 2.0
REWARD_ULPS = MEASURED_REWARD_ULPS


def width(n):
    """W = max(C + 1, 2 C - 1): a row takes C + max(k, 1) actions, k <= C - 1 its mid-tour depot returns."""
    return max(n, 2 * n - 3)


# ---- CVRPEnv's state (cvrp/env.py:66-136) -----------------------------------------------------------------------------------
def fresh(n):
    """The reset state: at the depot, nothing visited (the depot neither), nothing loaded."""
    return {"cur": 0, "used": f32(0.0), "visited": torch.zeros(n, dtype=torch.bool)}


def step_state(state, a, demand):
    """One action. demand [C] of the instance."""
    c = demand.shape[0]
    state["used"] = (state["used"] + demand[min(max(a - 1, 0), c - 1)]) * f32(1.0 if a != 0 else 0.0)
    state["visited"][a] = True
    state["cur"] = a
    return state


def done(state):
    return bool(state["visited"].all())


def mask(state, demand, capacity):
    """[n] bool, True = INFEASIBLE (the complement of get_action_mask)."""
    loc = state["visited"][1:] | (demand + state["used"] > capacity + 1e-5)
    depot = torch.tensor([state["cur"] == 0 and bool((~loc).any())])
    return torch.cat((depot, loc))


# ---- sampling ---------------------------------------------------------------------------------------------------------------
def sample(pheromone, log_heu, demand, capacity, start_nodes, ln_noise, alpha=1.0, beta=1.0, temperature=1.0, forced=None,
           rows=None):
    """One iteration's rows. demand [B, C], capacity [B]; start_nodes [rows] (multistart) or None (multisample, ``rows``
    given or taken from ``forced`` / ``ln_noise``); ln_noise [W, rows, n] (None with ``forced`` [rows, W]).
    Returns actions [rows, W], lengths [rows], logps [rows, W], all_logps [rows, W, n], masks [rows, W, n] (True = infeasible;
    rows of steps not taken are all False)."""
    b, n, _ = pheromone.shape
    w = width(n)
    if rows is None:
        rows = start_nodes.shape[0] if start_nodes is not None else (forced.shape[0] if forced is not None else ln_noise.shape[1])
    lg = logits(pheromone, log_heu, alpha, beta)
    actions = torch.zeros(rows, w, dtype=torch.int64)
    lengths = torch.zeros(rows, dtype=torch.int32)
    logps = torch.zeros(rows, w)
    full = torch.zeros(rows, w, n)
    masks = torch.zeros(rows, w, n, dtype=torch.bool)
    for r in range(rows):
        i = r % b
        state = fresh(n)
        t = 0
        if start_nodes is not None:
            actions[r, 0] = int(start_nodes[r])
            step_state(state, int(start_nodes[r]), demand[i])
            t = 1
        while t < w and not done(state):
            m = mask(state, demand[i], capacity[i])
            lp = step_logps(lg[i, state["cur"]], m, temperature)
            nxt = int(forced[r, t]) if forced is not None else select(lp, ln_noise[t, r], m)
            actions[r, t], logps[r, t], full[r, t], masks[r, t] = nxt, lp[nxt], lp, m
            step_state(state, nxt, demand[i])
            t += 1
        lengths[r] = t
    return actions, lengths, logps, full, masks


def reward_w(locs, actions):
    """CVRPEnv.get_reward on the CPU on the row as given (the depot prepended, ATen's arithmetic): minus the closed length."""
    rows = actions.shape[0]
    idx = torch.cat((torch.zeros(rows, 1, dtype=torch.int64), actions), 1)
    pts = locs[torch.arange(rows) % locs.shape[0]][torch.arange(rows)[:, None], idx]
    return -(pts.roll(-1, 1) - pts).norm(p=2, dim=-1).sum(1)


# ---- update -----------------------------------------------------------------------------------------------------------------
def update(state, actions, reward, decay, q, keep=None):
    """One iteration's update in place. state: {"pheromone" [B, n, n], "final_reward" [B] or None, "final_actions": list of
    B ragged rows or None}; actions [rows, T], reward [rows]. ``keep``: the width the reference's batch had in this
    iteration (its longest row) when ``actions`` is wider; the record's entries are that wide (antsystem.py:238-245)."""
    phe = state["pheromone"]
    b, n, _ = phe.shape
    ants = actions.shape[0] // b
    act = actions.view(ants, b, -1)
    rew = reward.view(ants, b).t().contiguous()  # [B, ants]
    rows_b = torch.arange(b)
    best = torch.stack([(rew[i] == rew[i].max()).nonzero()[0, 0] for i in range(b)])  # the lowest ant at the maximum
    best_reward, best_actions = rew[rows_b, best], act[best, rows_b][:, :keep]
    if state["final_reward"] is None:
        state["final_reward"], state["final_actions"] = best_reward.clone(), list(best_actions.clone())
    else:
        take = state["final_reward"] <= best_reward  # equal rewards replace too
        state["final_reward"][take] = best_reward[take]
        for i in take.nonzero()[:, 0].tolist():
            state["final_actions"][i] = best_actions[i].clone()
    v = reward_map(rew, q)
    delta = torch.zeros_like(phe)
    for j in range(ants):  # the ants in order: every edge's sum is built in this order
        for i in range(b):
            delta[i][act[j, i, :-1], act[j, i, 1:]] += v[i, j]
    delta[:, 0, 0] = 0  # the trailing zeros
    phe.mul_(f32(decay))
    phe.add_(delta)
    return state


def fresh_state(pheromone):
    return {"pheromone": pheromone.clone(), "final_reward": None, "final_actions": None}


def final_matrix(final_actions, w=None):
    """The ragged list zero-padded to ``w`` (default: the longest entry, antsystem.py:284-294)."""
    w = max(len(t) for t in final_actions) if w is None else w
    return torch.stack([torch.nn.functional.pad(t, (0, w - len(t))) for t in final_actions], 0)


def pad(actions, w):
    return torch.nn.functional.pad(actions, (0, w - actions.shape[-1]))


# ---- the recorder (needs the reference checkout) ------------------------------------------------------------------------------
def reference_run(case: str) -> dict:
    """The reference's own AntSystem with its CVRPEnv on the CPU in fp32, iteration by iteration as its ``run`` drives it.
    Per iteration i: actions_i / logps_i / logps64_i [rows, T_i] (T_i the reference's own width, its longest row),
    masks_i [rows, T_i, n] (True = infeasible, the reference's action masks replayed along its actions), lengths [iters, rows],
    reward, final_reward, final_actions (zero-padded to W) with final_widths, pheromone."""
    import importlib.util

    from oracle import ref_import

    ref = ref_import.load()
    spec = importlib.util.spec_from_file_location(
        "rl4co.models.zoo.deepaco.antsystem", ref_import.REFERENCE_ROOT / "rl4co/models/zoo/deepaco/antsystem.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    c, ants, b, iters, alpha, beta, decay, phe0, seed, mode = CASES[case]
    n, rows = c + 1, ants * b
    w = width(n)
    torch.manual_seed(seed)
    env = ref.CVRPEnv(generator_params=dict(num_loc=c))
    td0 = env.reset(env.generator(batch_size=[b]))
    locs = td0["locs"].clone()
    heu = heuristic(locs)
    gen = torch.Generator().manual_seed(seed + 1)
    starts = []

    def pick(td, env_, num_starts):
        s = torch.randint(1, n, (num_starts * b,), generator=gen)
        starts.append(s.clone())
        return s

    seen = {}

    class Recording(mod.Sampling):
        def post_decoder_hook(self, td, env_):
            seen["logps"] = torch.stack(self.logprobs, 1).clone()
            return super().post_decoder_hook(td, env_)

    mod.Sampling = Recording
    aco = mod.AntSystem(heu.clone(), n_ants=ants, alpha=alpha, beta=beta, decay=decay, pheromone=phe0)
    if mode == "multistart":
        kwargs = dict(multistart=True, num_starts=ants, select_start_nodes_fn=pick, select_best=False)
    else:
        kwargs = dict(multisample=True, num_samples=ants, select_best=False)
    rec = {"locs": locs, "demand": td0["demand"].clone(), "vehicle_capacity": td0["vehicle_capacity"].reshape(-1).clone(),
           "log_heuristic": heu, "pheromone0": aco.pheromone.clone(), "Q": f32(aco.Q)}
    keys = ("lengths", "reward", "final_reward", "final_actions", "final_widths", "pheromone")
    tab = {k: [] for k in keys}
    floor = 0.0
    idx = torch.arange(rows)
    for i in range(iters):
        before = aco.pheromone.clone()
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
            if t > 0 or mode != "multistart":
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
        rec[f"actions_{i}"], rec[f"logps_{i}"], rec[f"logps64_{i}"], rec[f"masks_{i}"] = actions, seen["logps"], lp64, masks
        finals = [t.clone() for t in aco.final_actions]
        for k, v in zip(keys, (lengths, reward, aco.final_reward.clone(), final_matrix(finals, w),
                               torch.tensor([len(t) for t in finals]), aco.pheromone.clone())):
            tab[k].append(v)
    rec.update({k: torch.stack(v, 0) for k, v in tab.items()})
    if starts:
        rec["start_nodes"] = torch.stack(starts, 0)
    rec["noise_floor"] = torch.tensor(floor, dtype=torch.float64)
    return rec


def record(case: str) -> dict:
    from tests.helpers import reference_record

    return reference_record(f"aco_cvrp_{case}", lambda: reference_run(case))


def record_finals(rec, i):
    """The record's ragged final_actions after iteration i."""
    return [rec["final_actions"][i][k, : int(rec["final_widths"][i][k])] for k in range(rec["final_actions"].shape[1])]


if __name__ == "__main__":  # RL4CO_RECORD_REFERENCE=1 python -m tests.aco_cvrp_ref
    for name in CASES:
        r = record(name)
        iters = CASES[name][3]
        ulps = 0.0
        for i in range(iters):
            got = reward_w(r["locs"], pad(r[f"actions_{i}"], width(r["locs"].shape[1])))
            ulps = max(ulps, float(((got - r["reward"][i]).abs() / torch.finfo(torch.float32).eps
                                    / 2.0 ** torch.floor(torch.log2(r["reward"][i].abs()))).max()))
        print(name, "noise_floor", float(r["noise_floor"]), "reward_w ulps", ulps,
              "widths", [r[f"actions_{i}"].shape[1] for i in range(iters)], "lengths", int(r["lengths"].min()), int(r["lengths"].max()))
