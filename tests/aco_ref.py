"""Ant System on a heatmap (TSP): a plain-torch fp32 restatement of one iteration (heatmap logits -> masked log-softmax ->
key = lp - ln_noise -> lowest-index argmax; reward map; best-tour record; pheromone deposit with the ants added in order) and
the recorder of the reference's own ``AntSystem`` runs (tests/golden/reference/aco_*.npz). tests/test_aco_cpu.py pins the
restatement's update to the records bit for bit; the GPU tests compare the kernel with the restatement and the records.
Rows are ant-major everywhere: row ``j * B + b`` is ant ``j`` of instance ``b``."""
import torch

# case -> (N, ants, B, iterations, alpha, beta, decay, initial pheromone (None: ones), data seed)
CASES = {"tsp12_a5": (12, 5, 4, 3, 1.0, 1.0, 0.95, None, 1234), "tsp20_a20": (20, 20, 4, 3, 1.0, 1.0, 0.95, None, 1235),
         "tsp12_a5_ab": (12, 5, 4, 3, 0.7, 2.0, 0.8, 2, 1236)}
# Per-step tolerance of a kernel log-prob against the recorded reference or this restatement (fp32 both sides, another
# operation order and another exp / log): 4 x the largest deviation of the reference's OWN fp32 per-step log-probs from the
# same steps evaluated in float64, over the three records (the key "noise_floor" of each record; measured on the CPU).
MEASURED_NOISE_FLOOR = 4.655e-07  # tsp20_a20 (4.654e-07 rounded up); tsp12_a5 2.801e-07, tsp12_a5_ab 3.609e-07
STEP_TOL = 4 * MEASURED_NOISE_FLOOR


def f32(x):
    return torch.tensor(x, dtype=torch.float32)


def heuristic(locs):
    """-log(d + 1e9 I): classic ACO's visibility 1 / d as a log-heuristic, the diagonal out of the way."""
    d = (locs[:, :, None, :] - locs[:, None, :, :]).norm(p=2, dim=-1)
    return -torch.log(d + 1e9 * torch.eye(locs.shape[1]))


# ---- sampling ---------------------------------------------------------------------------------------------------------------
def logits(pheromone, log_heu, alpha, beta):
    return f32(alpha) * torch.log(pheromone) + f32(beta) * log_heu


def step_logps(row, visited, temperature=1.0):
    """[.., N] logits of the current node and the visited mask -> log-probs (visited nodes -inf)."""
    z = row.masked_fill(visited, float("-inf"))
    if temperature != 1.0:
        z = z / f32(temperature)
    return torch.log_softmax(z, -1)


def select(lp, ln_noise, visited):
    """Lowest-index argmax over the unvisited nodes of lp - ln_noise, one row."""
    key = (lp - ln_noise).masked_fill(visited, float("-inf"))
    key = torch.where(key != key, torch.full_like(key, float("-inf")), key)
    cand = (~visited).nonzero()[:, 0]
    best = key[cand].max()
    return int(cand[(key[cand] == best).nonzero()[0, 0]])


def sample(pheromone, log_heu, start_nodes, ln_noise, alpha=1.0, beta=1.0, temperature=1.0, forced=None):
    """One iteration's tours. start_nodes [rows], ln_noise [N - 1, rows, N] (None with ``forced`` [rows, N]).
    Returns actions [rows, N], logps [rows, N], all_logps [rows, N, N]."""
    b, n, _ = pheromone.shape
    rows = start_nodes.shape[0]
    lg = logits(pheromone, log_heu, alpha, beta)
    actions = torch.zeros(rows, n, dtype=torch.int64)
    logps = torch.zeros(rows, n)
    full = torch.zeros(rows, n, n)
    for r in range(rows):
        cur = int(start_nodes[r])
        visited = torch.zeros(n, dtype=torch.bool)
        visited[cur] = True
        actions[r, 0] = cur
        for t in range(1, n):
            lp = step_logps(lg[r % b, cur], visited, temperature)
            nxt = int(forced[r, t]) if forced is not None else select(lp, ln_noise[t - 1, r], visited)
            actions[r, t], logps[r, t], full[r, t] = nxt, lp[nxt], lp
            visited[nxt] = True
            cur = nxt
    return actions, logps, full


# ---- update -----------------------------------------------------------------------------------------------------------------
def reward_map(reward, q):
    """reward [B, ants] -> deposit per ant; NaN where all ants of an instance tie (not guarded, as the reference)."""
    hi = reward.max(-1, keepdim=True).values
    lo = reward.min(-1, keepdim=True).values
    x = (reward - lo) / (hi - lo)
    return (x * x) * f32(q)


def update(state, actions, reward, decay, q):
    """One iteration's update in place. state: {"pheromone" [B, N, N], "final_reward" [B] or None, "final_actions" [B, N] or
    None}; actions [rows, N], reward [rows]."""
    phe = state["pheromone"]
    b, n, _ = phe.shape
    ants = actions.shape[0] // b
    act = actions.view(ants, b, n)
    rew = reward.view(ants, b).t().contiguous()  # [B, ants]
    rows_b = torch.arange(b)
    best = torch.stack([(rew[i] == rew[i].max()).nonzero()[0, 0] for i in range(b)])  # the lowest ant at the maximum
    best_reward, best_actions = rew[rows_b, best], act[best, rows_b]
    if state["final_reward"] is None:
        state["final_reward"], state["final_actions"] = best_reward.clone(), best_actions.clone()
    else:
        take = state["final_reward"] <= best_reward  # equal rewards replace too
        state["final_reward"][take] = best_reward[take]
        state["final_actions"][take] = best_actions[take]
    v = reward_map(rew, q)
    delta = torch.zeros_like(phe)
    for j in range(ants):  # the ants in order: every edge's sum is built in this order
        for i in range(b):
            delta[i][act[j, i, :-1], act[j, i, 1:]] += v[i, j]
    delta[:, 0, 0] = 0
    phe.mul_(f32(decay))
    phe.add_(delta)
    return state


def fresh_state(pheromone):
    return {"pheromone": pheromone.clone(), "final_reward": None, "final_actions": None}


def tour_reward(locs, actions):
    """TSPEnv.get_reward on the CPU: minus the closed tour length (ATen's arithmetic, the reference's own expression)."""
    b = locs.shape[0]
    pts = locs[torch.arange(actions.shape[0]) % b][torch.arange(actions.shape[0])[:, None], actions]
    return -(pts.roll(-1, 1) - pts).norm(p=2, dim=-1).sum(1)


def ln_exp1(shape, seed):
    """The natural log of Exp(1) draws (the kernel's parity-mode noise)."""
    g = torch.Generator().manual_seed(seed)
    return torch.log(torch.empty(shape).exponential_(1, generator=g)).contiguous()


# ---- the recorder (needs the reference checkout) ------------------------------------------------------------------------------
def reference_run(case: str) -> dict:
    """The reference's own AntSystem with TSPEnv on the CPU in fp32, iteration by iteration as its ``run`` drives it."""
    import importlib.util

    from oracle import ref_import

    ref = ref_import.load()
    spec = importlib.util.spec_from_file_location(
        "rl4co.models.zoo.deepaco.antsystem", ref_import.REFERENCE_ROOT / "rl4co/models/zoo/deepaco/antsystem.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n, ants, b, iters, alpha, beta, decay, phe0, seed = CASES[case]
    torch.manual_seed(seed)
    env = ref.TSPEnv(generator_params=dict(num_loc=n))
    td0 = env.reset(env.generator(batch_size=[b]))
    locs = td0["locs"].clone()
    heu = heuristic(locs)
    gen = torch.Generator().manual_seed(seed + 1)
    starts = []

    def pick(td, env_, num_starts):
        s = torch.randint(0, n, (num_starts * b,), generator=gen)
        starts.append(s.clone())
        return s

    seen = {}

    class Recording(mod.Sampling):
        def post_decoder_hook(self, td, env_):
            seen["logps"] = torch.stack(self.logprobs, 1).clone()
            return super().post_decoder_hook(td, env_)

    mod.Sampling = Recording
    aco = mod.AntSystem(heu.clone(), n_ants=ants, alpha=alpha, beta=beta, decay=decay, pheromone=phe0)
    kwargs = dict(multistart=True, num_starts=ants, select_start_nodes_fn=pick, select_best=False)
    rec = {"locs": locs, "log_heuristic": heu, "pheromone0": aco.pheromone.clone(), "Q": f32(aco.Q)}
    keys = ("actions", "logps", "logps64", "reward", "final_reward", "final_actions", "pheromone")
    tab = {k: [] for k in keys}
    floor = 0.0
    for _ in range(iters):
        before = aco.pheromone.clone()
        actions, reward = aco._one_step(td0.clone(), env, kwargs)  # [B, ants, N], [B, ants]
        actions = actions.transpose(0, 1).reshape(ants * b, n).contiguous()
        reward = reward.t().reshape(ants * b).contiguous()
        # the same steps in float64, through the reference's own process_logits
        lg64 = alpha * torch.log(before.double()) + beta * heu.double()
        lp64 = torch.zeros(ants * b, n, dtype=torch.float64)
        mask = torch.ones(ants * b, n, dtype=torch.bool)
        idx = torch.arange(ants * b)
        mask[idx, actions[:, 0]] = False
        for t in range(1, n):
            lp = ref.decoding.process_logits(lg64[idx % b, actions[:, t - 1]].clone(), mask)
            lp64[:, t] = lp[idx, actions[:, t]]
            mask[idx, actions[:, t]] = False
        floor = max(floor, float((seen["logps"].double() - lp64).abs().max()))
        for k, v in zip(keys, (actions, seen["logps"], lp64, reward, aco.final_reward.clone(),
                               torch.stack(aco.final_actions, 0), aco.pheromone.clone())):
            tab[k].append(v)
    rec.update({k: torch.stack(v, 0) for k, v in tab.items()})
    rec["start_nodes"] = torch.stack(starts, 0)
    rec["noise_floor"] = torch.tensor(floor, dtype=torch.float64)
    return rec


def record(case: str) -> dict:
    from tests.helpers import reference_record

    return reference_record(f"aco_{case}", lambda: reference_run(case))


if __name__ == "__main__":  # RL4CO_RECORD_REFERENCE=1 python -m tests.aco_ref
    for name in CASES:
        r = record(name)
        print(name, float(r["noise_floor"]), {k: tuple(v.shape) for k, v in r.items()})
