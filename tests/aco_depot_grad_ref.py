"""DeepACO's training path on the depot graphs (CVRP, OP, PCTSP): the ants' log-likelihood and its gradient with respect to the
heatmap. The masks come from the existing fp32 restatements of the sampling kernels (tests/aco_cvrp_ref.py ``sample``,
tests/aco_prize_ref.py ``sample``, both with ``forced=``); the masked log-softmax and its autograd gradient are evaluated
here in float64 (or float32). The recorder runs the reference's own train path (``NonAutoregressivePolicy``, its
``Sampling``, ``CVRPEnv`` / ``OPEnv`` / ``PCTSPEnv``, a stand-in encoder whose output is a free parameter, multisample, CPU;
tests/golden/reference/aco_depot_grad_*.npz). tests/test_aco_depot_grad_cpu.py pins the restatement to the records; the GPU
tests compare the kernels with the records and the float64 restatement.
Node 0 is the depot, ``n`` counts it, rows are ant-major (row ``j * B + b`` is ant ``j`` of instance ``b``) and W wide."""
import torch

from tests import aco_cvrp_ref as CV
from tests import aco_prize_ref as PZ
from tests.aco_grad_ref import _FreeHeatmap, reference_policy_class
from tests.aco_ref import ln_exp1

ENVS = ("cvrp", "op", "pctsp")
# case -> (customers, ants, B, temperature, data seed per environment)
CASES = {"c10_a5": (10, 5, 4, 1.0, {"cvrp": 5234, "op": 6234, "pctsp": 7234}),
         "c20_a20_t07": (20, 20, 4, 0.7, {"cvrp": 5235, "op": 6236, "pctsp": 7235})}
# (op c20_a20_t07: with data seed 6235 the reward of the W-wide row differs from the reference's reward of the row trimmed to
# its batch's longest by 2 ulps — the association difference tests/aco_prize_ref.py describes — above the existing
# REWARD_ULPS = 1 that the older records measured; 6236, the next seed, gives 1 ulp. The gradient floor does not rest on it.)
# The gradient's tolerance against the float64 gradient: 4 x the largest deviation of the reference's OWN fp32 autograd
# gradient from the float64 one over the six records (the key "grad_noise_floor" of each record, measured by the recorder on
# the CPU, |grad_ll| <= 1) — the rule aco_grad_ref.GRAD_TOL uses.
GRAD_NOISE_FLOORS = {"cvrp_c10_a5": 1.769e-07, "cvrp_c20_a20_t07": 7.035e-07, "op_c10_a5": 1.433e-07,
                     "op_c20_a20_t07": 2.627e-07, "pctsp_c10_a5": 8.484e-08, "pctsp_c20_a20_t07": 5.689e-07}  # (each rounded up)
MEASURED_GRAD_NOISE_FLOOR = max(GRAD_NOISE_FLOORS.values())
GRAD_TOL = 4 * MEASURED_GRAD_NOISE_FLOOR
STEP_TOL = {"cvrp": CV.STEP_TOL, "op": PZ.STEP_TOL, "pctsp": PZ.STEP_TOL}        # the environments' existing tolerances
REWARD_ULPS = {"cvrp": CV.REWARD_ULPS, "op": PZ.REWARD_ULPS, "pctsp": PZ.REWARD_ULPS}


def width(env, n):
    return CV.width(n) if env == "cvrp" else PZ.width(n)


# ---- the fp32 restatements of the sampling kernels: rows and masks ------------------------------------------------------------
def replay(env, heatmap, data, actions=None, ln_noise=None, start_nodes=None, temperature=1.0, rows=None):
    """The fp32 restatement of the SAMPLE launch with a pheromone of ones: follows ``actions`` [rows, W] (forced) or samples
    from ``ln_noise`` [W, rows, n]. Returns actions, lengths, logps, all_logps [rows, W, n], masks [rows, W, n] (True =
    infeasible; rows of steps not taken are all False)."""
    ones = torch.ones_like(heatmap)
    if env == "cvrp":
        return CV.sample(ones, heatmap, data["demand"], data["vehicle_capacity"], start_nodes, ln_noise,
                         temperature=temperature, forced=actions, rows=rows)
    return PZ.sample(env, ones, heatmap, data, ln_noise, temperature=temperature, forced=actions, rows=rows)


def sample_rows(env, heatmap, data, ants, seed, start_nodes=None, temperature=1.0):
    """Valid random rows of the environment: the fp32 restatement sampling under recorded noise."""
    b, n, _ = heatmap.shape
    noise = ln_exp1((width(env, n), ants * b, n), seed)
    finite = torch.where(torch.isfinite(heatmap), heatmap, torch.full_like(heatmap, -1e4))  # (select needs finite keys)
    return replay(env, finite, data, ln_noise=noise, start_nodes=start_nodes, temperature=temperature, rows=ants * b)


# ---- the float64 restatement ----------------------------------------------------------------------------------------------------
def rollout_logps(heatmap, actions, lengths, masks, start_nodes=None, temperature=1.0):
    """heatmap [B, n, n] (float32 or float64, may require grad), actions [rows, W], lengths [rows], masks [rows, W, n] ->
    per-step log-probs [rows, W], 0 after each row's length (and at column 0 under multistart)."""
    b = heatmap.shape[0]
    rows, w = actions.shape
    inst = (torch.arange(rows) % b)[:, None].expand(rows, w)
    cur = torch.cat((torch.zeros(rows, 1, dtype=torch.int64), actions[:, :-1]), 1)  # the node each step leaves
    live = torch.arange(w)[None, :] < lengths[:, None].long()
    if start_nodes is not None:
        live = live.clone()
        live[:, 0] = False
    z = heatmap[inst, cur].masked_fill(masks, float("-inf"))
    if temperature != 1.0:
        z = z / temperature
    z = torch.where(live[:, :, None], z, torch.zeros_like(z))  # (dead steps: anything finite)
    lp = torch.log_softmax(z, -1).gather(2, actions[:, :, None]).squeeze(2)
    return torch.where(live, lp, torch.zeros_like(lp))


def logp_grad(heatmap, actions, lengths, masks, grad_ll, grad_steps=None, start_nodes=None, temperature=1.0, dtype=torch.float64):
    """(logps [rows, W], d sum_r(grad_ll[r] * ll[r] + sum_t grad_steps[r, t] * logps[r, t]) / d heatmap) in ``dtype``."""
    h = heatmap.detach().to(dtype).requires_grad_(True)
    logps = rollout_logps(h, actions, lengths, masks, start_nodes, temperature)
    total = (grad_ll.to(dtype) * logps.sum(1)).sum()
    if grad_steps is not None:
        total = total + (grad_steps.to(dtype) * logps).sum()
    (grad,) = torch.autograd.grad(total, h)
    return logps.detach(), grad


def record_data(env, rec):
    keys = {"cvrp": ("locs", "demand", "vehicle_capacity"), "op": ("locs", "prize", "max_length")}.get(env, ("locs", "prize", "penalty"))
    return {k: rec[k] for k in keys}


def reward_w(env, data, actions):
    return CV.reward_w(data["locs"], actions) if env == "cvrp" else PZ.reward_w(env, data, actions)


def reward_scale(env, data, actions):
    return CV.reward_w(data["locs"], actions) if env == "cvrp" else PZ.reward_scale(env, data, actions)


def kernel_data(env, data, device="cuda"):
    """The keywords of ``kernels.aco_depot_logp_grad`` for this instance set."""
    keys = {"cvrp": ("demand", "vehicle_capacity"), "op": ("locs", "max_length")}.get(env, ("prize",))
    return {k: data[k].to(device).contiguous() for k in keys}


def as_td(env, data, device="cuda"):
    """The reset-state keys ``heatmap_rollout(td=...)`` reads."""
    if env == "cvrp":
        td = {"demand": data["demand"], "vehicle_capacity": data["vehicle_capacity"]}
    elif env == "op":
        td = {"prize": data["prize"], "max_length": data["max_length"]}
    else:
        td = {"real_prize": data["prize"], "penalty": data["penalty"]}
    td["locs"] = data["locs"]
    return {k: v.to(device) for k, v in td.items()}


def random_data(env, b, n, seed, **kw):
    """Seeded instances: aco_prize_ref.random_data for OP / PCTSP; CVRP: uniform locs, demands U{1..9} / 30, capacity 1."""
    if env != "cvrp":
        return PZ.random_data(env, b, n, seed, **kw)
    g = torch.Generator().manual_seed(seed)
    locs = torch.rand(b, n, 2, generator=g)
    demand = torch.randint(1, 10, (b, n - 1), generator=g).float() / kw.get("demand_scale", 30.0)
    return {"locs": locs, "demand": demand, "vehicle_capacity": torch.ones(b)}


# ---- the recorder (needs the reference checkout) ------------------------------------------------------------------------------
def reference_run(env_name: str, case: str) -> dict:
    """The reference's own train path (ConstructivePolicy.forward, multisample sampling, its Sampling strategy and its
    environment) on the CPU in fp32, then the same steps in float64 through its own env masks and process_logits. Rows are
    zero-padded from the reference's width (its longest row) to W."""
    from oracle import ref_import

    ref = ref_import.load()
    policy_cls = reference_policy_class()
    c, ants, b, temperature, seeds = CASES[case]
    seed = seeds[env_name]
    n, rows = c + 1, ants * b
    w = width(env_name, n)
    torch.manual_seed(seed)
    if env_name == "cvrp":
        env = ref.CVRPEnv(generator_params=dict(num_loc=c))
    elif env_name == "op":  # (prize_distribution: as in tests/aco_prize_ref.py)
        env = ref.OPEnv(generator_params=dict(num_loc=c, prize_distribution="dist"))
    else:
        env = ref.PCTSPEnv(generator_params=dict(num_loc=c))
    td0 = env.reset(env.generator(batch_size=[b]))
    gen = torch.Generator().manual_seed(seed + 1)
    heatmap = 2.0 * torch.randn(b, n, n, generator=gen)
    grad_ll = torch.rand(rows, generator=gen) * 2 - 1  # |grad_ll| <= 1
    enc = _FreeHeatmap(heatmap)
    policy = policy_cls(enc, env_name=env_name, train_decode_type="sampling")
    out = policy(td0.clone(), env, phase="train", multisample=True, num_samples=ants, select_best=False,
                 temperature=temperature, return_actions=True, return_sum_log_likelihood=False)
    logps, actions, reward = out["log_likelihood"], out["actions"], out["reward"]  # [rows, T], [rows, T], [rows]
    t_ref = actions.shape[1]
    assert logps.shape == (rows, t_ref) and reward.shape == (rows,)
    (grad_ll * logps.sum(1)).sum().backward()
    grad32 = enc.heatmap.grad.clone()
    # the same steps in float64: the reference's env replayed along its actions, its masks, its process_logits
    h64 = heatmap.double().requires_grad_(True)
    idx = torch.arange(rows)
    td = ref.ops.batchify(td0.clone(), ants)
    cols = []
    lengths = torch.zeros(rows, dtype=torch.int32)
    was_done = torch.zeros(rows, dtype=torch.bool)
    for t in range(t_ref):
        lp = ref.decoding.process_logits(h64[idx % b, td["current_node"].reshape(-1)], td["action_mask"].clone(),
                                         temperature=temperature)
        cols.append(lp[idx, actions[:, t]])
        lengths += (~was_done).to(torch.int32)
        td.set("action", actions[:, t])
        td = env.step(td)["next"]
        was_done = td["done"].reshape(-1).clone()
    assert bool(was_done.all()) and int(lengths.max()) == t_ref
    logps64 = torch.stack(cols, 1)
    (grad64,) = torch.autograd.grad((grad_ll.double() * logps64.sum(1)).sum(), h64)
    rec = {"locs": td0["locs"].clone(), "heatmap": heatmap, "actions": CV.pad(actions, w), "lengths": lengths,
           "logps": CV.pad(logps.detach(), w), "logps64": CV.pad(logps64.detach(), w), "reward": reward.detach(),
           "grad_ll": grad_ll, "grad32": grad32, "grad64": grad64, "temperature": torch.tensor(temperature, dtype=torch.float64),
           "grad_noise_floor": (grad32.double() - grad64).abs().max()}
    if env_name == "cvrp":
        rec.update(demand=td0["demand"].clone(), vehicle_capacity=td0["vehicle_capacity"].reshape(-1).clone())
    elif env_name == "op":
        rec.update(prize=td0["prize"].clone(), max_length=td0["max_length"].clone())
    else:
        rec.update(prize=td0["real_prize"].clone(), penalty=td0["penalty"].clone())
    return rec


def record(env_name: str, case: str) -> dict:
    from tests.helpers import reference_record

    return reference_record(f"aco_depot_grad_{env_name}_{case}", lambda: reference_run(env_name, case))


if __name__ == "__main__":  # RL4CO_RECORD_REFERENCE=1 python -m tests.aco_depot_grad_ref
    for env_name in ENVS:
        for name in CASES:
            r = record(env_name, name)
            print(f"{env_name}_{name}", "grad_noise_floor", float(r["grad_noise_floor"]), "step floor",
                  float((r["logps"].double() - r["logps64"]).abs().max()), "lengths", int(r["lengths"].min()),
                  int(r["lengths"].max()), "width", r["actions"].shape[1])
