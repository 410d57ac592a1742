"""Greedy and top-k / top-p decoding of a heatmap (csrc/ant_system.h: filter_kept and ant_step<true>; rl4co_amd.aco
.heatmap_decode; rl4co_amd.NARGNNPolicy): what the tests compare against.

The rules of a step (feasible sets, state) are the existing restatements' — tests/aco_ref.py (tsp), tests/aco_cvrp_ref.py,
tests/aco_prize_ref.py, reached through tests/aco_depot_grad_ref.py's ``replay`` — and the kept set is
tests/topkp_ref.py's ``filter_f64``; nothing of either is restated here. A greedy rollout is those samplers in float64 under
noise of zeros (``argmax(lp - 0)``, the lowest node on equal values). ``step_table`` lays a launch's rows out step by step
(the node each step leaves, its infeasible mask, whether the step was taken), from which the kept sets, the cut margins,
the filtered log-probs and their float64 autograd gradient follow for all steps at once.

The recorder runs the reference's own ``NARGNNPolicy`` (models/zoo/nargnn/policy.py) with its own ``NARGNNEncoder`` in eval
mode on the CPU, TSP N = 11 and CVRP N = 12 with B = 3 (tests/gfacs_ref.py's sizes, tests/nargnn_ref.py's seeded weights):
``phase="val"`` and ``phase="test"`` (the latter with ``select_best``) under the default ``multistart_greedy``, and two
``phase="test", decode_type="multistart_sampling"`` runs with ``top_k=3`` and with ``top_k=5, top_p=0.8``
(tests/golden/reference/heatmap_decode_<env>_<case>.npz). Rows are ant-major, row ``j * B + b`` is ant ``j`` of instance
``b``; on a depot graph node 0 is the depot and ``n`` counts it."""
import json

import torch

from tests import aco_depot_grad_ref as DG
from tests import aco_ref as A
from tests import nargnn_depot_ref as RD
from tests import nargnn_ref as R
from tests.topkp_ref import filter_f64, top_p_entry_margins

NEG_INF = float("-inf")
ENVS = ("tsp", "cvrp", "op", "pctsp")
MARGIN = 1e-5        # a step whose float64 top-p cut is closer than this to a tie is left out (tests/test_gpu_topkp.py's rule)
LEFT_OUT_SHARE = 0.02  # at most this share of the compared steps


# ---- instances --------------------------------------------------------------------------------------------------------------
def grid_heatmap(b, n, seed):
    """[B, n, n] float32 whose every row is a permutation of DISTINCT multiples of a power of two in [-4, 4]: 1/8 up to 65
    nodes (the 65 multiples of 1/8 in [-4, 4]); above, where 65 values cannot be distinct, the largest step that still gives
    ``n`` values (1/32 up to 257 nodes). The values and their differences are exact in fp32 and far above the rounding of a
    log-softmax over them (|lp| < 16: ulp 1e-6), so no two log-probs merge and the float64 argmax is the fp32 one."""
    step = 0.125
    while 8.0 / step + 1 < n:
        step /= 2
    g = torch.Generator().manual_seed(seed)
    values = -4.0 + step * torch.arange(int(8.0 / step) + 1, dtype=torch.float32)
    rows = [values[torch.randperm(values.numel(), generator=g)[:n]] for _ in range(b * n)]
    return torch.stack(rows, 0).view(b, n, n)


def random_heatmap(b, n, seed):
    return 2.0 * torch.randn(b, n, n, generator=torch.Generator().manual_seed(seed))


def instance(env, b, n, seed):
    """The instance tensors by the references' names (``locs`` among them)."""
    if env == "tsp":
        return {"locs": torch.rand(b, n, 2, generator=torch.Generator().manual_seed(seed))}
    return DG.random_data(env, b, n, seed)


def as_td(env, data, device="cuda"):
    if env == "tsp":
        return {"locs": data["locs"].to(device)}
    return DG.as_td(env, data, device)


def width(env, n):
    return n if env == "tsp" else DG.width(env, n)


def tsp_starts(b, n, ants):
    return (torch.arange(ants) % n).repeat_interleave(b)


# ---- a greedy rollout: the existing samplers in float64 under noise of zeros ------------------------------------------------
def greedy_rollout(env, heatmap, data, ants, start_nodes=None):
    """actions [rows, W] of the float64 greedy rollout of ``heatmap`` [B, n, n] (``start_nodes`` [rows]: tsp always, cvrp
    under multistart)."""
    b, n, _ = heatmap.shape
    rows, w = ants * b, width(env, n)
    h64 = heatmap.double()
    if env == "tsp":
        return A.sample(torch.ones_like(h64), h64, start_nodes, torch.zeros(n - 1, rows, n, dtype=torch.float64))[0]
    # (the environment's state stays fp32, as the kernel's: only the logits are float64)
    return DG.replay(env, h64, data, ln_noise=torch.zeros(w, rows, n, dtype=torch.float64), start_nodes=start_nodes,
                     rows=rows)[0]


# ---- a launch's rows, step by step ------------------------------------------------------------------------------------------
def step_table(env, heatmap, data, actions, start_nodes=None):
    """(cur [rows, W], infeasible [rows, W, n], live [rows, W]) of given rows: the node every step leaves, the step's
    infeasible nodes (the environment's rule, from the existing fp32 restatements under ``forced=``) and whether the step
    was taken and scored (tsp: t >= 1; depot graphs: t < length, and t >= 1 under multistart)."""
    b, n, _ = heatmap.shape
    rows, w = actions.shape
    if env == "tsp":
        visited = torch.zeros(rows, w, n, dtype=torch.bool)
        for t in range(1, w):
            visited[:, t] = visited[:, t - 1]
            visited[torch.arange(rows), t, actions[:, t - 1]] = True
        cur = torch.cat((actions[:, :1], actions[:, :-1]), 1)
        live = torch.arange(w)[None, :].expand(rows, w) >= 1
        return cur, visited, live
    finite = torch.where(torch.isfinite(heatmap), heatmap, torch.full_like(heatmap, -1e4))
    _, lengths, _, _, masks = DG.replay(env, finite.float(), data, actions=actions, start_nodes=start_nodes)
    cur = torch.cat((torch.zeros(rows, 1, dtype=torch.int64), actions[:, :-1]), 1)
    live = torch.arange(w)[None, :] < lengths[:, None].long()
    if start_nodes is not None:
        live = live.clone()
        live[:, 0] = False
    return cur, masks, live


def step_logits(heatmap, cur, infeasible, temperature):
    """[rows, W, n] float64: the quotient the kernel forms (fp32 row / fp32 temperature), -inf on infeasible nodes."""
    b = heatmap.shape[0]
    rows, w = cur.shape
    inst = (torch.arange(rows) % b)[:, None].expand(rows, w)
    z = heatmap.float()[inst, cur]
    if temperature != 1.0:
        z = z / A.f32(temperature)
    return z.masked_fill(infeasible, NEG_INF).double()


def kept_sets(z, top_k, top_p):
    """(kept [rows, W, n] bool by ``filter_f64``, margin [rows, W]: the step's smallest float64 top-p cut margin)."""
    return filter_f64(z, top_k, top_p), top_p_entry_margins(z, top_k, top_p).min(-1).values


def filtered_logp_grad(heatmap, actions, cur, live, kept, weights, temperature=1.0):
    """(per-step log-probs [rows, W] float64, d sum_r weights[r] * ll[r] / d heatmap float64) of the masked, filtered
    log-softmax along ``actions``: float64 autograd, the kept sets as constants."""
    b = heatmap.shape[0]
    rows, w = actions.shape
    inst = (torch.arange(rows) % b)[:, None].expand(rows, w)
    h = heatmap.detach().double().requires_grad_(True)
    z = (h[inst, cur] / temperature).masked_fill(~kept, NEG_INF)
    z = torch.where(live[:, :, None], z, torch.zeros_like(z))  # (dead steps: anything finite)
    lp = torch.log_softmax(z, -1).gather(2, actions[:, :, None]).squeeze(2)
    lp = torch.where(live, lp, torch.zeros_like(lp))
    (grad,) = torch.autograd.grad((weights.double() * lp.sum(1)).sum(), h)
    return lp.detach(), grad


# ---- the recorder (needs the reference checkout) -----------------------------------------------------------------------------
BATCH = 3
# env -> (N, GNN layers, heatmap MLP layers, weight seed, data seed): tests/gfacs_ref.py's sizes
RECORD_ENVS = {"tsp": (11, 2, 2, 501, 601), "cvrp": (12, 2, 2, 502, 602)}
RECORD_CASES = {"val": dict(phase="val"), "test": dict(phase="test", select_best=True),
                "k3": dict(phase="test", decode_type="multistart_sampling", top_k=3),
                "k5_p08": dict(phase="test", decode_type="multistart_sampling", top_k=5, top_p=0.8)}
SAMPLE_SEED = 4321


def record_state_dict(env):
    n, layers, mlp_layers, wseed, _ = RECORD_ENVS[env]
    return R.make_state_dict(wseed, layers, mlp_layers) if env == "tsp" else RD.make_state_dict(env, wseed, layers, mlp_layers)


def reference_policy_class():
    """The reference's NARGNNPolicy, its file executed verbatim on the loaders of tests/aco_grad_ref.py (the constructive
    policy) and tests/nargnn_ref.py (the encoder, the stand-in ``torch_geometric``)."""
    import importlib

    from tests.aco_grad_ref import reference_policy_class as constructive

    constructive()
    R.reference_encoder_class()
    return importlib.import_module("rl4co.models.zoo.nargnn.policy").NARGNNPolicy


def reference_run(env_name, case):
    from oracle import ref_import

    ref = ref_import.load()
    n, layers, mlp_layers, _, dseed = RECORD_ENVS[env_name]
    policy = reference_policy_class()(env_name=env_name, num_layers_heatmap_generator=mlp_layers,
                                      num_layers_graph_encoder=layers)
    policy.encoder.load_state_dict(record_state_dict(env_name), strict=True)
    policy = policy.eval()
    env = {"tsp": ref.TSPEnv, "cvrp": ref.CVRPEnv}[env_name](generator_params=dict(num_loc=n if env_name == "tsp" else n - 1))
    torch.manual_seed(dseed)
    td0 = env.reset(env.generator(batch_size=[BATCH]))
    starts = []

    def pick(td, env_, num_starts):
        s = env_.select_start_nodes(td, num_starts=num_starts)
        starts.append(s.clone())
        return s

    kw = dict(RECORD_CASES[case])
    torch.manual_seed(SAMPLE_SEED)
    with torch.inference_mode():
        out = policy(td0.clone(), env, select_start_nodes_fn=pick, return_hidden=True, return_actions=True, **kw)
    assert len(starts) == 1
    rec = {"heatmap": out["hidden"], "start_nodes": starts[0], "actions": out["actions"],
           "log_likelihood": out["log_likelihood"], "reward": out["reward"], "locs": td0["locs"]}
    if env_name == "cvrp":
        rec["demand"], rec["vehicle_capacity"] = td0["demand"], td0["vehicle_capacity"].reshape(-1)
    return {k: v.detach().clone() for k, v in rec.items()}


def record(env_name, case):
    from tests.helpers import reference_record

    return reference_record(f"heatmap_decode_{env_name}_{case}", lambda: reference_run(env_name, case))


def reference_state_dict_shapes():
    """{environment: {key: shape}} of the reference's own ``NARGNNPolicy().state_dict()`` at the default depth."""
    cls = reference_policy_class()
    return {env: {k: list(v.shape) for k, v in cls(env_name=env).state_dict().items()} for env in ENVS}


def recorded_state_dict_shapes():
    import os

    from tests.helpers import REFERENCE_RECORDS

    path = REFERENCE_RECORDS / "nargnn_policy_state_dict_shapes.json"
    if os.environ.get("RL4CO_RECORD_REFERENCE") == "1":
        path.write_text(json.dumps(reference_state_dict_shapes(), indent=0) + "\n")
    return json.loads(path.read_text())


def reference_process_logits_rows(seed=11, rows=64, n=23):
    """Heatmap rows with masks through the reference's own ``process_logits`` (decoding.py:138-188) in float64: the finite
    entries of its log-probs for a few (top_k, top_p, temperature) settings."""
    from oracle import ref_import

    ref = ref_import.load()
    g = torch.Generator().manual_seed(seed)
    logits = 2.0 * torch.randn(rows, n, generator=g, dtype=torch.float64)
    # (no equal logits: the reference's torch.sort is not stable, so which of two equal logits top-p cuts is not its to say;
    # tests/test_topkp_cpu.py pins the ties of top-k)
    mask = torch.rand(rows, n, generator=g) < 0.7
    mask[:, 0] = True
    rec = {"logits": logits, "mask": mask}
    for i, (k, p, t) in enumerate(PROCESS_CASES):
        lp = ref.decoding.process_logits(logits.clone(), mask, temperature=t, top_p=p, top_k=k)
        rec[f"kept{i}"] = torch.isfinite(lp)
    return rec


PROCESS_CASES = ((1, 0.0, 1.0), (3, 0.0, 1.0), (40, 0.0, 1.0), (0, 0.5, 1.0), (0, 0.9, 0.7), (5, 0.8, 0.7))


def process_logits_record():
    from tests.helpers import reference_record

    return reference_record("heatmap_decode_process_logits", reference_process_logits_rows)


if __name__ == "__main__":  # RL4CO_RECORD_REFERENCE=1 python -m tests.heatmap_decode_ref
    for e in RECORD_ENVS:
        for c in RECORD_CASES:
            r = record(e, c)
            print(e, c, {k: tuple(v.shape) for k, v in r.items()})
    print({k: len(v) for k, v in recorded_state_dict_shapes().items()})
    print({k: tuple(v.shape) for k, v in process_logits_record().items()})
