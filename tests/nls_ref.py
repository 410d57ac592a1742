"""Neural-guided local search for TSP (DeepACO's NLS): (a) a CPU restatement of ``AntSystem.local_search`` with ``use_nls``
(antsystem.py:204-225) built on tests/two_opt_ref.two_opt and ATen's ``get_tour_length`` (tests/aco_ref.tour_reward), and
(b) the recorder that runs the reference's own ``AntSystem.local_search`` on CPU tensors (through oracle/ref_import.py, with
the stand-in ``numba`` of tests/two_opt_ref.py) and writes ``tests/golden/reference/nls_<case>.npz``. Helper of
tests/test_nls_cpu.py and tests/test_gpu_nls.py; not collected. Rows are ant-major: row ``r`` uses instance ``r % I``."""
import numpy as np
import torch

from tests import two_opt_ref as T
from tests.aco_ref import tour_reward


# ---- (a) the restatement ---------------------------------------------------------------------------------------------
def heuristic_dist(log_heuristic: torch.Tensor) -> torch.Tensor:
    """antsystem.py:78-85 on the CPU. [I, N, N] -> [I, N, N], 0 on the diagonal."""
    heuristic = log_heuristic.exp().detach().cpu() + 1e-10
    dist = 1 / (heuristic / heuristic.max(-1, keepdim=True)[0] + 1e-5)
    n = dist.shape[1]
    dist[:, torch.arange(n), torch.arange(n)] = 0
    return dist


def nls(locs, perturb_distances, tours, n_perturbations, ls_max_iterations=1000, perturb_max_iterations=1000):
    """``locs`` [I, N, 2], ``perturb_distances`` [I, N, N] (without the 1e9 diagonal), ``tours`` [R, T] with R % I == 0 ->
    (best tours int64 [R, T], best rewards fp32 [R], scans int32 [R, 1 + 2 P], accepted int32 [R])."""
    locs = locs.detach().cpu().float()
    tours = tours.detach().cpu().long()
    rows = tours.shape[0]
    inst = torch.arange(rows) % locs.shape[0]
    real = T.distance_matrix(locs)[inst]
    perturb = perturb_distances.detach().cpu().float()[inst]
    cur, s = T.two_opt(real, tours, ls_max_iterations)
    scans = [s]
    best, best_r = cur.clone(), tour_reward(locs, cur)
    accepted = torch.zeros(rows, dtype=torch.int32)
    for _ in range(n_perturbations):
        cur, s = T.two_opt(perturb, cur, perturb_max_iterations)
        scans.append(s)
        cur, s = T.two_opt(real, cur, ls_max_iterations)
        scans.append(s)
        r = tour_reward(locs, cur)
        win = r > best_r  # fp32 '>': NaN never wins
        best[win], best_r[win] = cur[win], r[win]
        accepted += win.to(torch.int32)
        # cur carries on whether or not it won (the reference's new_actions)
    return best, best_r, torch.stack(scans, 1), accepted


# ---- (b) the recorder (needs the reference checkout) -------------------------------------------------------------------
# case -> (N, ants, instances, n_perturbations, local_search_params, perturbation_params, data seed)
CASES = {
    "tsp12_a5_p2": (12, 5, 2, 2, {}, {"max_iterations": 5}, 2101),
    "tsp20_a4_p1": (20, 4, 2, 1, {}, {}, 2102),
    "tsp12_a3_p3_cap": (12, 3, 2, 3, {"max_iterations": 2}, {"max_iterations": 5}, 2103),  # the caps bind
}


def case_params(case: str) -> dict:
    """What a test passes to the restatement / the kernel for a record."""
    _, _, _, p, ls, pert, _ = CASES[case]
    return dict(n_perturbations=p, ls_max_iterations=ls.get("max_iterations", 1000),
                perturb_max_iterations=pert.get("max_iterations", 1000))


def case_inputs(case: str) -> dict:
    """Seeded coordinates, a heatmap that is a noisy function of distance (a learned heatmap's stand-in: close to 1 / d, wrong
    in places, so that some perturbed tours repair to something better and others do not) and random starting tours."""
    n, ants, b, _, _, _, seed = CASES[case]
    g = torch.Generator().manual_seed(seed)
    locs = torch.rand(b, n, 2, generator=g)
    d = T.distance_matrix(locs)
    log_heu = -torch.log(d + 1e9 * torch.eye(n)) + 0.75 * torch.randn(b, n, n, generator=g)
    tours = torch.stack([torch.randperm(n, generator=g) for _ in range(ants * b)])
    return {"locs": locs, "log_heuristic": log_heu, "in_actions": tours}


def reference_run(case: str) -> dict:
    """The reference's own ``AntSystem.local_search`` with ``use_nls=True`` and its TSPEnv on CPU tensors. The 2-opt under it
    is the reference's local_search.py run as plain Python; every scan is checked as in tests/two_opt_ref.reference_run (the
    stand-in compares the move threshold in fp32 where numba compares in double: no scan's best change may tell the two
    apart). Per round the record keeps which rows replaced their best tour."""
    import importlib
    import importlib.util

    from oracle import ref_import

    ls_mod = T._reference_module()
    ref = ref_import.load()
    env_mod = importlib.import_module("rl4co.envs.routing.tsp.env")
    spec = importlib.util.spec_from_file_location(
        "rl4co.models.zoo.deepaco.antsystem", ref_import.REFERENCE_ROOT / "rl4co/models/zoo/deepaco/antsystem.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    n, ants, b, n_pert, ls_params, pert_params, _ = CASES[case]
    data = case_inputs(case)
    once = ls_mod.two_opt_once

    def checked(distmat, tour, fixed_i=0):
        move = T.best_move(distmat, tour.astype(np.int64), T.pair_list(tour.shape[0]))
        if move is not None:
            assert bool(move[0] < np.float32(T.THRESHOLD)) == (float(move[0]) < T.THRESHOLD), (case, move)
        return once(distmat, tour, fixed_i)

    td_cls = ref.TensorDict
    had_search, had_cpu = env_mod.local_search, getattr(td_cls, "cpu", None)
    ls_mod.two_opt_once = checked
    env_mod.local_search = ls_mod.local_search  # (env.py imported it before the stand-in numba existed: None)
    td_cls.cpu = lambda self: self.to("cpu")    # the container stand-in has no .cpu(); no arithmetic in it
    rounds = []
    try:
        env = ref.TSPEnv(generator_params=dict(num_loc=n))
        replace = env.replace_selected_actions

        def recording(cur_actions, new_actions, selection_mask):
            rounds.append(selection_mask.clone())
            return replace(cur_actions, new_actions, selection_mask)

        env.replace_selected_actions = recording
        aco = mod.AntSystem(data["log_heuristic"].clone(), n_ants=ants, use_local_search=True, use_nls=True,
                            n_perturbations=n_pert, local_search_params=ls_params, perturbation_params=pert_params)
        td = td_cls({"locs": data["locs"].repeat(ants, 1, 1)}, batch_size=[ants * b])
        best_actions, best_rewards = aco.local_search(td, env, data["in_actions"].clone(), {})
    finally:
        ls_mod.two_opt_once = once
        env_mod.local_search = had_search
        if had_cpu is None:
            del td_cls.cpu
        else:
            td_cls.cpu = had_cpu
    won = torch.stack(rounds, 0)  # [n_perturbations, rows]
    # the record is what it is meant to be: some row took a perturbed tour, some row turned a round down
    assert bool(won.any()) and bool((~won).any()), (case, won.sum().item())
    rec = dict(data)
    rec["heuristic_dist"] = aco.heuristic_dist.clone()
    rec["best_actions"] = best_actions.to(torch.int64)
    rec["best_rewards"] = best_rewards.to(torch.float32)
    rec["accepted"] = won.sum(0).to(torch.int32)
    return rec


def record(case: str) -> dict:
    from tests.helpers import reference_record

    return reference_record(f"nls_{case}", lambda: reference_run(case))


if __name__ == "__main__":  # RL4CO_RECORD_REFERENCE=1 python -m tests.nls_ref
    for name in CASES:
        r = record(name)
        acts, rews, _, acc = nls(r["locs"], r["heuristic_dist"], r["in_actions"], **case_params(name))
        assert torch.equal(acts, r["best_actions"]) and torch.equal(rews, r["best_rewards"]), name
        assert torch.equal(acc, r["accepted"]), name
        print(name, {k: tuple(v.shape) for k, v in r.items()}, "accepted", r["accepted"].tolist(), "== restatement")
