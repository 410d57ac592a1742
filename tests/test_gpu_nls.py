"""Neural-guided local search on the MI355X (csrc/tsp_nls.hip, AntSystem(use_nls=True)): the fused launch against the
records of the reference's own AntSystem.local_search, against the CPU restatement (tests/nls_ref.py) at the shapes where
the kernel can go wrong, against the host composition of the kernels it fuses, on bad input, and through the class.
Every comparison is exact: there is no tolerance anywhere."""
from functools import lru_cache

import pytest
import torch

from rl4co_amd import _lib
from tests import nls_ref as R
from tests import two_opt_ref as T

pytestmark = pytest.mark.gpu


def _K():
    from rl4co_amd import kernels as K

    return K


def _kernel(acts, locs, pert, **kw):
    out = _K().tsp_nls(acts.cuda(), locs=locs.cuda(), perturb_distances=pert.cuda(), return_counts=True, **kw)
    return tuple(t.cpu() for t in out)


def _same(got, want):
    """(tours, rewards, scans, accepted) of the kernel and of the restatement, one by one."""
    for name, g, w in zip(("tours", "rewards", "scans", "accepted"), got, want):
        assert g.dtype == w.dtype and torch.equal(g, w), name


# ---- 1. the records ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
def test_records(case):
    rec = R.record(case)
    tours, rewards, scans, accepted = _kernel(rec["in_actions"], rec["locs"], rec["heuristic_dist"], **R.case_params(case))
    assert torch.equal(tours, rec["best_actions"])
    assert torch.equal(rewards, rec["best_rewards"])
    assert torch.equal(accepted, rec["accepted"])
    # a perturbed tour was taken somewhere, a round was turned down somewhere
    assert bool((accepted > 0).any()) and bool((accepted < R.case_params(case)["n_perturbations"]).any())
    if case != "tsp12_a3_p3_cap":  # (with the 2-opt capped at 2 scans every row gains in some round; elsewhere rows take none)
        assert bool((accepted == 0).any())
    _same((tours, rewards, scans, accepted),
          R.nls(rec["locs"], rec["heuristic_dist"], rec["in_actions"], **R.case_params(case)))


# ---- 2. seeded shapes against the restatement ------------------------------------------------------------------------------
def _inputs(rows, inst, n, seed, lattice=False):
    g = torch.Generator().manual_seed(seed)
    locs = torch.rand(inst, n, 2, generator=g)
    if lattice:  # small integers, asymmetric: many exactly equal changes, the lowest (i, j) decides
        pert = torch.randint(1, 4, (inst, n, n), generator=g).float()
    else:
        pert = torch.rand(inst, n, n, generator=g)
    acts = torch.stack([torch.randperm(n, generator=g) for _ in range(rows)])
    return acts, locs, pert


# id -> (rows, instances, N, lattice, n_perturbations, ls_max_iterations, perturb_max_iterations)
SHAPES = {
    "first_call": (6, 2, 12, False, 2, 1000, 5),
    "n2": (33, 3, 2, False, 2, 1000, 1000),        # no pairs
    "n3": (33, 3, 3, False, 2, 1000, 1000),        # one pair, always skipped
    "n5": (33, 11, 5, False, 3, 1000, 1000),
    "lattice12": (12, 4, 12, True, 3, 1000, 1000),
    "perturb_cap0": (8, 4, 12, False, 2, 1000, 0),  # every round turned down: the first 2-opt comes back
    "ls_cap0": (8, 4, 12, False, 2, 0, 1000),
    "no_rounds": (8, 4, 20, False, 0, 1000, 1000),
    "three_ants": (12, 4, 16, False, 2, 1000, 3),   # R = 3 I, distinct instances: a wrong r % I shows
    "wave_edge": (4, 2, 65, False, 2, 1000, 4),
    "tsp100": (3, 3, 100, False, 2, 1000, 5),      # several pairs per thread
}


@lru_cache(maxsize=None)
def _shape_case(name):
    rows, inst, n, lattice, p, ls, pm = SHAPES[name]
    acts, locs, pert = _inputs(rows, inst, n, seed=3000 + n + rows, lattice=lattice)
    kw = dict(n_perturbations=p, ls_max_iterations=ls, perturb_max_iterations=pm)
    return acts, locs, pert, kw, R.nls(locs, pert, acts, **kw)


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_against_the_restatement(name):
    acts, locs, pert, kw, want = _shape_case(name)
    got = _kernel(acts, locs, pert, **kw)
    _same(got, want)
    tours, rewards, scans, accepted = got
    if name == "perturb_cap0":
        first, _ = T.two_opt(T.distance_matrix(locs)[torch.arange(8) % 4], acts)
        assert torch.equal(tours, first) and not bool(accepted.any())
    if name == "lattice12":  # ties decided something: some perturbation search moved, on a matrix of three values
        assert bool((scans[:, 1::2] > 1).any())
    if name == "no_rounds":
        K = _K()
        tiled = locs.cuda()[torch.arange(8, device="cuda") % 4].contiguous()
        two_opt, iters = K.tsp_two_opt(acts.cuda(), locs=tiled, return_iterations=True)
        reward = K.tour_length(tiled, two_opt, prepend_depot=False, negate=True)
        assert torch.equal(tours, two_opt.cpu()) and torch.equal(rewards, reward.cpu())
        assert torch.equal(scans, iters.cpu()[:, None]) and scans.shape == (8, 1)


# ---- 3. both sides of the LDS tier ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over", [0, 1])
def test_both_sides_of_the_lds_tier(over):
    """N = lds_nodes: one matrix slot in LDS, restaged per phase; N = lds_nodes + 1: coordinates in LDS for the real
    phases, the perturbation matrix read from global memory."""
    n = _K().nls_lds_nodes() + over
    acts, locs, pert = _inputs(2, 2, n, seed=4000 + n)
    kw = dict(n_perturbations=4, ls_max_iterations=4, perturb_max_iterations=4)
    want = R.nls(locs, pert, acts, **kw)
    assert bool((want[2] == 4).all())  # every search ran into its cap: all nine phases did work
    _same(_kernel(acts, locs, pert, **kw), want)


# ---- 4. the composition the launch replaces ------------------------------------------------------------------------------------
def _composition(acts, locs, pert, n_perturbations, ls_max_iterations, perturb_max_iterations):
    """AntSystem.local_search(use_nls=True) written with the kernels the fused launch is made of: matrices tiled per ant,
    1 + 2 P two-opt launches, as many reward launches, compare / select glue."""
    from rl4co_amd.envs import TSPEnv

    K, env = _K(), TSPEnv(check_solution=False)
    rows, inst = acts.shape[0], locs.shape[0]
    td = {"locs": locs.repeat(rows // inst, 1, 1)}
    tiled = pert.repeat(rows // inst, 1, 1)
    cur, it = K.tsp_two_opt(acts, locs=td["locs"], max_iterations=ls_max_iterations, return_iterations=True)
    scans = [it]
    best, best_r = cur.clone(), env.get_reward(td, cur)
    for _ in range(n_perturbations):
        cur, it = K.tsp_two_opt(cur, distances=tiled, max_iterations=perturb_max_iterations, return_iterations=True)
        scans.append(it)
        cur, it = K.tsp_two_opt(cur, locs=td["locs"], max_iterations=ls_max_iterations, return_iterations=True)
        scans.append(it)
        r = env.get_reward(td, cur)
        win = r > best_r
        best, best_r = torch.where(win[:, None], cur, best), torch.where(win, r, best_r)
    return best, best_r, torch.stack(scans, 1)


def test_fused_equals_the_composition_on_the_device():
    acts, locs, pert = (t.cuda() for t in _inputs(40, 8, 50, seed=5050))
    kw = dict(n_perturbations=3, ls_max_iterations=1000, perturb_max_iterations=5)
    tours, rewards, scans, accepted = _K().tsp_nls(acts, locs=locs, perturb_distances=pert, return_counts=True, **kw)
    want_tours, want_rewards, want_scans = _composition(acts, locs, pert, **kw)
    assert torch.equal(tours, want_tours) and torch.equal(rewards, want_rewards) and torch.equal(scans, want_scans)
    assert bool((accepted > 0).any()) and bool((accepted < 3).any())
    again = _K().tsp_nls(acts, locs=locs, perturb_distances=pert, **kw)
    assert torch.equal(again[0], tours) and torch.equal(again[1], rewards)  # two runs are bit-identical


# ---- 5. bad input ------------------------------------------------------------------------------------------------------------
def test_bad_index_rows_pass_through():
    rec = R.record("tsp12_a5_p2")
    kw = R.case_params("tsp12_a5_p2")
    acts = rec["in_actions"].clone()
    acts[3, 7] = 12  # == N
    acts[8, 0] = -1
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    tours, rewards, scans, accepted = _kernel(acts, rec["locs"], rec["heuristic_dist"], err=err, **kw)
    assert int(err.item()) == _lib.EBIT_TOUR_INDEX
    good = torch.ones(10, dtype=torch.bool)
    good[[3, 8]] = False
    assert torch.equal(tours[~good], acts[~good]) and bool(rewards[~good].isnan().all())
    assert not bool(scans[~good].any()) and not bool(accepted[~good].any())
    assert torch.equal(tours[good], rec["best_actions"][good]) and torch.equal(rewards[good], rec["best_rewards"][good])
    assert torch.equal(accepted[good], rec["accepted"][good]) and bool((scans[good] > 0).all())
    with pytest.raises(AssertionError, match="tour index out of range"):
        _K().tsp_nls(acts.cuda(), locs=rec["locs"].cuda(), perturb_distances=rec["heuristic_dist"].cuda(), **kw)


# ---- 6. the class surface ------------------------------------------------------------------------------------------------------
def test_class_surface():
    from rl4co_amd import AntSystem
    from rl4co_amd.envs import get_env
    from rl4co_amd.tensordict import TensorDict

    dev = torch.device("cuda", 0)
    rec = R.record("tsp12_a5_p2")
    inst, n, ants = 2, 12, 5
    env = get_env("tsp", generator_params=dict(num_loc=n, device=dev), device=dev)
    td = env.reset(TensorDict({"locs": rec["locs"].to(dev)}, batch_size=[inst]))
    params = dict(use_local_search=True, use_nls=True, n_perturbations=2, perturbation_params={"max_iterations": 5})
    aco = AntSystem(rec["log_heuristic"].to(dev), n_ants=ants, **params)
    torch.manual_seed(3)
    tours, cache = aco.run(td, env, 3, dict(multistart=True, num_starts=ants, select_best=False))
    perm = torch.arange(n).expand(inst, n)
    assert tours.shape == (inst, n) and torch.equal(tours.cpu().sort(1).values, perm)
    its = {k: v.cpu() for k, v in aco.last_iterations.items()}
    assert torch.equal(its["actions"].reshape(-1, n).sort(1).values, torch.arange(n).expand(3 * ants * inst, n))
    assert sorted(cache) == [0, 1, 2] and all(bool((cache[i] >= cache[i - 1]).all()) for i in (1, 2))
    assert bool((its["reward"] >= its["sampled_reward"]).all()) and bool((its["reward"] > its["sampled_reward"]).any())
    assert torch.equal(env.get_reward(td, tours).cpu(), cache[2].cpu())

    # local_search on given tours is the restatement on the class's own perturbation matrix
    assert aco.heuristic_dist.is_cuda and aco.heuristic_dist.dtype == torch.float32
    got_actions, got_rewards = aco.local_search(td, env, rec["in_actions"].to(dev), {})
    want = R.nls(rec["locs"], aco.heuristic_dist.cpu(), rec["in_actions"], 2, perturb_max_iterations=5)
    assert got_actions.is_cuda and got_rewards.is_cuda
    assert torch.equal(got_actions.cpu(), want[0]) and torch.equal(got_rewards.cpu(), want[1])
    # The matrix is the reference's formula up to the device's exp: exp(x) and the row maximum within 2 ulp each of the
    # CPU's, then two divisions and two additions of half an ulp each, every one with relative condition <= 1: under
    # 8 ulp = 9.6e-7 relative. The bound allows twice that.
    assert torch.allclose(aco.heuristic_dist.cpu(), rec["heuristic_dist"], rtol=2e-6, atol=0)


class _Env:
    def __init__(self, name):
        self.name = name


def test_class_constructs_and_keeps_the_references_signature():
    """The host-side surface of a constructed object (the constructor refuses a heatmap on the CPU, so these run here)."""
    from rl4co_amd import AntSystem

    rec = R.record("tsp12_a5_p2")
    heu, td, acts = rec["log_heuristic"].cuda(), {"locs": rec["locs"].cuda()}, rec["in_actions"].cuda()
    aco = AntSystem(heu, n_ants=5, use_local_search=True, use_nls=True, n_perturbations=2,
                    perturbation_params={"max_iterations": 5})
    assert aco.use_nls and aco.use_local_search and aco.n_perturbations == 2
    assert aco.perturbation_params == {"max_iterations": 5} and aco.local_search_params == {}
    assert aco.heuristic_dist is aco.heuristic_dist and aco.heuristic_dist.shape == heu.shape
    with pytest.raises(AssertionError, match="use_nls requires use_local_search"):
        AntSystem(heu, n_ants=5, use_nls=True)
    # an unknown key is the TypeError the reference's env.local_search signature would raise; num_threads is ignored
    bad = AntSystem(heu, n_ants=5, use_local_search=True, use_nls=True, perturbation_params={"max_iterations": 5, "depth": 3})
    with pytest.raises(TypeError, match="depth"):
        bad.local_search(td, _Env("tsp"), acts, {})
    bad = AntSystem(heu, n_ants=5, use_local_search=True, use_nls=True, local_search_params={"first_improvement": True})
    with pytest.raises(TypeError, match="first_improvement"):
        bad.local_search(td, _Env("tsp"), acts, {})
    threads = AntSystem(heu, n_ants=5, use_local_search=True, use_nls=True, n_perturbations=2,
                        local_search_params={"num_threads": 4}, perturbation_params={"max_iterations": 5, "num_threads": 4})
    got, want = threads.local_search(td, _Env("tsp"), acts, {}), aco.local_search(td, _Env("tsp"), acts, {})
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(NotImplementedError, match="rl4co_tsp_nls"):  # tours on the CPU
        aco.local_search(td, _Env("tsp"), rec["in_actions"], {})
    # CVRP stays refused: local_search itself and, through run, use_local_search
    with pytest.raises(NotImplementedError, match="cvrp"):
        aco.local_search(td, _Env("cvrp"), acts, {})
    with pytest.raises(NotImplementedError, match="use_local_search is not served for cvrp"):
        aco.run(td, _Env("cvrp"), 1, dict(multisample=True, num_samples=5, select_best=False))
