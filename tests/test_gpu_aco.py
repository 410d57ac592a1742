"""Ant System search on the MI355X (csrc/aco_tsp.hip, rl4co_amd/aco.py): the update against the records of the reference's
own AntSystem and the CPU restatement (tests/aco_ref.py) with no tolerance, the per-step log-probs within STEP_TOL (4 x the
reference's own fp32-vs-float64 deviation), the selection rule exactly, fused against split launches bit for bit on both
sides of the LDS tier, the class surface, and the sticky error bits on inputs the kernel has to survive."""
from functools import lru_cache

import pytest
import torch

from rl4co_amd import _lib
from tests import aco_ref as R

pytestmark = pytest.mark.gpu
SAMPLE, UPDATE = _lib.ACO_SAMPLE, _lib.ACO_UPDATE


def _K():
    from rl4co_amd import kernels as K

    return K


def _cpu(out):
    return {k: v.cpu() for k, v in out.items()}


def _is_permutation(actions, n):
    flat = actions.reshape(-1, n)
    return torch.equal(flat.sort(1).values, torch.arange(n).expand(flat.shape[0], n))


def _update_launch(phe, actions, reward, state, decay, q, n_ants):
    """One UPDATE-only launch on device copies; ``state``: None or (final_reward, final_actions) on the device."""
    kw = {} if state is None else dict(final_reward=state[0], final_actions=state[1], has_best=True)
    out = _K().aco_tsp(phe, n_ants=n_ants, phases=UPDATE, actions=actions.cuda(), reward=reward.cuda(), decay=decay, Q=q, **kw)
    return out["final_reward"], out["final_actions"], out["final_reward_cache"]


# ---- 1. the update against the records -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
def test_update_equals_the_record(case):
    rec = R.record(case)
    n, ants, b, iters, alpha, beta, decay, phe0, _ = R.CASES[case]
    phe = rec["pheromone0"].cuda()
    state = None
    for i in range(iters):
        fr, fa, cache = _update_launch(phe, rec["actions"][i], rec["reward"][i], state, decay, float(rec["Q"]), ants)
        state = (fr, fa)
        assert torch.equal(phe.cpu(), rec["pheromone"][i])
        assert torch.equal(fr.cpu(), rec["final_reward"][i]) and torch.equal(cache.cpu()[0], rec["final_reward"][i])
        assert torch.equal(fa.cpu(), rec["final_actions"][i])


def test_update_with_equal_rewards_is_nan_where_the_restatement_is():
    g = torch.Generator().manual_seed(5)
    b, n, ants = 3, 9, 4
    acts = torch.stack([torch.randperm(n, generator=g) for _ in range(ants * b)])
    reward = -torch.rand(ants * b, generator=g) - 1
    reward.view(ants, b)[:, 1] = -2.5  # instance 1: every ant the same reward -> 0 / 0
    want = R.update(R.fresh_state(torch.full((b, n, n), 1.5)), acts, reward, 0.9, 0.3)
    phe = torch.full((b, n, n), 1.5).cuda()
    fr, fa, _ = _update_launch(phe, acts, reward, None, 0.9, 0.3, ants)
    got = phe.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want["pheromone"])) and bool(torch.isnan(got[1]).any())
    assert not bool(torch.isnan(got[0]).any()) and not bool(torch.isnan(got[2]).any())
    assert torch.equal(got.nan_to_num(7.0), want["pheromone"].nan_to_num(7.0))
    assert torch.equal(fr.cpu(), want["final_reward"]) and torch.equal(fa.cpu(), want["final_actions"])
    assert torch.equal(fa.cpu()[1], acts[1])  # the lowest ant (ant 0, row 0 * B + 1) on equal rewards


def test_update_with_one_ant():
    g = torch.Generator().manual_seed(6)
    b, n = 2, 7
    acts = torch.stack([torch.randperm(n, generator=g) for _ in range(b)])
    reward = -torch.rand(b, generator=g) - 1
    want = R.update(R.fresh_state(torch.ones(b, n, n)), acts, reward, 0.95, 1.0)
    phe = torch.ones(b, n, n).cuda()
    fr, fa, _ = _update_launch(phe, acts, reward, None, 0.95, 1.0, 1)
    assert torch.equal(torch.isnan(phe.cpu()), torch.isnan(want["pheromone"])) and bool(torch.isnan(phe).any())
    assert torch.equal(phe.cpu().nan_to_num(7.0), want["pheromone"].nan_to_num(7.0))
    assert torch.equal(fr.cpu(), reward) and torch.equal(fa.cpu(), acts)


# ---- 2. evaluate against the records -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
def test_evaluate_equals_the_record(case):
    from rl4co_amd.envs import TSPEnv

    rec = R.record(case)
    n, ants, b, iters, alpha, beta, decay, phe0, _ = R.CASES[case]
    locs = rec["locs"].cuda()
    before = rec["pheromone0"]
    for i in range(iters):
        phe = before.cuda()
        out = _K().aco_tsp(phe, n_ants=ants, phases=SAMPLE, log_heuristic=rec["log_heuristic"].cuda(), locs=locs,
                           start_nodes=rec["start_nodes"][i][None].contiguous().cuda(), alpha=alpha, beta=beta,
                           forced_actions=rec["actions"][i].cuda())
        dev = float((out["logps"].cpu() - rec["logps"][i]).abs().max())
        print(f"{case} iteration {i}: largest per-step log-prob deviation {dev:.3e} (STEP_TOL {R.STEP_TOL:.3e})")
        assert dev <= R.STEP_TOL
        assert torch.equal(out["actions"].cpu(), rec["actions"][i]) and torch.equal(phe.cpu(), before)
        env_reward = TSPEnv(generator_params=dict(num_loc=n)).get_reward({"locs": locs}, out["actions"])
        assert torch.equal(out["reward"], env_reward) and torch.equal(out["reward"].cpu(), rec["reward"][i])
        before = rec["pheromone"][i]


# ---- 3. the selection rule -----------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _instance(b, n, seed):
    g = torch.Generator().manual_seed(seed)
    locs = torch.rand(b, n, 2, generator=g)
    return locs, R.heuristic(locs), 0.5 + torch.rand(b, n, n, generator=g)


@pytest.mark.parametrize("n,ants", [(5, 5), (65, 8), (5, 8), (65, 5)])
@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_selection_is_the_lowest_index_argmax(n, ants, temperature):
    b = 3
    rows = ants * b
    locs, heu, phe0 = _instance(b, n, 100 + n)
    g = torch.Generator().manual_seed(n * ants)
    starts = torch.randint(0, n, (1, rows), generator=g)
    noise = R.ln_exp1((1, n - 1, rows, n), seed=n + ants)
    out = _cpu(_K().aco_tsp(phe0.cuda(), n_ants=ants, log_heuristic=heu.cuda(), locs=locs.cuda(), start_nodes=starts.cuda(),
                            ln_noise=noise.cuda(), temperature=temperature, alpha=0.9, beta=1.3, all_logps=True))
    acts, logps, full = out["actions"], out["logps"], out["all_logps"]
    assert _is_permutation(acts, n) and torch.equal(acts[:, 0], starts[0])
    assert bool((logps[:, 0] == 0).all()) and bool((logps[:, n - 1] == 0).all()) and bool((full[:, 0] == 0).all())
    for r in range(rows):
        visited = torch.zeros(n, dtype=torch.bool)
        visited[acts[r, 0]] = True
        for t in range(1, n):
            assert bool((full[r, t][visited] == float("-inf")).all()) and bool(torch.isfinite(full[r, t][~visited]).all())
            assert R.select(full[r, t], noise[0, t - 1, r], visited) == int(acts[r, t]), (r, t)
            assert float(logps[r, t]) == float(full[r, t, acts[r, t]])
            visited[acts[r, t]] = True
    _, ref_logps, ref_full = R.sample(phe0, heu, starts[0], None, 0.9, 1.3, temperature, forced=acts)
    finite = torch.isfinite(ref_full)
    assert torch.equal(finite, torch.isfinite(full))
    dev = float((full[finite] - ref_full[finite]).abs().max())
    print(f"N {n} ants {ants} T {temperature}: largest log-prob deviation from the restatement {dev:.3e}")
    assert dev <= R.STEP_TOL and float((logps - ref_logps).abs().max()) <= R.STEP_TOL


# ---- 4. fused equals split -------------------------------------------------------------------------------------------------
def _fused(phe, n_ants, iters, heu, locs, starts, noise, **kw):
    return _cpu(_K().aco_tsp(phe, n_ants=n_ants, iterations=iters, log_heuristic=heu.cuda(), locs=locs.cuda(),
                             start_nodes=starts.cuda(), ln_noise=noise.cuda(), record_iterations=True, **kw))


def test_fused_equals_split_launches():
    b, n, ants, iters = 3, 21, 6, 3
    rows = ants * b
    locs, heu, phe0 = _instance(b, n, 77)
    g = torch.Generator().manual_seed(3)
    starts = torch.randint(0, n, (iters, rows), generator=g)
    noise = R.ln_exp1((iters, n - 1, rows, n), seed=4)
    kw = dict(alpha=1.1, beta=0.8, decay=0.9, Q=0.25)
    phe_f = phe0.cuda()
    fused = _fused(phe_f, ants, iters, heu, locs, starts, noise, **kw)
    phe_s = phe0.cuda()
    state = {}
    for i in range(iters):
        s = _K().aco_tsp(phe_s, n_ants=ants, phases=SAMPLE, log_heuristic=heu.cuda(), locs=locs.cuda(),
                         start_nodes=starts[i : i + 1].contiguous().cuda(), ln_noise=noise[i : i + 1].contiguous().cuda(), **kw)
        assert torch.equal(s["actions"].cpu(), fused["iter_actions"][i]) and torch.equal(s["reward"].cpu(), fused["iter_reward"][i])
        u = _K().aco_tsp(phe_s, n_ants=ants, phases=UPDATE, actions=s["actions"], reward=s["reward"], has_best=bool(state),
                         **state, **kw)
        state = dict(final_reward=u["final_reward"], final_actions=u["final_actions"])
        assert torch.equal(u["final_reward"].cpu(), fused["final_reward_cache"][i])
    assert torch.equal(phe_s, phe_f) and not torch.equal(phe_f.cpu(), phe0)
    assert torch.equal(state["final_reward"].cpu(), fused["final_reward"])
    assert torch.equal(state["final_actions"].cpu(), fused["final_actions"])
    assert torch.equal(fused["actions"], fused["iter_actions"][-1]) and torch.equal(fused["reward"], fused["iter_reward"][-1])


@pytest.mark.parametrize("side", [0, 1], ids=["lds", "global"])
def test_both_sides_of_the_lds_tier_follow_the_restatement(side):
    n = _K().aco_lds_nodes() + side
    b, ants, iters = 2, 4, 2
    rows = ants * b
    locs, heu, phe0 = _instance(b, n, 900 + side)
    g = torch.Generator().manual_seed(side)
    starts = torch.randint(0, n, (iters, rows), generator=g)
    noise = R.ln_exp1((iters, n - 1, rows, n), seed=10 + side)
    phe = phe0.cuda()
    out = _fused(phe, ants, iters, heu, locs, starts, noise, decay=0.9, Q=0.5)
    assert _is_permutation(out["iter_actions"], n)
    assert torch.equal(out["iter_reward"].reshape(-1), R.tour_reward(locs, out["iter_actions"].reshape(-1, n)))
    state = R.fresh_state(phe0)
    for i in range(iters):
        R.update(state, out["iter_actions"][i], out["iter_reward"][i], 0.9, 0.5)
        assert torch.equal(state["final_reward"], out["final_reward_cache"][i])
    assert torch.equal(phe.cpu(), state["pheromone"])
    assert torch.equal(out["final_reward"], state["final_reward"]) and torch.equal(out["final_actions"], state["final_actions"])


# ---- 5. the class surface --------------------------------------------------------------------------------------------------
KW = dict(multistart=True, num_starts=8, select_best=False)


@lru_cache(maxsize=None)
def _problem():
    from rl4co_amd.envs import TSPEnv

    torch.manual_seed(11)
    env = TSPEnv(generator_params=dict(num_loc=20))
    td = env.reset(batch_size=[6])
    return env, td, R.heuristic(td["locs"].cpu()).cuda()


def _run(seed, n_iterations=4, **kw):
    from rl4co_amd import AntSystem

    env, td, heu = _problem()
    aco = AntSystem(heu, n_ants=8, **kw)
    torch.manual_seed(seed)
    tours, cache = aco.run(td, env, n_iterations, KW)
    return aco, tours, cache


def _replay_identity(aco, tours, cache, n_iterations):
    env, td, heu = _problem()
    assert tours.shape == (6, 20) and _is_permutation(tours.cpu(), 20) and sorted(cache) == list(range(n_iterations))
    its = _cpu(aco.last_iterations)
    state = R.fresh_state(torch.ones(6, 20, 20))
    for i in range(n_iterations):
        R.update(state, its["actions"][i], its["reward"][i], aco.decay, aco.Q)
        assert torch.equal(cache[i].cpu(), state["final_reward"])
        assert torch.equal(env.get_reward(td, state["final_actions"].cuda()).cpu(), cache[i].cpu())
        assert i == 0 or bool((cache[i] >= cache[i - 1]).all())
    assert torch.equal(aco.pheromone.cpu(), state["pheromone"])
    assert torch.equal(tours.cpu(), state["final_actions"]) and torch.equal(aco.final_reward.cpu(), state["final_reward"])
    assert len(aco.final_actions) == 6 and all(t.shape == (20,) for t in aco.final_actions)
    return its


def test_class_surface_run():
    aco, tours, cache = _run(1)
    its = _replay_identity(aco, tours, cache, 4)
    assert _is_permutation(its["actions"], 20)
    again, tours2, _ = _run(1)
    assert torch.equal(_cpu(again.last_iterations)["actions"], its["actions"]) and torch.equal(tours2, tours)
    assert torch.equal(again.pheromone, aco.pheromone)
    other, _, _ = _run(2)
    assert not torch.equal(_cpu(other.last_iterations)["actions"], its["actions"])


def test_class_surface_with_local_search():
    aco, tours, cache = _run(1, n_iterations=3, use_local_search=True)
    its = _replay_identity(aco, tours, cache, 3)
    assert bool((its["reward"] >= its["sampled_reward"]).all()) and bool((its["reward"] > its["sampled_reward"]).any())
    assert _is_permutation(its["actions"], 20)


def test_custom_start_nodes_are_called_once_per_iteration():
    from rl4co_amd import AntSystem

    env, td, heu = _problem()
    calls = []

    def pick(td_, env_, num_starts):
        calls.append(num_starts)
        return torch.full((num_starts * 6,), len(calls), dtype=torch.int64, device="cuda")

    aco = AntSystem(heu, n_ants=8)
    aco.run(td, env, 3, dict(KW, select_start_nodes_fn=pick, temperature=0.5))
    assert calls == [8, 8, 8]
    firsts = aco.last_iterations["actions"][:, :, 0].cpu()
    assert all(bool((firsts[i] == i + 1).all()) for i in range(3))


# ---- 6. error bits -----------------------------------------------------------------------------------------------------------
def _bits_run(phe, heu, locs, starts, ants):
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = _K().aco_tsp(phe, n_ants=ants, iterations=2, log_heuristic=heu.cuda(), locs=locs.cuda(), start_nodes=starts.cuda(),
                       philox_seed=99, record_iterations=True, err=err)
    return int(err.item()), _cpu(out)


def test_error_bits_on_inputs_the_kernel_survives():
    b, n, ants = 3, 10, 4
    locs, heu, phe0 = _instance(b, n, 55)
    starts = torch.arange(ants * b).remainder(n).repeat(2, 1)
    bits, out = _bits_run(phe0.cuda(), heu, locs, starts, ants)
    assert bits == 0 and _is_permutation(out["iter_actions"], n)

    dead = heu.clone()
    dead[:, 3, :] = float("-inf")  # whoever stands on node 3 sees no finite logit
    bits, out = _bits_run(phe0.cuda(), dead, locs, starts, ants)
    assert bits & _lib.EBIT_INFEASIBLE and not bits & _lib.EBIT_TOUR_INDEX and _is_permutation(out["iter_actions"], n)

    phe = phe0.clone()
    phe[:, 2, :] = float("nan")
    bits, out = _bits_run(phe.cuda(), heu, locs, torch.full_like(starts, 2), ants)
    assert bits & _lib.EBIT_NAN_LOGIT and _is_permutation(out["iter_actions"], n)

    bad = starts.clone()
    bad[1, 2 * b + 1] = n  # ant 2 of instance 1, second iteration
    phe = phe0.cuda()
    bits, out = _bits_run(phe, heu, locs, bad, ants)
    assert bits == _lib.EBIT_TOUR_INDEX
    assert torch.equal(phe.cpu()[1], phe0[1]) and not torch.equal(phe.cpu()[0], phe0[0]) and not torch.equal(phe.cpu()[2], phe0[2])
    with pytest.raises(AssertionError, match="tour index out of range"):
        _K().aco_tsp(phe0.cuda(), n_ants=ants, iterations=2, log_heuristic=heu.cuda(), locs=locs.cuda(), start_nodes=bad.cuda())
