"""Ant System search for CVRP on the MI355X (csrc/aco_cvrp.hip, rl4co_amd/aco.py): the update against the records of the
reference's own AntSystem with its CVRPEnv and the CPU restatement (tests/aco_cvrp_ref.py) with no tolerance, the per-step
log-probs within STEP_TOL (4 x the reference's own fp32-vs-float64 deviation), mask and selection rule exactly in both entry
modes and three capacity regimes, the W-wide reward bit for bit (also on rows of 520 and more segments, where the summation
cascade has more than one level), fused against split launches on both sides of the LDS tier,
the class surface with the reference's ragged final_actions, and the sticky error bits on inputs the kernel has to survive."""
from functools import lru_cache

import pytest
import torch

from rl4co_amd import _lib
from tests import aco_cvrp_ref as R

pytestmark = pytest.mark.gpu
SAMPLE, UPDATE = _lib.ACO_SAMPLE, _lib.ACO_UPDATE
NEG_INF = float("-inf")


def _K():
    from rl4co_amd import kernels as K

    return K


def _env(c, **kw):
    from rl4co_amd.envs import CVRPEnv

    return CVRPEnv(generator_params=dict(num_loc=c), **kw)


def _cpu(out):
    return {k: v.cpu() for k, v in out.items()}


def _td(locs, demand, cap):
    return {"locs": locs.cuda(), "demand": demand.cuda(), "vehicle_capacity": cap.reshape(-1, 1).cuda()}


def _valid(locs, demand, cap, actions):
    _env(demand.shape[1]).check_solution_validity(_td(locs, demand, cap), actions.cuda().contiguous())


# ---- 1. the update against the records -----------------------------------------------------------------------------------------
def _update_launch(phe, actions, reward, state, decay, q, n_ants, base=0):
    """One UPDATE-only launch on device copies; ``state``: None or the last launch's output (its record carried over in a
    fresh [B, T] buffer: the rows the launch replaces are the ones whose final_iteration becomes ``base``)."""
    kw = {}
    if state is not None:
        kw = dict(final_reward=state["final_reward"], final_iteration=state["final_iteration"], has_best=True,
                  final_actions=torch.zeros((phe.shape[0], actions.shape[1]), dtype=torch.int64, device="cuda"))
    return _K().aco_cvrp(phe, n_ants=n_ants, phases=UPDATE, actions=actions.cuda(), reward=reward.cuda(), decay=decay, Q=q,
                         iteration_base=base, **kw)


@pytest.mark.parametrize("case", list(R.CASES))
def test_update_equals_the_record(case):
    rec = R.record(case)
    c, ants, b, iters, alpha, beta, decay, phe0, _, mode = R.CASES[case]
    phe = rec["pheromone0"].cuda()
    state, finals = None, [None] * b
    for i in range(iters):
        state = _update_launch(phe, rec[f"actions_{i}"], rec["reward"][i], state, decay, float(rec["Q"]), ants, base=i)
        assert torch.equal(phe.cpu(), rec["pheromone"][i])
        assert torch.equal(state["final_reward"].cpu(), rec["final_reward"][i])
        assert torch.equal(state["final_reward_cache"].cpu()[0], rec["final_reward"][i])
        for k in (state["final_iteration"].cpu() == i).nonzero()[:, 0].tolist():
            finals[k] = state["final_actions"][k].cpu()
        assert i > 0 or all(f is not None for f in finals)
        assert all(torch.equal(x, y) for x, y in zip(finals, R.record_finals(rec, i)))


def _random_rows(g, b, ants, c, t):
    """Valid CVRP rows of width t: a customer permutation with one mid-tour depot return, zero-padded."""
    rows = []
    for _ in range(ants * b):
        perm = (torch.randperm(c, generator=g) + 1).tolist()
        cut = int(torch.randint(1, c, (1,), generator=g))
        row = perm[:cut] + [0] + perm[cut:]
        rows.append(row + [0] * (t - len(row)))
    return torch.tensor(rows)


def _assert_update_equals_restatement(acts, reward, b, n, ants, decay, q, fill):
    want = R.update(R.fresh_state(torch.full((b, n, n), fill)), acts, reward, decay, q)
    phe = torch.full((b, n, n), fill).cuda()
    out = _update_launch(phe, acts, reward, None, decay, q, ants)
    got = phe.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want["pheromone"]))
    assert torch.equal(got.nan_to_num(7.0), want["pheromone"].nan_to_num(7.0))
    assert torch.equal(out["final_reward"].cpu(), want["final_reward"])
    assert torch.equal(out["final_actions"].cpu(), torch.stack(want["final_actions"], 0))
    assert bool((out["final_iteration"] == 0).all())
    return got, out


def test_update_with_equal_rewards_is_nan_where_the_restatement_is():
    g = torch.Generator().manual_seed(5)
    b, c, ants, t = 3, 8, 4, 12
    acts = _random_rows(g, b, ants, c, t)
    reward = -torch.rand(ants * b, generator=g) - 1
    reward.view(ants, b)[:, 1] = -2.5  # instance 1: every ant the same reward -> 0 / 0
    got, out = _assert_update_equals_restatement(acts, reward, b, c + 1, ants, 0.9, 0.3, 1.5)
    assert bool(torch.isnan(got[1]).any()) and not bool(torch.isnan(got[0]).any()) and not bool(torch.isnan(got[2]).any())
    assert float(got[1, 0, 0]) == float(R.f32(1.5) * R.f32(0.9))  # delta[0][0] = 0 whatever the trailing zeros carry
    assert torch.equal(out["final_actions"].cpu()[1], acts[1])  # the lowest ant (ant 0, row 0 * B + 1) on equal rewards


def test_update_with_one_ant():
    g = torch.Generator().manual_seed(6)
    b, c, t = 2, 6, 9
    acts = _random_rows(g, b, 1, c, t)
    reward = -torch.rand(b, generator=g) - 1
    got, _ = _assert_update_equals_restatement(acts, reward, b, c + 1, 1, 0.95, 1.0, 1.0)
    assert bool(torch.isnan(got).any())


# ---- 2. evaluate against the records -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
def test_evaluate_equals_the_record(case):
    rec = R.record(case)
    c, ants, b, iters, alpha, beta, decay, phe0, _, mode = R.CASES[case]
    w = R.width(c + 1)
    td = _td(rec["locs"], rec["demand"], rec["vehicle_capacity"])
    before = rec["pheromone0"]
    for i in range(iters):
        phe = before.cuda()
        trimmed = rec[f"actions_{i}"]
        t_i = trimmed.shape[1]
        forced = R.pad(trimmed, w)
        starts = rec["start_nodes"][i][None].contiguous().cuda() if mode == "multistart" else None
        out = _K().aco_cvrp(phe, n_ants=ants, phases=SAMPLE, log_heuristic=rec["log_heuristic"].cuda(), locs=td["locs"],
                            demand=td["demand"], vehicle_capacity=td["vehicle_capacity"], start_nodes=starts, alpha=alpha,
                            beta=beta, forced_actions=forced.cuda())
        logps = out["logps"].cpu()
        dev = float((logps[:, :t_i] - rec[f"logps_{i}"]).abs().max())
        print(f"{case} iteration {i}: largest per-step log-prob deviation {dev:.3e} (STEP_TOL {R.STEP_TOL:.3e})")
        assert dev <= R.STEP_TOL and bool((logps[:, t_i:] == 0).all())
        assert torch.equal(out["lengths"].cpu(), rec["lengths"][i])
        assert torch.equal(out["actions"].cpu(), forced) and torch.equal(phe.cpu(), before)
        env_reward = _env(c).get_reward(td, out["actions"])
        assert torch.equal(out["reward"], env_reward) and torch.equal(out["reward"].cpu(), R.reward_w(rec["locs"], forced))
        before = rec["pheromone"][i]


# ---- 3. the selection rule and the mask ----------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _instance(b, n, seed):
    g = torch.Generator().manual_seed(seed)
    locs = torch.rand(b, n, 2, generator=g)
    return locs, R.heuristic(locs), 0.5 + torch.rand(b, n, n, generator=g)


@lru_cache(maxsize=None)
def _regimes(n):
    """Three instances, one per capacity regime: never binding (with the noise of _depot_last every row is C + 1 long), about
    three customers per route, every demand 0.6 of the capacity (a return between any two customers: every row is
    2 C - 1 = W long)."""
    locs, heu, phe0 = _instance(3, n, 300 + n)
    c = n - 1
    g = torch.Generator().manual_seed(n)
    demand = torch.stack((torch.full((c,), 0.5 / c), 0.25 + 0.1 * torch.rand(c, generator=g), torch.full((c,), 0.6)))
    return locs, heu, phe0, demand, torch.ones(3)


def _depot_last(noise, b):
    """Parity-mode noise under which the rows of instance 0 take the depot only when nothing else is feasible: its key is
    lp - 40 there (the log-probs themselves stay what they are)."""
    noise[:, :, 0::b, 0] = 40.0
    return noise


@pytest.mark.parametrize("mode", ["multisample", "multistart"])
@pytest.mark.parametrize("temperature", [1.0, 0.7])
@pytest.mark.parametrize("n,ants", [(6, 5), (6, 8), (65, 8), (66, 5)])
def test_selection_and_mask_follow_the_restatement(n, ants, temperature, mode):
    b, c, w = 3, n - 1, R.width(n)
    rows = ants * b
    locs, heu, phe0, demand, cap = _regimes(n)
    g = torch.Generator().manual_seed(n * ants)
    starts = torch.randint(1, n, (1, rows), generator=g) if mode == "multistart" else None
    noise = _depot_last(R.ln_exp1((1, w, rows, n), seed=n + ants), b)
    out = _cpu(_K().aco_cvrp(phe0.cuda(), n_ants=ants, log_heuristic=heu.cuda(), locs=locs.cuda(), demand=demand.cuda(),
                             vehicle_capacity=cap.cuda(), start_nodes=None if starts is None else starts.cuda(),
                             ln_noise=noise.cuda(), temperature=temperature, alpha=0.9, beta=1.3, all_logps=True))
    acts, lengths, logps, full = out["actions"], out["lengths"], out["logps"], out["all_logps"]
    _valid(locs, demand, cap, acts)
    ref_acts, ref_len, ref_logps, ref_full, masks = R.sample(phe0, heu, demand, cap, None if starts is None else starts[0], None,
                                                             0.9, 1.3, temperature, forced=acts)
    assert torch.equal(lengths, ref_len) and torch.equal(acts, ref_acts)
    by_instance = lengths.view(ants, b)
    assert bool((by_instance[:, 0] == c + 1).all()) and bool((by_instance[:, 2] == 2 * c - 1).all())
    for r in range(1, rows, b):  # about three customers per route: at least one mid-tour return, not one after every customer
        returns = int((acts[r, : int(lengths[r]) - 1] == 0).sum())
        assert 1 <= returns < c - 1 and int(lengths[r]) == c + returns
    t0 = 1 if mode == "multistart" else 0
    for r in range(rows):
        length = int(lengths[r])
        assert bool((acts[r, length:] == 0).all()) and bool((logps[r, length:] == 0).all()) and bool((full[r, length:] == 0).all())
        if t0:
            assert int(acts[r, 0]) == int(starts[0, r]) and float(logps[r, 0]) == 0 and bool((full[r, 0] == 0).all())
        for t in range(t0, length):
            infeasible = masks[r, t]
            assert torch.equal(full[r, t] == NEG_INF, infeasible), (r, t)
            assert R.select(full[r, t], noise[0, t, r], infeasible) == int(acts[r, t]), (r, t)
            assert float(logps[r, t]) == float(full[r, t, acts[r, t]])
    finite = torch.isfinite(ref_full)
    assert torch.equal(finite, torch.isfinite(full))
    dev = float((full[finite] - ref_full[finite]).abs().max())
    print(f"n {n} ants {ants} T {temperature} {mode}: largest log-prob deviation from the restatement {dev:.3e}")
    assert dev <= R.STEP_TOL and float((logps - ref_logps).abs().max()) <= R.STEP_TOL
    assert torch.equal(out["reward"], R.reward_w(locs, acts))


# ---- 4. fused equals split -------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _problem(b, n, seed):
    locs, heu, phe0 = _instance(b, n, seed)
    g = torch.Generator().manual_seed(seed + 1)
    return locs, heu, phe0, 0.1 + 0.3 * torch.rand(b, n - 1, generator=g), torch.ones(b)


def _fused(phe, n_ants, iters, prob, starts, noise, **kw):
    locs, heu, _, demand, cap = prob
    return _cpu(_K().aco_cvrp(phe, n_ants=n_ants, iterations=iters, log_heuristic=heu.cuda(), locs=locs.cuda(),
                              demand=demand.cuda(), vehicle_capacity=cap.cuda(), ln_noise=noise.cuda(),
                              start_nodes=None if starts is None else starts.cuda(), record_iterations=True, **kw))


@pytest.mark.parametrize("mode", ["multisample", "multistart"])
def test_fused_equals_split_launches(mode):
    b, n, ants, iters = 3, 21, 6, 3
    rows, w = ants * b, R.width(n)
    prob = _problem(b, n, 77)
    locs, heu, phe0, demand, cap = prob
    g = torch.Generator().manual_seed(3)
    starts = torch.randint(1, n, (iters, rows), generator=g) if mode == "multistart" else None
    noise = R.ln_exp1((iters, w, rows, n), seed=4)
    kw = dict(alpha=1.1, beta=0.8, decay=0.9, Q=0.25)
    phe_f = phe0.cuda()
    fused = _fused(phe_f, ants, iters, prob, starts, noise, **kw)
    phe_s = phe0.cuda()
    state = {}
    for i in range(iters):
        s = _K().aco_cvrp(phe_s, n_ants=ants, phases=SAMPLE, log_heuristic=heu.cuda(), locs=locs.cuda(), demand=demand.cuda(),
                          vehicle_capacity=cap.cuda(), ln_noise=noise[i : i + 1].contiguous().cuda(),
                          start_nodes=None if starts is None else starts[i : i + 1].contiguous().cuda(), **kw)
        assert torch.equal(s["actions"].cpu(), fused["iter_actions"][i]) and torch.equal(s["reward"].cpu(), fused["iter_reward"][i])
        assert torch.equal(s["lengths"].cpu(), fused["iter_lengths"][i])
        u = _K().aco_cvrp(phe_s, n_ants=ants, phases=UPDATE, actions=s["actions"], reward=s["reward"], has_best=bool(state),
                          iteration_base=i, **state, **kw)
        state = dict(final_reward=u["final_reward"], final_actions=u["final_actions"], final_iteration=u["final_iteration"])
        assert torch.equal(u["final_reward"].cpu(), fused["final_reward_cache"][i])
    _valid(locs, demand, cap, fused["iter_actions"].reshape(-1, w))
    assert torch.equal(phe_s, phe_f) and not torch.equal(phe_f.cpu(), phe0)
    assert torch.equal(state["final_reward"].cpu(), fused["final_reward"])
    assert torch.equal(state["final_actions"].cpu(), fused["final_actions"])
    assert torch.equal(state["final_iteration"].cpu(), fused["final_iteration"]) and bool((fused["final_iteration"] >= 0).all())
    assert torch.equal(fused["actions"], fused["iter_actions"][-1]) and torch.equal(fused["reward"], fused["iter_reward"][-1])
    assert torch.equal(fused["lengths"], fused["iter_lengths"][-1])


# ---- 5. both sides of the LDS tier ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [0, 1], ids=["lds", "global"])
def test_both_sides_of_the_lds_tier_follow_the_restatement(side):
    n = _K().aco_cvrp_lds_nodes() + side
    b, ants, iters = 2, 4, 2
    rows, w = ants * b, R.width(n)
    prob = _problem(b, n, 900 + side)
    locs, heu, phe0, demand, cap = prob
    noise = R.ln_exp1((iters, w, rows, n), seed=10 + side)
    phe = phe0.cuda()
    out = _fused(phe, ants, iters, prob, None, noise, decay=0.9, Q=0.5)
    _valid(locs, demand, cap, out["iter_actions"].reshape(-1, w))
    assert torch.equal(out["iter_reward"].reshape(-1), R.reward_w(locs, out["iter_actions"].reshape(-1, w)))
    state = R.fresh_state(phe0)
    for i in range(iters):
        R.update(state, out["iter_actions"][i], out["iter_reward"][i], 0.9, 0.5)
        assert torch.equal(state["final_reward"], out["final_reward_cache"][i])
    assert torch.equal(phe.cpu(), state["pheromone"])
    assert torch.equal(out["final_reward"], state["final_reward"])
    assert torch.equal(out["final_actions"], torch.stack(state["final_actions"], 0))


LONG_ROW_SEED = 2730  # (the locs of the two cases below; the N = 273 case failed on the kernel's earlier private reward)


@pytest.mark.parametrize("n", [273, 261])
def test_reward_of_long_rows_equals_tour_length(n):
    """Rows of 520 and more segments (W + 1 >= 520, n >= 261: more than 64 eight-lane vectors, so SumKernel's cascade has
    non-zero higher levels AND a non-zero tail when it folds): every demand is 0.6 of the capacity, so every customer forces
    a depot return, every row is 2 C - 1 = W long and ends at a customer. Global-memory tier, one ant per wave, in-kernel
    Philox. The kernel's reward is bit for bit rl4co_tour_length_f32 with the depot prepended and ATen's own sum."""
    c, w = n - 1, R.width(n)
    locs, heu, phe0 = _instance(1, n, LONG_ROW_SEED + n)
    assert n > _K().aco_cvrp_lds_nodes() and (w + 1) // 8 > 64
    out = _K().aco_cvrp(phe0.cuda(), n_ants=4, phases=SAMPLE, log_heuristic=heu.cuda(), locs=locs.cuda(),
                        demand=torch.full((1, c), 0.6).cuda(), vehicle_capacity=torch.ones(1).cuda(), philox_seed=n)
    assert out["actions"].shape == (4, w) and bool((out["lengths"] == w).all())
    _valid(locs, torch.full((1, c), 0.6), torch.ones(1), out["actions"])
    want = _K().tour_length(locs.cuda(), out["actions"], prepend_depot=True, negate=True)
    host = R.reward_w(locs, out["actions"].cpu())
    bits = out["reward"].cpu().view(torch.int32)  # (same sign, same binade: a difference of the words is one in ulps)
    print(f"n {n}: reward {out['reward'].tolist()}, off tour_length by {(bits - want.cpu().view(torch.int32)).tolist()} ulps, "
          f"off ATen on the CPU by {(bits - host.view(torch.int32)).tolist()} ulps")
    assert torch.equal(out["reward"], want)
    assert torch.equal(out["reward"].cpu(), host)


# ---- 6. the class surface --------------------------------------------------------------------------------------------------
MS = dict(multisample=True, num_samples=8, select_best=False)


@lru_cache(maxsize=None)
def _class_problem():
    torch.manual_seed(11)
    env = _env(20)
    td = env.reset(batch_size=[6])
    return env, td, R.heuristic(td["locs"].cpu()).cuda()


def _run(seed, kw, n_iterations=4):
    from rl4co_amd import AntSystem

    env, td, heu = _class_problem()
    aco = AntSystem(heu, n_ants=8)
    torch.manual_seed(seed)
    tours, cache = aco.run(td, env, n_iterations, kw)
    return aco, tours, cache


def _replay(aco, tours, cache, n_iterations):
    """The reference's rule replayed from last_iterations: entry b of final_actions has the width of the iteration that last
    replaced it (that iteration's longest row), the matrix is zero-padded to the longest entry."""
    env, td, heu = _class_problem()
    w = R.width(21)
    its = _cpu(aco.last_iterations)
    assert its["actions"].shape == (n_iterations, 48, w) and sorted(cache) == list(range(n_iterations))
    state = R.fresh_state(torch.ones(6, 21, 21))
    for i in range(n_iterations):
        R.update(state, its["actions"][i], its["reward"][i], aco.decay, aco.Q, keep=int(its["lengths"][i].max()))
        assert torch.equal(cache[i].cpu(), state["final_reward"])
        assert torch.equal(env.get_reward(td, R.final_matrix(state["final_actions"], w).cuda()).cpu(), cache[i].cpu())
        assert i == 0 or bool((cache[i] >= cache[i - 1]).all())
    assert torch.equal(aco.pheromone.cpu(), state["pheromone"]) and torch.equal(aco.final_reward.cpu(), state["final_reward"])
    assert len(aco.final_actions) == 6
    assert all(torch.equal(x.cpu(), y) for x, y in zip(aco.final_actions, state["final_actions"]))
    want = R.final_matrix(state["final_actions"])
    assert tours.shape == want.shape and torch.equal(tours.cpu(), want) and tours.shape[1] <= w
    env.check_solution_validity(td, tours)
    env.check_solution_validity(td, aco.last_iterations["actions"].reshape(-1, w))
    return its


def test_class_surface_run():
    aco, tours, cache = _run(1, MS)
    its = _replay(aco, tours, cache, 4)
    again, tours2, _ = _run(1, MS)
    assert torch.equal(_cpu(again.last_iterations)["actions"], its["actions"]) and torch.equal(tours2, tours)
    assert torch.equal(again.pheromone, aco.pheromone)
    other, _, _ = _run(2, MS)
    assert not torch.equal(_cpu(other.last_iterations)["actions"], its["actions"])
    env, td, heu = _class_problem()
    actions, reward = aco._one_step(td, env, MS)  # a further iteration on the same record
    assert actions.shape == (48, R.width(21)) and bool((aco.final_reward >= cache[3]).all())
    assert torch.equal(env.get_reward(td, actions), reward)


def test_class_surface_multistart_with_custom_start_nodes():
    calls = []

    def pick(td_, env_, num_starts):
        calls.append(num_starts)
        return torch.full((num_starts * 6,), len(calls), dtype=torch.int64, device="cuda")

    kw = dict(multistart=True, num_starts=8, select_best=False, select_start_nodes_fn=pick, temperature=0.5)
    aco, tours, cache = _run(1, kw, n_iterations=3)
    assert calls == [8, 8, 8]
    its = _replay(aco, tours, cache, 3)
    assert all(bool((its["actions"][i][:, 0] == i + 1).all()) for i in range(3))
    default, tours, cache = _run(1, dict(multistart=True, num_starts=8, select_best=False), n_iterations=2)
    firsts = _replay(default, tours, cache, 2)["actions"][0][:, 0]
    env, td, heu = _class_problem()
    assert torch.equal(firsts, env.select_start_nodes(td, num_starts=8).cpu())


# ---- 7. error bits -----------------------------------------------------------------------------------------------------------
def _bits_run(phe, heu, prob, starts, ants, demand=None):
    locs, _, _, dem, cap = prob
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = _K().aco_cvrp(phe, n_ants=ants, iterations=2, log_heuristic=heu.cuda(), locs=locs.cuda(),
                        demand=(dem if demand is None else demand).cuda(), vehicle_capacity=cap.cuda(),
                        start_nodes=None if starts is None else starts.cuda(), philox_seed=99, record_iterations=True, err=err)
    return int(err.item()), _cpu(out)


def test_error_bits_on_inputs_the_kernel_survives():
    b, n, ants = 3, 10, 4
    w = R.width(n)
    prob = _problem(b, n, 55)
    locs, heu, phe0, demand, cap = prob
    starts = (torch.arange(ants * b).remainder(n - 1) + 1).repeat(2, 1)
    bits, out = _bits_run(phe0.cuda(), heu, prob, starts, ants)
    assert bits == 0
    _valid(locs, demand, cap, out["iter_actions"].reshape(-1, w))

    dead = heu.clone()
    dead[:, 3, :] = NEG_INF  # whoever stands on node 3 sees no finite logit
    bits, out = _bits_run(phe0.cuda(), dead, prob, None, ants)
    assert bits & _lib.EBIT_INFEASIBLE and not bits & _lib.EBIT_TOUR_INDEX
    _valid(locs, demand, cap, out["iter_actions"].reshape(-1, w))

    phe = phe0.clone()
    phe[:, 2, :] = float("nan")
    bits, out = _bits_run(phe.cuda(), heu, prob, torch.full_like(starts, 2), ants)
    assert bits & _lib.EBIT_NAN_LOGIT
    _valid(locs, demand, cap, out["iter_actions"].reshape(-1, w))

    for bad_node in (0, n):
        bad = starts.clone()
        bad[1, 2 * b + 1] = bad_node  # ant 2 of instance 1, second iteration
        phe = phe0.cuda()
        bits, out = _bits_run(phe, heu, prob, bad, ants)
        assert bits == _lib.EBIT_TOUR_INDEX
        assert torch.equal(phe.cpu()[1], phe0[1]) and not torch.equal(phe.cpu()[0], phe0[0]) and not torch.equal(phe.cpu()[2], phe0[2])
    with pytest.raises(AssertionError, match="tour index out of range"):
        _K().aco_cvrp(phe0.cuda(), n_ants=ants, iterations=2, log_heuristic=heu.cuda(), locs=locs.cuda(), demand=demand.cuda(),
                      vehicle_capacity=cap.cuda(), start_nodes=bad.cuda())

    heavy = demand.clone()
    heavy[1, 4] = 1.5  # customer 5 of instance 1 can never be served
    bits, out = _bits_run(phe0.cuda(), heu, prob, None, ants, demand=heavy)
    assert bits == _lib.EBIT_INFEASIBLE
    lengths = out["iter_lengths"].view(2, ants, b)
    assert bool((lengths <= w).all()) and bool((lengths[:, :, 1] == w).all()) and bool((lengths[:, :, 0] < w).all())
    assert not bool((out["iter_actions"].view(2, ants, b, w)[:, :, 1] == 5).any())
    others = out["iter_actions"].view(2, ants, b, w)[:, :, 0].reshape(-1, w)
    _env(n - 1).check_solution_validity(_td(locs[:1], demand[:1], cap[:1]), others.cuda().contiguous())
