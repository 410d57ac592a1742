"""Ant System search for OP and PCTSP on the MI355X (csrc/aco_prize.hip, rl4co_amd/aco.py): the kernel under the recorded
noise against the records of the reference's own AntSystem and the CPU restatement (tests/aco_prize_ref.py), seeded shapes
against the restatement bit for bit (lane-slot boundaries, both sides of the LDS tier, ant counts that are no multiple of the
wave count, any number of workgroups, the environments' edge regimes), the masks against the project's own environments on
the device, the index refusal and the class surface."""
from functools import lru_cache

import pytest
import torch

from rl4co_amd import _lib
from tests import aco_prize_ref as R

pytestmark = pytest.mark.gpu
SAMPLE, UPDATE = _lib.ACO_SAMPLE, _lib.ACO_UPDATE
RECORDS = [(env, case) for env in R.ENVS for case in R.CASES]


def _K():
    from rl4co_amd import kernels as K

    return K


def _cpu(out):
    return {k: v.cpu() for k, v in out.items()}


def _dev(data):
    return {k: v.cuda() for k, v in data.items() if k != "locs"}


def _launch(env, phe, heu, data, n_ants, **kw):
    return _cpu(_K().aco_prize(phe, env=env, n_ants=n_ants, log_heuristic=heu.cuda(), locs=data["locs"].cuda(), **_dev(data), **kw))


# ---- 1. the records ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,case", RECORDS)
def test_kernel_under_the_recorded_noise_equals_record_and_restatement(env, case):
    rec = R.record(env, case)
    c, ants, b, iters, alpha, beta, decay, phe0, _ = R.CASES[case]
    n = c + 1
    w, data, q = R.width(n), R.record_data(env, rec), float(rec["Q"])
    kw = dict(alpha=alpha, beta=beta, decay=decay, Q=q)
    phe_f = rec["pheromone0"].cuda()
    fused = _launch(env, phe_f, rec["log_heuristic"], data, ants, iterations=iters, ln_noise=rec["ln_noise"].cuda(),
                    record_iterations=True, **kw)
    phe_s, carried = rec["pheromone0"].cuda(), {}
    state = R.fresh_state(rec["pheromone0"])
    for i in range(iters):
        before = state["pheromone"].clone()
        one = _launch(env, phe_s, rec["log_heuristic"], data, ants, ln_noise=rec["ln_noise"][i : i + 1].contiguous().cuda(),
                      has_best=bool(carried), iteration_base=i, **carried, **kw)
        carried = {k: one[k].cuda() for k in ("final_reward", "final_actions", "final_iteration")}
        # all iterations in one launch == the same iterations launched one at a time
        assert torch.equal(one["actions"], fused["iter_actions"][i]) and torch.equal(one["reward"], fused["iter_reward"][i])
        assert torch.equal(one["lengths"], fused["iter_lengths"][i])
        assert torch.equal(one["final_reward"], fused["final_reward_cache"][i])
        # the reference's record
        ref_actions = rec[f"actions_{i}"]
        t_i = ref_actions.shape[1]
        assert torch.equal(one["actions"], R.pad(ref_actions, w)) and torch.equal(one["lengths"], rec["lengths"][i])
        dev = float((one["logps"][:, :t_i] - rec[f"logps_{i}"]).abs().max())
        dev64 = float((one["logps"][:, :t_i].double() - rec[f"logps64_{i}"]).abs().max())
        off = float(R.ulps(one["reward"], rec["reward"][i], R.reward_scale(env, data, one["actions"])).max())
        print(f"{env} {case} iteration {i}: log-prob deviation {dev:.3e} / float64 {dev64:.3e} (STEP_TOL {R.STEP_TOL:.3e}), "
              f"reward off the record by {off} ulps (bound {R.REWARD_ULPS})")
        assert dev <= R.STEP_TOL and dev64 <= R.STEP_TOL and bool((one["logps"][:, t_i:] == 0).all())
        assert off <= R.REWARD_ULPS
        # the restatement: everything bit for bit but the log-probs
        actions, lengths, logps, _, _ = R.sample(env, before, rec["log_heuristic"], data, rec["ln_noise"][i], alpha, beta)
        assert torch.equal(one["actions"], actions) and torch.equal(one["lengths"], lengths)
        assert float((one["logps"] - logps).abs().max()) <= R.STEP_TOL
        assert torch.equal(one["reward"], R.reward_w(env, data, actions))
        R.update(state, actions, one["reward"], decay, q, keep=int(lengths.max()))
        assert torch.equal(phe_s.cpu(), state["pheromone"]) and torch.equal(one["final_reward"], state["final_reward"])
        assert torch.equal(one["final_actions"], R.final_matrix(state["final_actions"], w))
        if float(rec["reward_ulps"]) == 0:  # the W-wide reward is the reference's: so are its pheromone and its record
            assert torch.equal(phe_s.cpu(), rec["pheromone"][i]) and torch.equal(one["final_reward"], rec["final_reward"][i])
            assert all(torch.equal(x, y) for x, y in zip(state["final_actions"], R.record_finals(rec, i)))
    assert torch.equal(phe_f, phe_s) and torch.equal(fused["final_actions"], one["final_actions"])
    assert torch.equal(fused["final_iteration"], one["final_iteration"]) and torch.equal(fused["final_reward"], one["final_reward"])


@pytest.mark.parametrize("env,case", RECORDS)
def test_update_alone_on_the_reference_rows_equals_the_record(env, case):
    rec = R.record(env, case)
    c, ants, b, iters, alpha, beta, decay, phe0, _ = R.CASES[case]
    phe, carried, finals = rec["pheromone0"].cuda(), {}, [None] * b
    for i in range(iters):
        acts = rec[f"actions_{i}"]
        if carried:
            carried["final_actions"] = torch.zeros((b, acts.shape[1]), dtype=torch.int64, device="cuda")
        out = _K().aco_prize(phe, env=env, n_ants=ants, phases=UPDATE, actions=acts.cuda(), reward=rec["reward"][i].cuda(),
                             decay=decay, Q=float(rec["Q"]), iteration_base=i, has_best=bool(carried), **carried)
        carried = {k: out[k] for k in ("final_reward", "final_actions", "final_iteration")}
        assert torch.equal(phe.cpu(), rec["pheromone"][i]) and torch.equal(out["final_reward"].cpu(), rec["final_reward"][i])
        for k in (out["final_iteration"].cpu() == i).nonzero()[:, 0].tolist():
            finals[k] = out["final_actions"][k].cpu()
        assert all(torch.equal(x, y) for x, y in zip(finals, R.record_finals(rec, i)))


# ---- 2. seeded shapes against the restatement, bit for bit under given noise ------------------------------------------------------
@lru_cache(maxsize=None)
def _problem(env, b, n, seed, budget=1.2, prize_scale=None):
    data = R.random_data(env, b, n, seed, budget=budget, prize_scale=prize_scale)
    g = torch.Generator().manual_seed(seed + 1)
    return data, R.heuristic(data["locs"]), 0.5 + torch.rand(b, n, n, generator=g)


def _against_restatement(env, b, n, ants, seed, iters=2, budget=1.2, prize_scale=None, data=None, **kw):
    """``iters`` iterations in one launch under given noise against the restatement, bit for bit. Where every ant of an
    instance earns the same reward (one ant; N = 2) the reward map is 0 / 0 as in the reference and the pheromone turns NaN:
    the comparison then ends with that iteration (NaN for NaN), and the next one must raise RL4CO_EBIT_NAN_LOGIT."""
    prob = _problem(env, b, n, seed, budget, prize_scale)
    data = prob[0] if data is None else data
    _, heu, phe0 = prob
    rows, w = ants * b, R.width(n)
    noise = R.ln_exp1((iters, w, rows, n), seed=seed + 2)
    phe = phe0.cuda()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = _launch(env, phe, heu, data, ants, iterations=iters, ln_noise=noise.cuda(), record_iterations=True, alpha=0.9,
                  beta=1.3, decay=0.9, Q=0.5, err=err, **kw)
    state = R.fresh_state(phe0)
    for i in range(iters):
        actions, lengths, logps, _, _ = R.sample(env, state["pheromone"], heu, data, noise[i], 0.9, 1.3)
        assert torch.equal(out["iter_actions"][i], actions) and torch.equal(out["iter_lengths"][i], lengths)
        assert torch.equal(out["iter_reward"][i], R.reward_w(env, data, actions))
        R.update(state, actions, out["iter_reward"][i], 0.9, 0.5)
        assert torch.equal(out["final_reward_cache"][i], state["final_reward"])
        if i + 1 < iters and bool(torch.isnan(state["pheromone"]).any()):
            assert int(err.item()) & _lib.EBIT_NAN_LOGIT and not int(err.item()) & _lib.EBIT_TOUR_INDEX
            assert bool((out["iter_lengths"] >= 1).all()) and bool((out["iter_lengths"] <= w).all())
            return out
    assert int(err.item()) == 0
    assert float((out["logps"] - logps).abs().max()) <= R.STEP_TOL
    got = phe.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(state["pheromone"]))
    assert torch.equal(got.nan_to_num(7.0), state["pheromone"].nan_to_num(7.0))
    assert torch.equal(out["final_reward"], state["final_reward"])
    assert torch.equal(out["final_actions"], torch.stack(state["final_actions"], 0))
    return out


@pytest.mark.parametrize("env", R.ENVS)
@pytest.mark.parametrize("n,ants", [(2, 4), (3, 4), (64, 4), (65, 4), (129, 4), (21, 1), (21, 5), (21, 9)])
def test_shapes_follow_the_restatement(env, n, ants):
    _against_restatement(env, 3, n, ants, 100 + n + ants, budget=1.2 if n < 64 else 2.5)


@pytest.mark.parametrize("env", R.ENVS)
@pytest.mark.parametrize("side", [0, 1], ids=["lds", "global"])
def test_both_sides_of_the_lds_tier_follow_the_restatement(env, side):
    n = _K().aco_prize_lds_nodes(env) + side
    assert n == 141 + side
    _against_restatement(env, 2, n, 4, 900 + side, budget=2.5)


@pytest.mark.parametrize("env", R.ENVS)
def test_any_number_of_workgroups_gives_the_same_outputs(env):
    outs = [_against_restatement(env, 67, 12, 5, 67, budget=2.0, n_workgroups=g) for g in (1, 5, 0)]
    for other in outs[1:]:
        assert all(torch.equal(outs[0][k], other[k]) for k in outs[0])


def test_op_budget_so_tight_that_only_the_depot_is_feasible():
    out = _against_restatement("op", 3, 12, 5, 31, budget=0.0)
    assert bool((out["iter_actions"] == 0).all()) and bool((out["iter_lengths"] == 2).all())
    assert bool((out["iter_reward"] == 0).all()) and bool((out["logps"] == 0).all())


def test_pctsp_total_prize_below_one_visits_every_customer():
    n = 12
    out = _against_restatement("pctsp", 3, n, 5, 32, prize_scale=0.5)
    assert float(_problem("pctsp", 3, n, 32, 1.2, 0.5)[0]["prize"].sum(-1).max()) < 1
    assert bool((out["iter_lengths"] == n).all())
    assert all(sorted(row.tolist()) == list(range(n)) for row in out["iter_actions"].reshape(-1, n))


def test_pctsp_one_customer_holding_the_whole_prize():
    n = 12
    data = {k: v.clone() for k, v in _problem("pctsp", 3, n, 33, 1.2, 0.5)[0].items()}
    data["prize"][:, 4] = 1.25
    out = _against_restatement("pctsp", 3, n, 5, 33, prize_scale=0.5, data=data)
    rows = out["iter_actions"].reshape(-1, n)
    lengths = out["iter_lengths"].reshape(-1)
    assert bool((lengths < n).any())  # some row returns early, and only after customer 4
    for row, length in zip(rows.tolist(), lengths.tolist()):
        assert length == n or 4 in row[: length - 1]


# ---- 3. mask parity with the project's environments ----------------------------------------------------------------------------
def _tile(td, ants):
    """Ant-major rows: row j * B + b is a copy of instance b."""
    rows = ants * td.batch_size[0]
    return type(td)({k: v.repeat(ants, *([1] * (v.dim() - 1))).contiguous() for k, v in td.items()}, batch_size=[rows])


@pytest.mark.parametrize("name", ["op", "pctsp", "spctsp"])
def test_rows_replayed_through_the_environment_on_the_device(name):
    from rl4co_amd.envs import get_env

    n, ants, b = 30, 8, 8
    env = get_env(name, generator_params=dict(num_loc=n - 1))
    torch.manual_seed(5)
    td0 = env.reset(batch_size=[b])
    heu = R.heuristic(td0["locs"].cpu())
    phe = 0.5 + torch.rand(b, n, n, generator=torch.Generator().manual_seed(6))
    if name == "op":
        data = dict(prize=td0["prize"], max_length=td0["max_length"])
    else:
        data = dict(prize=td0["real_prize"], penalty=td0["penalty"])
        # expected_prize is the deterministic prize: SPCTSPEnv's reset put the stochastic one into real_prize
        assert torch.equal(td0["real_prize"][:, 1:], td0["expected_prize"]) == (name == "pctsp")
    out = _K().aco_prize(phe.cuda(), env=name, n_ants=ants, phases=SAMPLE, log_heuristic=heu.cuda(), locs=td0["locs"],
                         philox_seed=77, temperature=0.8, **data)
    actions, lengths, logps = out["actions"], out["lengths"].cpu(), out["logps"].cpu()
    rows = ants * b
    lg64 = (torch.log(phe.double()) + heu.double()) / torch.tensor(0.8, dtype=torch.float32).double()
    td = _tile(td0, ants)
    was_done = torch.zeros(rows, dtype=torch.bool)
    cur = torch.zeros(rows, dtype=torch.int64)
    worst = 0.0
    ar = torch.arange(rows)
    for t in range(n):
        feasible = env.get_action_mask(td).bool().cpu()
        a = actions[:, t].cpu()
        live = ~was_done
        assert bool(feasible[ar, a][live].all()), t  # every chosen action is feasible under get_action_mask
        assert bool((a[~live] == 0).all()) and bool((logps[~live, t] == 0).all())
        lp = torch.log_softmax(lg64[ar % b, cur].masked_fill(~feasible, float("-inf")), -1)[ar, a]
        worst = max(worst, float((logps[:, t].double() - lp)[live].abs().max()) if bool(live.any()) else 0.0)
        assert torch.equal(lengths > t, live)  # done falls where the row's length says
        td.set("action", actions[:, t].contiguous())
        td = env.step(td)["next"]
        was_done = was_done | td["done"].reshape(-1).bool().cpu()
        cur = a
    assert bool(was_done.all())
    print(f"{name}: largest deviation of a per-step log-prob from the float64 log-softmax over the env's mask {worst:.3e}")
    assert worst <= R.STEP_TOL
    env.check_solution_validity(_tile(td0, ants), actions)


# ---- 4. index refusal ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", R.ENVS)
def test_out_of_range_rows_set_the_error_word_and_leave_the_instance_untouched(env):
    b, n, ants = 3, 10, 4
    data, heu, phe0 = _problem(env, b, n, 55)
    good = _launch(env, phe0.cuda(), heu, data, ants, phases=SAMPLE, philox_seed=9)["actions"]
    for bad_node in (-1, n):
        forced = good.clone()
        forced[2 * b + 1, 3] = bad_node  # ant 2 of instance 1
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = _launch(env, phe0.cuda(), heu, data, ants, phases=SAMPLE, forced_actions=forced.cuda(), err=err)
        assert int(err.item()) == _lib.EBIT_TOUR_INDEX
        rows_of_1 = torch.arange(ants) * b + 1
        assert bool((out["lengths"][rows_of_1] == 0).all()) and bool((out["actions"][rows_of_1] == 0).all())
        keep = torch.ones(ants * b, dtype=torch.bool)
        keep[rows_of_1] = False
        assert torch.equal(out["actions"][keep], good[keep]) and bool((out["lengths"][keep] >= 2).all())
        phe = phe0.cuda()
        err.zero_()
        reward = torch.rand(ants * b, generator=torch.Generator().manual_seed(1))
        _K().aco_prize(phe, env=env, n_ants=ants, phases=UPDATE, actions=forced.cuda(), reward=reward.cuda(), err=err)
        assert int(err.item()) == _lib.EBIT_TOUR_INDEX
        assert torch.equal(phe.cpu()[1], phe0[1]) and not torch.equal(phe.cpu()[0], phe0[0]) and not torch.equal(phe.cpu()[2], phe0[2])
    with pytest.raises(AssertionError, match="tour index out of range"):
        _K().aco_prize(phe0.cuda(), env=env, n_ants=ants, phases=UPDATE, actions=forced.cuda(), reward=reward.cuda())


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------
MS = dict(multisample=True, num_samples=8, select_best=False)


@lru_cache(maxsize=None)
def _class_problem(name):
    from rl4co_amd.envs import get_env

    env = get_env(name, generator_params=dict(num_loc=20))
    torch.manual_seed(11)
    td = env.reset(batch_size=[6])
    return env, td, R.heuristic(td["locs"].cpu()).cuda()


def _run(name, seed):
    from rl4co_amd import AntSystem

    env, td, heu = _class_problem(name)
    aco = AntSystem(heu, n_ants=8)
    torch.manual_seed(seed)
    tours, cache = aco.run(td, env, 3, MS)
    return aco, tours, cache


@pytest.mark.parametrize("name", R.ENVS)
def test_class_surface_run(name):
    env, td, heu = _class_problem(name)
    aco, tours, cache = _run(name, 1)
    env.check_solution_validity(td, tours)
    data = {"locs": td["locs"].cpu(), "prize": td["prize" if name == "op" else "real_prize"].cpu()}
    data["max_length" if name == "op" else "penalty"] = td["max_length" if name == "op" else "penalty"].cpu()
    got = env.get_reward(td, tours).cpu()
    off = float(R.ulps(cache[2].cpu(), got, R.reward_scale(name, data, tours.cpu())).max())
    print(f"{name}: final reward off env.get_reward on the returned actions by {off} ulps (bound {R.REWARD_ULPS})")
    assert off <= R.REWARD_ULPS
    assert sorted(cache) == [0, 1, 2] and all(bool((cache[i] >= cache[i - 1]).all()) for i in (1, 2))
    assert torch.equal(aco.final_reward, cache[2]) and len(aco.final_actions) == 6 and tours.shape[1] <= 21
    its = _cpu(aco.last_iterations)
    state = R.fresh_state(torch.ones(6, 21, 21))
    for i in range(3):  # the reference's rule replayed from last_iterations: the ragged record
        assert torch.equal(its["reward"][i], R.reward_w(name, data, its["actions"][i]))
        R.update(state, its["actions"][i], its["reward"][i], aco.decay, aco.Q, keep=int(its["lengths"][i].max()))
        assert torch.equal(cache[i].cpu(), state["final_reward"])
    assert torch.equal(aco.pheromone.cpu(), state["pheromone"])
    assert all(torch.equal(x.cpu(), y) for x, y in zip(aco.final_actions, state["final_actions"]))
    assert torch.equal(tours.cpu(), R.final_matrix(state["final_actions"]))
    again, tours2, _ = _run(name, 1)
    assert torch.equal(tours2, tours) and torch.equal(again.pheromone, aco.pheromone)
    assert torch.equal(_cpu(again.last_iterations)["actions"], its["actions"])
    other, _, _ = _run(name, 2)
    assert not torch.equal(_cpu(other.last_iterations)["actions"], its["actions"])
    actions, reward = aco._one_step(td, env, MS)  # a further iteration on the same record
    assert actions.shape == (48, 21) and bool((aco.final_reward >= cache[2]).all())
    assert torch.equal(env.get_reward(td, actions), reward)


def test_deepaco_policy_reaches_the_kernel_for_op():
    from rl4co_amd import DeepACOPolicy

    env, td, heu = _class_problem("op")

    class Fixed(torch.nn.Module):
        def forward(self, td_):
            return heu.clone(), None

    policy = DeepACOPolicy(encoder=Fixed(), env_name="op", n_ants=8, n_iterations=3)
    torch.manual_seed(1)
    out = policy(td, env, phase="test")
    assert sorted(out) == ["actions", "reward", "reward_000", "reward_001", "reward_002"]
    assert torch.equal(out["reward"], out["reward_002"]) and bool((out["reward_002"] >= out["reward_000"]).all())
    env.check_solution_validity(td, out["actions"])
    assert policy.last_aco.last_iterations["lengths"].shape == (3, 48)  # (the prize kernel's read-back)
    _, tours, cache = _run("op", 1)
    assert torch.equal(out["actions"], tours) and torch.equal(out["reward"], cache[2])
