"""DeepACO's training path on the depot graphs on the MI355X (csrc/aco_depot_grad.hip, rl4co_amd/aco.py,
NonAutoregressivePolicy): the backward kernel against the records of the reference's own train path and against the float64
restatement (tests/aco_depot_grad_ref.py) on the shapes where it can go wrong, the mask against the forward's own, its exact
properties (run-to-run, split-to-split and tier-to-tier identical bits, zeros where nothing contributes), the refusals, the
autograd seam, the policy and a short training run.

Tolerance. Against a record and against the float64 restatement alike the gradient stays within GRAD_TOL = 4 x the
reference's own fp32-vs-float64 deviation of its autograd gradient (tests/aco_depot_grad_ref.py), for every shape here."""
from functools import lru_cache

import pytest
import torch

from rl4co_amd import _lib
from tests import aco_depot_grad_ref as G

pytestmark = pytest.mark.gpu
NEG_INF = float("-inf")


def _K():
    from rl4co_amd import kernels as K

    return K


def _grad(env, heat, acts, grad_ll, data, **kw):
    steps = kw.pop("grad_steps", None)
    return _K().aco_depot_logp_grad(heat.cuda(), acts.cuda(), grad_ll.cuda(), env=env, grad_steps=None if steps is None else steps.cuda(),
                                    **G.kernel_data(env, data), **kw)


# ---- 1. against the records -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,case", [(env, case) for env in G.ENVS for case in G.CASES])
def test_forward_and_gradient_against_the_record(env, case):
    from rl4co_amd.aco import heatmap_rollout

    rec = G.record(env, case)
    c, ants, b, temperature, _ = G.CASES[case]
    data = G.record_data(env, rec)
    heat = rec["heatmap"].cuda().requires_grad_(True)
    out = heatmap_rollout(heat, rec["locs"].cuda(), n_ants=ants, actions=rec["actions"].cuda(), temperature=temperature,
                          env_name=env, td=G.as_td(env, data))
    assert torch.equal(out["actions"].cpu(), rec["actions"]) and torch.equal(out["lengths"].cpu(), rec["lengths"])
    assert torch.equal(out["reward"].cpu(), G.reward_w(env, data, rec["actions"]))  # get_reward on the W-wide row, bit for bit
    reward_ulps = float(G.PZ.ulps(out["reward"].cpu(), rec["reward"], G.reward_scale(env, data, rec["actions"])).max())
    step_err = float((out["logps"].detach().cpu() - rec["logps"]).abs().max())
    (out["log_likelihood"] * rec["grad_ll"].cuda()).sum().backward()
    grad_err = float((heat.grad.cpu().double() - rec["grad64"]).abs().max())
    print(f"{env}_{case}: log-prob error {step_err:.3e} (tol {G.STEP_TOL[env]:.3e}), gradient error {grad_err:.3e} (floor "
          f"{float(rec['grad_noise_floor']):.3e}, tol {G.GRAD_TOL:.3e}), reward {reward_ulps} ulps (bound {G.REWARD_ULPS[env]})")
    assert step_err <= G.STEP_TOL[env]
    assert reward_ulps <= G.REWARD_ULPS[env]
    assert grad_err <= G.GRAD_TOL
    direct = _grad(env, rec["heatmap"], rec["actions"], rec["grad_ll"], data, temperature=temperature)
    assert torch.equal(direct, heat.grad)


# ---- 2. against the float64 restatement ---------------------------------------------------------------------------------------
# name -> (envs, N, ants, B, temperature, grad_steps given, variant, binding keywords)
ALL = G.ENVS
RANDOM = {
    "n3_a1_b1": (ALL, 3, 1, 1, 1.0, False, None, {}),
    "n6_a5_b3": (ALL, 6, 5, 3, 1.0, False, None, {}),
    "n64_a5_b3": (ALL, 64, 5, 3, 1.0, False, None, {}),
    "n65_a33_b1": (ALL, 65, 33, 1, 1.0, False, None, {}),
    "n130_a5_b3": (ALL, 130, 5, 3, 1.0, False, None, {}),
    "n20_a7_b3_t05": (ALL, 20, 7, 3, 0.5, False, None, {}),
    "n65_a2_b3_steps": (ALL, 65, 2, 3, 1.0, True, None, {}),
    "n20_a5_b3_scratch_forced": (ALL, 20, 5, 3, 1.0, True, None, dict(table_in_scratch=True, row_split=2)),
    # 8 320 entries: the table leaves LDS (8 192). Few ants on purpose: the tolerance is an absolute one recorded at 20 ants,
    # and a depot-row word is a sum of ants x routes terms — at 127 ants x 65 nodes torch's own fp32 autograd is 4.7e-6 off
    # the float64 gradient on the CPU, above GRAD_TOL, so that shape measures the number format, not the kernel. For the same
    # reason CVRP's demands are U{1..9} / 200 here (about 13 routes per ant, not 87: with those torch's fp32 is 2.2e-6 off).
    "n520_a16_b1_scratch": (ALL, 520, 16, 1, 1.0, False, "long_routes", {}),
    "n1024_a2_b1": (ALL, 1024, 2, 1, 1.0, False, None, {}),          # CVRP: W = 2045
    "n64_a5_b3_neg_inf": (ALL, 64, 5, 3, 1.0, False, "neg_inf", {}),
    "n12_a5_b3_big_demands": (("cvrp",), 12, 5, 3, 1.0, False, "big_demands", {}),
    "n40_a5_b3_tiny_demands": (("cvrp",), 40, 5, 3, 1.0, False, "tiny_demands", {}),
    "n30_a6_b3_multistart": (("cvrp",), 30, 6, 3, 0.8, True, "multistart", {}),
    "n20_a5_b3_depot_first": (("op",), 20, 5, 3, 1.0, False, "depot_first", {}),
    "n20_a5_b3_small_prizes": (("pctsp",), 20, 5, 3, 1.0, False, "small_prizes", {}),
}
RANDOM_CASES = [(env, name) for name, spec in RANDOM.items() for env in spec[0]]


@lru_cache(maxsize=None)
def _random_case(env, name):
    _, n, ants, b, temperature, with_steps, variant, _ = RANDOM[name]
    seed = 2000 + 10 * sorted(RANDOM).index(name) + G.ENVS.index(env)
    gen = torch.Generator().manual_seed(seed)
    rows, w = ants * b, G.width(env, n)
    extra = {"prize_scale": 0.5} if variant == "small_prizes" else {"demand_scale": 200.0} if (variant, env) == ("long_routes", "cvrp") else {}
    data = G.random_data(env, b, n, seed, **extra)
    if variant == "big_demands":
        data["demand"] = 0.5 + 0.4 * torch.rand(b, n - 1, generator=gen) + 0.05
    if variant == "tiny_demands":
        data["demand"] = torch.full((b, n - 1), 1e-3)
    heat = 2.0 * torch.randn(b, n, n, generator=gen)
    starts = torch.randint(1, n, (rows,), generator=gen) if variant == "multistart" else None
    acts, lengths, _, _, masks = G.sample_rows(env, heat, data, ants, seed + 1, start_nodes=starts, temperature=temperature)
    if variant == "depot_first":  # ant 0 of every instance takes the depot at step 0 (and again at step 1: the row is done)
        acts = acts.clone()
        acts[:b] = 0
        acts, lengths, _, _, masks = G.replay(env, heat, data, actions=acts)
        assert bool((lengths[:b] == 2).all()) and bool((lengths[b:] >= 2).all())
    if variant == "big_demands":  # one route per customer: the longest row, C departures from the depot
        assert bool((lengths == w).all()) and bool(((acts[:, 1::2] == 0).all())) and bool((acts[:, 0::2] != 0).all())
    if variant == "tiny_demands":  # a single route: the sampled customers in their order, then the depot (a sampled ant may
        single = torch.zeros_like(acts)  # return early of its own accord)
        for r in range(rows):
            single[r, : n - 1] = acts[r][acts[r] != 0]
        acts, lengths, _, _, masks = G.replay(env, heat, data, actions=single, temperature=temperature)
        assert bool((lengths == n).all()) and bool((acts[:, : n - 1] != 0).all())
    if variant == "small_prizes":  # the total prize stays below 1: every customer must be visited
        assert float(data["prize"].sum(-1).max()) < 1.0 and bool((lengths == n).all())
    if variant == "multistart":
        assert torch.equal(acts[:, 0], starts)
    grad_ll = torch.rand(rows, generator=gen) * 2 - 1
    steps = (torch.rand(rows, w, generator=gen) * 2 - 1) if with_steps else None
    if variant == "neg_inf":  # -inf on a third of the entries, never on an edge an ant takes: every step stays feasible
        drop = torch.rand(b, n, n, generator=gen) < 1 / 3
        inst = (torch.arange(rows) % b)[:, None].expand(rows, w)
        cur = torch.cat((torch.zeros(rows, 1, dtype=torch.int64), acts[:, :-1]), 1)
        live = torch.arange(w)[None, :] < lengths[:, None]
        drop[inst[live], cur[live], acts[live]] = False
        heat = heat.masked_fill(drop, NEG_INF)
    _, want = G.logp_grad(heat, acts, lengths, masks, grad_ll, grad_steps=steps, start_nodes=starts, temperature=temperature)
    assert bool(torch.isfinite(want).all())
    return heat, acts, lengths, masks, grad_ll, steps, data, want, starts is not None


@pytest.mark.parametrize("env,name", RANDOM_CASES)
def test_gradient_against_the_float64_restatement(env, name):
    _, n, ants, b, temperature, _, _, kw = RANDOM[name]
    heat, acts, lengths, _, grad_ll, steps, data, want, multistart = _random_case(env, name)
    K = _K()
    if name.endswith("_scratch"):
        assert ants * n > K.aco_depot_grad_lds_entries()
    got = _grad(env, heat, acts, grad_ll, data, grad_steps=steps, temperature=temperature, multistart=multistart, **kw)
    assert got.shape == (b, n, n) and bool(torch.isfinite(got).all())
    err = float((got.cpu().double() - want).abs().max())
    print(f"{env} {name}: gradient error {err:.3e} (tol {G.GRAD_TOL:.3e}, largest entry {float(want.abs().max()):.3e}, "
          f"lengths {int(lengths.min())}..{int(lengths.max())})")
    assert err <= G.GRAD_TOL
    assert float(got.diagonal(dim1=1, dim2=2)[:, 1:].abs().max()) == 0.0  # a customer's row never holds the customer itself


# ---- 3. the mask is the forward's ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["cvrp", "op"])
def test_the_mask_is_the_forward_s(env):
    K = _K()
    n, b = 24, 4
    gen = torch.Generator().manual_seed(77)
    if env == "cvrp":  # demands in eighths, capacity 1: demand + used == capacity occurs, and is feasible
        data = {"locs": torch.rand(b, n, 2, generator=gen), "demand": torch.randint(1, 5, (b, n - 1), generator=gen).float() / 8,
                "vehicle_capacity": torch.ones(b)}
    else:  # a tight budget: the length test masks unvisited customers
        data = G.random_data("op", b, n, 78, budget=1.6)
    heat = torch.randn(b, n, n, generator=gen)
    acts, lengths, _, _, masks = G.sample_rows(env, heat, data, 1, 79)
    if env == "cvrp":
        ties = 0
        for r in range(b):
            state = G.CV.fresh(n)
            for t in range(int(lengths[r])):
                ties += int(((data["demand"][r] + state["used"] == data["vehicle_capacity"][r]) & ~state["visited"][1:]).sum())
                G.CV.step_state(state, int(acts[r, t]), data["demand"][r])
        assert ties > 0
    else:
        live = torch.arange(n)[None, :] < lengths[:, None]
        visited = torch.zeros(b, n, dtype=torch.bool)
        by_length = 0
        for t in range(n):
            by_length += int((masks[:, t, 1:] & ~visited[:, 1:] & live[:, t, None] & (acts[:, :t] != 0).all(1)[:, None]).sum())
            visited[torch.arange(b), acts[:, t]] = True
        assert by_length > 0
    common = dict(n_ants=1, phases=_lib.ACO_SAMPLE, log_heuristic=heat.cuda(), locs=data["locs"].cuda(),
                  forced_actions=acts.cuda(), all_logps=True)
    if env == "cvrp":
        fwd = K.aco_cvrp(torch.ones_like(heat).cuda(), demand=data["demand"].cuda(), vehicle_capacity=data["vehicle_capacity"].cuda(), **common)
    else:
        fwd = K.aco_prize(torch.ones_like(heat).cuda(), env="op", prize=data["prize"].cuda(), max_length=data["max_length"].cuda(), **common)
    assert torch.equal(fwd["lengths"].cpu(), lengths)
    all_logps = fwd["all_logps"].cpu()
    assert torch.equal(torch.isinf(all_logps) & (torch.arange(all_logps.shape[1])[None, :, None] < lengths[:, None, None]), masks)
    grad = _grad(env, heat, acts, torch.ones(b), data).cpu()
    rows_checked = 0
    for r in range(b):
        for t in range(1, int(lengths[r])):
            i = int(acts[r, t - 1])
            if i == 0:
                continue
            finite = torch.isfinite(all_logps[r, t])
            assert float(grad[r, i][~finite].abs().max()) == 0.0
            if int(finite.sum()) > 1:
                assert bool((grad[r, i][finite] != 0).all()), (r, t)
                rows_checked += 1
    assert rows_checked > b


# ---- 4. exact properties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", G.ENVS)
def test_launches_splits_and_tiers_give_identical_bits(env):
    for name in ("n20_a7_b3_t05", "n130_a5_b3", "n65_a2_b3_steps"):
        _, n, _, _, temperature, _, _, _ = RANDOM[name]
        heat, acts, lengths, _, grad_ll, steps, data, _, _ = _random_case(env, name)
        kw = dict(grad_steps=steps, temperature=temperature)
        one = _grad(env, heat, acts, grad_ll, data, row_split=1, **kw)
        assert torch.equal(one, _grad(env, heat, acts, grad_ll, data, row_split=1, **kw))
        for split in (2, 5, n):
            assert torch.equal(one, _grad(env, heat, acts, grad_ll, data, row_split=split, **kw)), (name, split)
        assert torch.equal(one, _grad(env, heat, acts, grad_ll, data, **kw))  # the binding's own choice
        assert torch.equal(one, _grad(env, heat, acts, grad_ll, data, table_in_scratch=True, row_split=3, **kw))
        # padded steps after a row's length contribute nothing
        w = acts.shape[1]
        pad = torch.arange(w)[None, :] >= lengths[:, None]
        assert bool(pad.any())
        noisy = (torch.zeros(acts.shape) if steps is None else steps.clone()).masked_fill(pad, 99.0)
        base = one if steps is not None else _grad(env, heat, acts, grad_ll, data, grad_steps=torch.zeros(acts.shape), temperature=temperature)
        assert torch.equal(base, _grad(env, heat, acts, grad_ll, data, grad_steps=noisy, temperature=temperature))


@pytest.mark.parametrize("env", G.ENVS)
def test_zeros_where_nothing_contributes(env):
    heat, acts, lengths, _, grad_ll, _, data, _, _ = _random_case(env, "n64_a5_b3")
    n, ants, b = 64, 5, 3
    g = grad_ll.clone()
    g.view(ants, b)[:, 1] = 0.0  # instance 1: every upstream gradient is zero
    got = _grad(env, heat, acts, g, data).cpu()
    assert float(got[1].abs().max()) == 0.0 and float(got[0].abs().max()) > 0 and float(got[2].abs().max()) > 0
    # one ant: the rows it never leaves are zero, the depot's column 0 is zero where the depot is infeasible at step 0
    one = _grad(env, heat[:1], acts[:1], torch.ones(1), {k: v[:1] for k, v in data.items()}).cpu()[0]
    left = set(acts[0, : int(lengths[0]) - 1].tolist()) | {0}
    never = [i for i in range(n) if i not in left]
    if never:
        assert float(one[never].abs().max()) == 0.0
    assert float(one[0].abs().max()) > 0
    if env != "op":
        assert float(one[0, 0]) == 0.0
    # visited customers get nothing: the row of a_t is zero on a_0 .. a_t (customers)
    for t in range(min(int(lengths[0]) - 1, 6)):
        i = int(acts[0, t])
        if i != 0:
            seen = [a for a in acts[0, : t + 1].tolist() if a != 0]
            assert float(one[i, seen].abs().max()) == 0.0


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["above_range", "negative", "repeated", "infeasible"])
@pytest.mark.parametrize("env", G.ENVS)
def test_bad_rows_are_refused_per_instance(env, kind):
    K = _K()
    heat, acts, lengths, _, grad_ll, _, data, _, _ = _random_case(env, "n64_a5_b3")
    n, ants, b = 64, 5, 3
    clean = _grad(env, heat, acts, grad_ll, data)
    bad = acts.clone()
    row = next(j * b + 1 for j in range(ants) if int(lengths[j * b + 1]) >= 4)  # an ant of instance 1 with three customers
    assert 0 not in bad[row, :3].tolist()
    if kind == "repeated":
        bad[row, 2] = bad[row, 0]
        bit, message = _lib.EBIT_INVALID_TOUR, "Invalid tour"
    elif kind == "infeasible":  # the depot at step 0: CVRP and PCTSP mask it; OP allows it but no customer after it
        bad[row, 1:] = acts[row, :-1]
        bad[row, 0] = 0
        bit, message = _lib.EBIT_INFEASIBLE, "infeasible"
    else:
        bad[row, 2] = n if kind == "above_range" else -1
        bit, message = _lib.EBIT_TOUR_INDEX, "tour index out of range"
    for kw in ({}, dict(row_split=4), dict(table_in_scratch=True)):
        err = K.new_error_word("cuda")
        got = _grad(env, heat, bad, grad_ll, data, err=err, **kw)
        bits = int(err.item())
        assert bits & bit and not bits & ~(_lib.EBIT_INVALID_TOUR | _lib.EBIT_INFEASIBLE | _lib.EBIT_TOUR_INDEX), (bits, kw)
        assert bits == bit  # (after a repeated customer the row's later verdicts are consequences and are not added)
        assert float(got[1].abs().max()) == 0.0
        assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])
    with pytest.raises(AssertionError, match=message):
        _grad(env, heat, bad, grad_ll, data)


def test_a_row_not_done_and_a_depot_start_are_refused():
    K = _K()
    heat, acts, lengths, _, grad_ll, _, data, _, _ = _random_case("cvrp", "n12_a5_b3_big_demands")
    bad = acts.clone()
    bad[0] = torch.cat((acts[0, :2], acts[0, 4:], torch.zeros(2, dtype=torch.int64)))  # a customer left out: never done
    err = K.new_error_word("cuda")
    got = _grad("cvrp", heat, bad, grad_ll, data, err=err)
    assert int(err.item()) == _lib.EBIT_INFEASIBLE and float(got[0].abs().max()) == 0.0 and float(got[1].abs().max()) > 0
    heat, acts, _, _, grad_ll, steps, data, _, _ = _random_case("cvrp", "n30_a6_b3_multistart")
    bad = acts.clone()
    bad[1, 0] = 0  # a multistart start is a customer
    err = K.new_error_word("cuda")
    got = _grad("cvrp", heat, bad, grad_ll, data, multistart=True, err=err)
    assert int(err.item()) & _lib.EBIT_TOUR_INDEX and float(got[1].abs().max()) == 0.0 and float(got[0].abs().max()) > 0


# ---- 6. the autograd seam ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", G.ENVS + ("spctsp",))
def test_heatmap_rollout_backward_is_the_kernel(env):
    from rl4co_amd.aco import heatmap_rollout

    K = _K()
    base = "pctsp" if env == "spctsp" else env
    gen = torch.Generator().manual_seed(21)
    b, n, ants = 3, 21, 7
    data = G.random_data(base, b, n, 31)
    td, locs = G.as_td(base, data), data["locs"].cuda()
    w = G.width(base, n)
    heat = (2.0 * torch.randn(b, n, n, generator=gen)).cuda().requires_grad_(True)
    wl = (torch.rand(ants * b, generator=gen) * 2 - 1).cuda()
    kw = dict(n_ants=ants, temperature=0.8, env_name=env, td=td)
    out = heatmap_rollout(heat, locs, seed=7, **kw)
    acts, lengths = out["actions"], out["lengths"]
    assert acts.shape == (ants * b, w) and out["logps"].shape == (ants * b, w) and lengths.shape == (ants * b,)
    pad = torch.arange(w, device="cuda")[None, :] >= lengths[:, None]
    assert float(acts[pad].abs().max()) == 0 and float(out["logps"][pad].abs().max()) == 0
    assert torch.equal(out["log_likelihood"], out["logps"].sum(1))
    assert torch.equal(out["reward"].cpu(), G.reward_w(base, data, acts.cpu()))
    assert out["log_likelihood"].requires_grad and out["logps"].requires_grad
    assert not acts.requires_grad and not out["reward"].requires_grad and not lengths.requires_grad
    (wl * out["log_likelihood"]).sum().backward()
    kd = G.kernel_data(base, data)
    assert torch.equal(heat.grad, K.aco_depot_logp_grad(heat.detach(), acts, wl, env=env, temperature=0.8, **kd))
    assert float(heat.grad.abs().max()) > 0
    # the per-step log-probs carry the gradient too, and both add up
    ws = (torch.rand(ants * b, w, generator=gen) * 2 - 1).cuda()
    again = heatmap_rollout(heat, locs, seed=7, **kw)
    assert torch.equal(again["actions"], acts) and torch.equal(again["logps"], out["logps"])  # the same seed, the same ants
    (grad,) = torch.autograd.grad((ws * again["logps"]).sum() + (wl * again["log_likelihood"]).sum(), heat)
    assert torch.equal(grad, K.aco_depot_logp_grad(heat.detach(), acts, wl, env=env, grad_steps=ws, temperature=0.8, **kd))
    assert not torch.equal(heatmap_rollout(heat, locs, seed=8, **kw)["actions"], acts)
    # evaluation of given rows: the forced forward reports the sampled run's log-probs
    forced = heatmap_rollout(heat, locs, actions=acts, **kw)
    assert torch.equal(forced["logps"], out["logps"]) and torch.equal(forced["reward"], out["reward"])
    # no double backward
    fresh = heatmap_rollout(heat, locs, seed=7, **kw)
    with pytest.raises(RuntimeError, match="no double backward"):
        torch.autograd.grad(fresh["log_likelihood"].sum(), heat, create_graph=True)
    # a heatmap that needs no gradient: nothing is recorded, nothing is saved
    plain = heatmap_rollout(heat.detach(), locs, seed=7, **kw)
    assert plain["log_likelihood"].grad_fn is None and not plain["log_likelihood"].requires_grad
    assert plain["logps"].grad_fn is None and torch.equal(plain["logps"], out["logps"])
    # the caller's error word: nothing raises, the bit is there; without it the forward raises
    err = K.new_error_word("cuda")
    spoiled = acts.clone()
    spoiled[0, 0] = n
    heatmap_rollout(heat.detach(), locs, actions=spoiled, err=err, **kw)
    assert int(err.item()) == _lib.EBIT_TOUR_INDEX
    with pytest.raises(AssertionError, match="tour index out of range"):
        heatmap_rollout(heat.detach(), locs, actions=spoiled, **kw)
    if env == "cvrp":  # multistart: the given customers are column 0 with log-prob 0, and the backward knows
        starts = torch.randint(1, n, (ants * b,), generator=gen).cuda()
        heat.grad = None
        ms = heatmap_rollout(heat, locs, start_nodes=starts, seed=9, **kw)
        assert torch.equal(ms["actions"][:, 0], starts) and float(ms["logps"][:, 0].abs().max()) == 0
        (wl * ms["log_likelihood"]).sum().backward()
        assert torch.equal(heat.grad, K.aco_depot_logp_grad(heat.detach(), ms["actions"], wl, env=env, multistart=True,
                                                            temperature=0.8, **kd))
    else:
        with pytest.raises(NotImplementedError, match="start_nodes"):
            heatmap_rollout(heat, locs, start_nodes=torch.ones(ants * b, dtype=torch.int64).cuda(), **kw)


def test_a_refusal_of_the_backward_launch_comes_through_the_seam():
    """The forward accepts its rows; the saved rows are then spoiled behind autograd's back, so only the backward launch can
    refuse: with ``err=None`` it reads its own word and raises, with the caller's word it sets the bit there."""
    from rl4co_amd.aco import heatmap_rollout

    b, n, ants = 2, 9, 3
    data = G.random_data("pctsp", b, n, 41, prize_scale=0.5)  # every customer is visited: the rows are n long
    kw = dict(n_ants=ants, env_name="pctsp", td=G.as_td("pctsp", data), seed=1)
    heat = torch.randn(b, n, n, generator=torch.Generator().manual_seed(22)).cuda().requires_grad_(True)
    out = heatmap_rollout(heat, data["locs"].cuda(), **kw)
    out["actions"].data[1 * b + 1, 4] = out["actions"].data[1 * b + 1, 2]  # ant 1 of instance 1 repeats a customer
    with pytest.raises(AssertionError, match="Invalid tour"):
        out["log_likelihood"].sum().backward()
    err = _K().new_error_word("cuda")
    out = heatmap_rollout(heat, data["locs"].cuda(), err=err, **kw)
    assert int(err.item()) == 0
    out["actions"].data[1 * b + 1, 4] = out["actions"].data[1 * b + 1, 2]
    heat.grad = None
    out["log_likelihood"].sum().backward()
    assert int(err.item()) == _lib.EBIT_INVALID_TOUR
    assert float(heat.grad[1].abs().max()) == 0.0 and float(heat.grad[0].abs().max()) > 0


# ---- 7. the policy ------------------------------------------------------------------------------------------------------------------
class _PairwiseEncoder(torch.nn.Module):
    """A tiny differentiable encoder: an MLP on pairwise distances -> (heatmap [B, N, N], None)."""

    def __init__(self):
        super().__init__()
        self.mlp = torch.nn.Sequential(torch.nn.Linear(1, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1))

    def forward(self, td):
        locs = td["locs"]
        d = (locs[:, :, None, :] - locs[:, None, :, :]).norm(p=2, dim=-1)
        return self.mlp(d[..., None])[..., 0], None


@pytest.mark.parametrize("env", ["tsp", "cvrp", "cvrp_multistart", "op", "pctsp", "spctsp"])
def test_policy_trains_an_encoder_through_the_kernels(env):
    from rl4co_amd import NonAutoregressivePolicy
    from rl4co_amd.aco import deepaco_loss

    torch.manual_seed(3)
    b, n, ants = 4, 20, 6
    name, multistart = env.split("_")[0], env in ("tsp", "cvrp_multistart")
    base = "pctsp" if name == "spctsp" else name
    if name == "tsp":
        td = {"locs": torch.rand(b, n, 2, generator=torch.Generator().manual_seed(5)).cuda()}
        td["action_mask"] = torch.ones(b, n, dtype=torch.bool, device="cuda")
        w = n
    else:
        td = G.as_td(base, G.random_data(base, b, n, 51))
        td["action_mask"] = torch.ones(b, n, dtype=torch.bool, device="cuda")
        td["action_mask"][:, 0] = False
        w = G.width(base, n)
    enc = _PairwiseEncoder().cuda()
    pol = NonAutoregressivePolicy(enc, env_name=name, temperature=0.9,
                                  train_decode_type="multistart_sampling" if multistart else "sampling")
    pick = lambda td_, env_, k: torch.multinomial(td_["action_mask"].float(), k, replacement=True).t().reshape(-1)  # noqa: E731
    kw = dict(num_starts=ants, select_start_nodes_fn=pick) if multistart else dict(multisample=True, num_samples=ants)
    out = pol(td, name, phase="train", return_hidden=True, **kw)
    assert sorted(out) == ["actions", "hidden", "log_likelihood", "reward"]
    assert out["reward"].shape == out["log_likelihood"].shape == (ants * b,) and out["actions"].shape == (ants * b, w)
    assert out["hidden"].shape == (b, n, n) and out["hidden"].requires_grad and out["log_likelihood"].requires_grad
    assert bool((out["log_likelihood"] < 0).all())
    loss = deepaco_loss({"reward": out["reward"].view(ants, b).t(), "log_likelihood": out["log_likelihood"].view(ants, b).t()})
    loss.backward()
    for p in enc.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    plain = pol(td, name, phase="train", return_actions=False, **kw)
    assert sorted(plain) == ["log_likelihood", "reward"]
    for bad, match in ((dict(phase="val"), "DeepACOPolicy"), (dict(top_k=5), "top_k"), (dict(return_entropy=True), "return_entropy")):
        with pytest.raises(NotImplementedError, match=match):
            pol(td, name, **{"phase": "train", **kw, **bad})


# ---- 8. learning ----------------------------------------------------------------------------------------------------------------------
def test_a_free_heatmap_learns_shorter_routes():
    """CVRP, B = 8, 20 customers, 16 ants, Adam(lr = 0.2), 40 steps: on the CPU restatement (the fp32 sampling restatement,
    autograd through tests/aco_depot_grad_ref.py rollout_logps) the mean reward rises from -12.3 .. -12.5 over the first five
    steps to -8.9 .. -9.0 over the last five (three seeds); here only the direction."""
    from rl4co_amd.aco import deepaco_loss, heatmap_rollout

    torch.manual_seed(0)
    b, n, ants = 8, 21, 16
    data = G.random_data("cvrp", b, n, 9)
    td, locs = G.as_td("cvrp", data), data["locs"].cuda()
    heat = torch.nn.Parameter(torch.zeros(b, n, n, device="cuda"))
    opt = torch.optim.Adam([heat], lr=0.2)
    rewards = []
    for step in range(40):
        out = heatmap_rollout(heat, locs, n_ants=ants, seed=100 + step, env_name="cvrp", td=td)
        loss = deepaco_loss({"reward": out["reward"].view(ants, b).t(), "log_likelihood": out["log_likelihood"].view(ants, b).t()})
        opt.zero_grad()
        loss.backward()
        opt.step()
        rewards.append(out["reward"].mean())
    rewards = torch.stack(rewards).cpu()
    first, last = float(rewards[:5].mean()), float(rewards[-5:].mean())
    print(f"mean reward: first five steps {first:.3f}, last five {last:.3f}")
    assert last > first
