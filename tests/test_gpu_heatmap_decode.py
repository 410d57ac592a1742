"""Greedy and top-k / top-p decoding of a heatmap on the MI355X (csrc/ant_system.h: filter_kept, ant_step<true>; the *_opts
entry points; rl4co_amd.aco.heatmap_decode; rl4co_amd.NARGNNPolicy) against tests/heatmap_decode_ref.py.

Sizes: N = 5, 64, 65, 130 (1, 1, 2 and 4 words per lane: the ladder's edges) and 150 (above the LDS tier) for tsp, n = 12 and
66 for the depot graphs, B = 3 with 3 ants. Tolerances: actions, kept sets, rewards of tsp and every bit-for-bit comparison
are exact; a gradient stays within the unfiltered path's GRAD_TOL (tests/aco_grad_ref.py, tests/aco_depot_grad_ref.py: 4 x
the reference's own fp32-vs-float64 deviation, weights in (0, 1]); a summed log-likelihood within W x the unfiltered path's
per-step STEP_TOL (a sum of at most W per-step log-probs, each within STEP_TOL). Measured on the MI355X: gradient errors
1.0e-07 .. 5.1e-07 (0.20 .. 0.98 of the reference's own fp32 noise floor; 4 is allowed), log-likelihood errors of the recorded
rollouts 9.5e-07 .. 5.7e-06, at most 0.07 % of the kept-set steps left out as near-ties."""
from functools import lru_cache

import pytest
import torch

from rl4co_amd import _lib
from tests import aco_cvrp_ref as CV
from tests import aco_depot_grad_ref as DG
from tests import aco_grad_ref as G
from tests import aco_ref as A
from tests import heatmap_decode_ref as H

pytestmark = pytest.mark.gpu
B, ANTS = 3, 3
SIZES = [("tsp", 5), ("tsp", 64), ("tsp", 65), ("tsp", 130), ("tsp", 150), ("cvrp", 12), ("cvrp", 66), ("op", 12), ("op", 66),
         ("pctsp", 12), ("pctsp", 66)]
SMALL = [("tsp", 5), ("tsp", 65), ("cvrp", 12), ("op", 12), ("pctsp", 12)]


def _K():
    from rl4co_amd import kernels as K

    return K


@lru_cache(maxsize=None)
def _case(env, n, grid=False, seed=0):
    """(heatmap, data, start_nodes or None) on the CPU, computed once and left unchanged."""
    heat = H.grid_heatmap(B, n, 100 + n + seed) if grid else H.random_heatmap(B, n, 200 + n + seed)
    return heat, H.instance(env, B, n, 300 + n), (H.tsp_starts(B, n, ANTS) if env == "tsp" else None)


def _search(env, heat, data, starts, **kw):
    """One SAMPLE launch through kernels.aco_search with a pheromone of ones."""
    K = _K()
    given = {k: v.cuda() for k, v in data.items() if k != "locs"}
    if env == "tsp":
        given["start_nodes"] = starts[None].cuda()
    return K.aco_search(env, torch.ones_like(heat).cuda(), n_ants=ANTS, phases=_lib.ACO_SAMPLE, log_heuristic=heat.cuda(),
                        locs=data["locs"].cuda(), **given, **kw)


def _decode(env, heat, data, starts, **kw):
    from rl4co_amd.aco import heatmap_decode

    return heatmap_decode(heat, data["locs"].cuda(), n_ants=ANTS, start_nodes=None if starts is None else starts.cuda(),
                          env_name=env, td=H.as_td(env, data), **kw)


# ---- 1. options off is the parent, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("env,n", SMALL)
def test_options_off_is_the_parent_bit_for_bit(env, n, monkeypatch):
    from rl4co_amd.aco import heatmap_rollout

    K = _K()
    heat, data, starts = _case(env, n)
    old = _search(env, heat, data, starts, philox_seed=77, all_logps=True)
    weights = torch.rand(ANTS * B, generator=torch.Generator().manual_seed(5)).cuda()
    grad_kw = {} if env == "tsp" else DG.kernel_data(env, data)
    old_grad = K.aco_logp_grad(env, heat.cuda(), old["actions"], weights, **grad_kw)
    # the *_opts symbols with a zero-initialised struct
    monkeypatch.setattr(K, "heatmap_decode_opts", lambda greedy, top_k, top_p, n: _lib.HeatmapDecodeOpts())
    new = _search(env, heat, data, starts, philox_seed=77, all_logps=True)
    new_grad = K.aco_logp_grad(env, heat.cuda(), old["actions"], weights, **grad_kw)
    monkeypatch.undo()
    for key in ("actions", "logps", "reward", "all_logps"):
        assert torch.equal(old[key], new[key]), key
    assert torch.equal(old_grad, new_grad)
    # heatmap_decode("sampling") against heatmap_rollout
    h1, h2 = heat.cuda().requires_grad_(True), heat.cuda().requires_grad_(True)
    td = H.as_td(env, data)
    s = None if starts is None else starts.cuda()
    a = heatmap_rollout(h1, data["locs"].cuda(), n_ants=ANTS, start_nodes=s, seed=78, env_name=env, td=td)
    b = _decode(env, h2, data, starts, decode_type="sampling", seed=78)
    for key in ("actions", "logps", "log_likelihood", "reward"):
        assert torch.equal(a[key], b[key]), key
    (a["log_likelihood"] * weights).sum().backward()
    (b["log_likelihood"] * weights).sum().backward()
    assert torch.equal(h1.grad, h2.grad)


# ---- 2. greedy tours, exact -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,n", SIZES)
def test_greedy_tours_are_the_float64_rollout(env, n):
    heat, data, starts = _case(env, n, grid=True)
    want = H.greedy_rollout(env, heat, data, ANTS, starts)
    out = _decode(env, heat.cuda(), data, starts, decode_type="greedy")
    assert torch.equal(out["actions"].cpu(), want)
    again = _decode(env, heat.cuda(), data, starts, decode_type="greedy", seed=12345)  # no noise is read: the seed is nothing
    assert torch.equal(again["actions"], out["actions"]) and torch.equal(again["logps"], out["logps"])
    if env == "tsp":
        assert torch.equal(out["reward"].cpu(), A.tour_reward(data["locs"], want))


@pytest.mark.parametrize("env,n", [("tsp", 65), ("cvrp", 12)])
def test_greedy_takes_the_lowest_node_on_equal_maxima(env, n):
    heat, data, starts = _case(env, n, grid=True)
    heat = heat.clone()
    heat[:, :, 1:] = heat[:, :, 1:].clamp(max=2.0)  # every row: several customers share the maximum 2.0
    want = H.greedy_rollout(env, heat, data, ANTS, starts)
    out = _decode(env, heat.cuda(), data, starts, decode_type="greedy")
    assert torch.equal(out["actions"].cpu(), want)


# ---- 3. kept sets, exact ----------------------------------------------------------------------------------------------------------------
FILTERS = [(1, 0.0, 1.0), (3, 0.0, 1.0), (2000, 0.0, 1.0), (0, 0.5, 1.0), (0, 0.9, 1.0), (3, 0.5, 0.7), (0, 0.9, 0.7)]


@pytest.mark.parametrize("env,n", SIZES)
def test_kept_sets_are_filter_f64s(env, n):
    K = _K()
    heat, data, starts = _case(env, n)
    compared = left_out = 0
    for top_k, top_p, temperature in FILTERS:
        if top_k >= n:  # (decoding_filter turns k >= n off on the host: hand the kernel a k above the feasible count)
            top_k = n - 1
        out = _search(env, heat, data, starts, philox_seed=31 + top_k, all_logps=True, top_k=top_k, top_p=top_p,
                      temperature=temperature)
        actions = out["actions"].cpu()
        cur, infeasible, live = H.step_table(env, heat, data, actions, None)
        kept, margin = H.kept_sets(H.step_logits(heat, cur, infeasible, temperature), top_k, top_p)
        got = torch.isfinite(out["all_logps"].cpu())
        use = live & (margin >= H.MARGIN)
        compared += int(live.sum())
        left_out += int((live & ~use).sum())
        assert torch.equal(got[use], kept[use]), (top_k, top_p, temperature)
        # the sampled action is in the kept set and its log-prob is the reported one
        taken = out["all_logps"].cpu().gather(2, actions[:, :, None]).squeeze(2)
        assert torch.equal(taken[live], out["logps"].cpu()[live]) and bool(torch.isfinite(taken[live]).all())
    share = left_out / compared
    print(f"{env} n={n}: {compared} steps compared, {left_out} left out ({share:.4f})")
    assert share <= H.LEFT_OUT_SHARE


@pytest.mark.parametrize("env,n", SMALL)
def test_top_k_1_sampling_is_greedy(env, n):
    heat, data, starts = _case(env, n, grid=True)
    greedy = _decode(env, heat.cuda(), data, starts, decode_type="greedy")
    top1 = _decode(env, heat.cuda(), data, starts, decode_type="sampling", top_k=1, seed=9)
    assert torch.equal(greedy["actions"], top1["actions"])
    assert bool((top1["logps"] == 0).all())  # one node kept: its probability is 1


# ---- 4. sampling draws from the reported log-probs: forced replay --------------------------------------------------------------------
@pytest.mark.parametrize("env,n", SMALL)
def test_forced_replay_of_a_filtered_rollout(env, n):
    heat, data, starts = _case(env, n)
    kw = dict(top_k=4, top_p=0.8, temperature=0.7)
    out = _decode(env, heat.cuda(), data, starts, decode_type="sampling", seed=3, **kw)
    again = _decode(env, heat.cuda(), data, starts, actions=out["actions"], **kw)
    assert torch.equal(again["logps"], out["logps"]) and torch.equal(again["reward"], out["reward"])
    # forced actions outside the kept set: rows sampled WITHOUT a filter stay feasible (feasibility does not depend on the
    # filter) and, evaluated under top_k = 1, hold a step that is not the argmax of its row
    free = _decode(env, heat.cuda(), data, starts, decode_type="sampling", seed=4)
    assert not torch.equal(free["actions"], _decode(env, heat.cuda(), data, starts, decode_type="greedy")["actions"])
    with pytest.raises(AssertionError, match="Logprobs should not be -inf"):
        _decode(env, heat.cuda(), data, starts, actions=free["actions"], top_k=1)


# ---- 5. the gradient under the filter -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,n", SIZES)
def test_gradient_under_the_filter(env, n):
    K = _K()
    heat, data, starts = _case(env, n)
    top_k, top_p, temperature = 5, 0.9, 0.7
    h = heat.cuda().requires_grad_(True)
    out = _decode(env, h, data, starts, decode_type="sampling", seed=21, top_k=top_k, top_p=top_p, temperature=temperature)
    weights = torch.rand(ANTS * B, generator=torch.Generator().manual_seed(6)) * 0.9 + 0.1  # fixed, positive, <= 1
    (out["log_likelihood"] * weights.cuda()).sum().backward()
    actions = out["actions"].cpu()
    cur, infeasible, live = H.step_table(env, heat, data, actions, None)
    kept, margin = H.kept_sets(H.step_logits(heat, cur, infeasible, temperature), top_k, top_p)
    got_kept = torch.isfinite(_search(env, heat, data, starts, forced_actions=out["actions"], all_logps=True, top_k=top_k,
                                      top_p=top_p, temperature=temperature)["all_logps"].cpu())
    near = live & (margin < H.MARGIN)
    kept = torch.where(near[:, :, None], got_kept, kept)  # (a near-tie step: the kernel's own set, as in test 3)
    assert torch.equal(got_kept[live], kept[live])
    logps64, want = H.filtered_logp_grad(heat, actions, cur, live, kept, weights, temperature)
    tol = G.GRAD_TOL if env == "tsp" else DG.GRAD_TOL
    err = float((h.grad.cpu().double() - want).abs().max())
    print(f"{env} n={n}: gradient error {err:.3e} (tol {tol:.3e}, ratio to the noise floor {4 * err / tol:.2f})")
    assert err <= tol
    # removed nodes have gradient exactly 0: a word no kept node of any step maps to
    b_idx = (torch.arange(ANTS * B) % B)[:, None].expand_as(cur)
    touched = torch.zeros(B, n, n, dtype=torch.bool)
    sel = (kept & live[:, :, None]).nonzero()
    touched[b_idx[sel[:, 0], sel[:, 1]], cur[sel[:, 0], sel[:, 1]], sel[:, 2]] = True
    assert bool((h.grad.cpu()[~touched] == 0).all())
    # two launches and two row splits: identical bits
    grad_kw = {} if env == "tsp" else DG.kernel_data(env, data)
    direct = [K.aco_logp_grad(env, heat.cuda(), out["actions"], weights.cuda(), temperature=temperature, top_k=top_k,
                              top_p=top_p, row_split=split, **grad_kw) for split in (1, 1, 3)]
    assert torch.equal(direct[0], direct[1]) and torch.equal(direct[0], direct[2]) and torch.equal(direct[0], h.grad)


# ---- 6. the reference's recorded NARGNNPolicy rollouts -----------------------------------------------------------------------------------
def _record_td(env, rec):
    td = {"locs": rec["locs"].cuda()}
    if env == "cvrp":
        td.update(demand=rec["demand"].cuda(), vehicle_capacity=rec["vehicle_capacity"].cuda())
    return td


class _Given(torch.nn.Module):
    """The stand-in encoder: the recorded heatmap."""

    def __init__(self, heatmap):
        super().__init__()
        self.heatmap = torch.nn.Parameter(heatmap.clone())

    def forward(self, td):
        return self.heatmap, None


def _same_rows(got, want):
    """Kernel rows are W wide and zero-filled; the reference trims to its batch's longest row."""
    return torch.equal(got[:, : want.shape[1]], want) and bool((got[:, want.shape[1]:] == 0).all())


@pytest.mark.parametrize("env", list(H.RECORD_ENVS))
@pytest.mark.parametrize("case", list(H.RECORD_CASES))
def test_recorded_reference_rollouts(env, case):
    from rl4co_amd import NARGNNPolicy

    rec = H.record(env, case)
    kw = dict(H.RECORD_CASES[case])
    phase = kw.pop("phase")
    policy = NARGNNPolicy(encoder=_Given(rec["heatmap"]).cuda(), env_name=env)
    starts = rec["start_nodes"].cuda()
    n = rec["heatmap"].shape[1]
    w = H.width(env, n)
    ll_tol = w * (A.STEP_TOL if env == "tsp" else CV.STEP_TOL)
    if "decode_type" in kw:  # a sampled run follows its own noise: the recorded rows are evaluated under the same filter
        rows = torch.nn.functional.pad(rec["actions"], (0, w - rec["actions"].shape[1])).cuda()
        out = policy(_record_td(env, rec), phase=phase, actions=rows, multistart=True, top_k=kw["top_k"], top_p=kw.get("top_p", 0.0))
    else:
        out = policy(_record_td(env, rec), phase=phase, num_starts=starts.numel() // H.BATCH,
                     select_start_nodes_fn=lambda td, env_, k: starts, **kw)
    assert _same_rows(out["actions"].cpu(), rec["actions"])
    ll_err = float((out["log_likelihood"].detach().cpu() - rec["log_likelihood"]).abs().max())
    print(f"{env} {case}: log-likelihood error {ll_err:.3e} (tol {ll_tol:.3e})")
    assert torch.equal(out["reward"].cpu(), rec["reward"])  # (best-of selection included: the selected rows' rewards)
    assert ll_err <= ll_tol


# ---- 7. a training step with the filter on --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,n", [("tsp", 11), ("cvrp", 12)])
def test_training_step_with_top_k(env, n):
    from rl4co_amd import NARGNNPolicy
    from rl4co_amd.aco import deepaco_loss

    data = H.instance(env, B, n, 400 + n)
    td = H.as_td(env, data)
    grads = {}
    for tag, kw in (("plain", {}), ("top_k", dict(top_k=4))):
        torch.manual_seed(0)
        policy = NARGNNPolicy(env_name=env, num_layers_graph_encoder=2, num_layers_heatmap_generator=2).cuda().train()
        opt = torch.optim.SGD(policy.parameters(), lr=1e-3)
        multi = (dict(num_starts=4, select_start_nodes_fn=lambda td_, env_, k: H.tsp_starts(B, n, k).cuda()) if env == "tsp"
                 else dict(decode_type="sampling", num_samples=4))
        out = policy(td, phase="train", **multi, **kw)
        loss = deepaco_loss({"reward": out["reward"].view(4, B).t(), "log_likelihood": out["log_likelihood"].view(4, B).t()})
        loss.backward()
        grads[tag] = {k: p.grad.clone() for k, p in policy.named_parameters() if p.grad is not None}
        opt.step()
    for key, g in grads["plain"].items():
        assert bool(torch.isfinite(grads["top_k"][key]).all()), key
        if bool((g != 0).any()):
            assert bool((grads["top_k"][key] != 0).any()), key
