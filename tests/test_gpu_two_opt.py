"""TSP 2-opt local search on the MI355X (csrc/tsp_two_opt.hip): the kernel's tours and iteration counts against the records
of the reference's own local_search.py and against the CPU restatement (tests/two_opt_ref.py) at the shapes where the
kernel changes path. Every comparison is exact: there is no tolerance anywhere.

At N = 200 the kernel is in matrix mode, not on the on-the-fly path the case was meant for: the LDS formula admits 201
nodes. The on-the-fly and the global-memory paths are the ``lds_nodes + 1`` cases."""
from functools import lru_cache

import pytest
import torch

from tests import two_opt_ref as R

pytestmark = pytest.mark.gpu


def _kernel(acts, *, locs=None, distances=None, max_iterations=1000, **kw):
    from rl4co_amd import kernels as K

    src = dict(locs=locs.cuda()) if distances is None else dict(distances=distances.cuda())
    tours, iters = K.tsp_two_opt(acts.cuda(), max_iterations=max_iterations, return_iterations=True, **src, **kw)
    return tours.cpu(), iters.cpu()


@lru_cache(maxsize=None)
def _random_case(b: int, n: int, cap: int = 1000):
    """Seeded coordinates and starting tours with the restatement's answer (computed once, shared, left unchanged)."""
    locs, acts = R.random_locs(b, n, seed=1000 + n), R.random_tours(b, n, seed=n)
    dist = R.distance_matrix(locs)
    tours, iters = R.two_opt(dist, acts, cap)
    return locs, dist, acts, tours, iters


@pytest.mark.parametrize("case", list(R.CASES))
def test_records(case):
    from rl4co_amd.envs import TSPEnv

    rec = R.record(case)
    cap = R.CASES[case][3]
    if "in_distances" in rec:
        tours, iters = _kernel(rec["in_actions"], distances=rec["in_distances"], max_iterations=cap)
        via_env = TSPEnv.local_search({"locs": torch.zeros(*rec["in_distances"].shape[:2], 2, device="cuda"),
                                       "distances": rec["in_distances"].cuda()}, rec["in_actions"].cuda(), max_iterations=cap)
    else:
        tours, iters = _kernel(rec["in_actions"], locs=rec["in_locs"], max_iterations=cap)
        via_env = TSPEnv.local_search({"locs": rec["in_locs"].cuda()}, rec["in_actions"].cuda(), max_iterations=cap, num_threads=2)
    assert via_env.is_cuda and via_env.dtype == torch.int64
    assert torch.equal(via_env.cpu(), rec["out_actions"])
    assert torch.equal(tours, rec["out_actions"])
    assert torch.equal(iters, rec["iterations"])


@pytest.mark.parametrize("b,n,cap", [(33, 2, 1000), (33, 3, 1000), (33, 4, 1000), (33, 5, 1000),  # no or few pairs
                                     (5, 64, 1000), (5, 65, 1000),                                # the wave edge
                                     (7, 100, 1000),                                              # several pairs per thread
                                     (3, 200, 40)])
def test_shapes_against_the_restatement(b, n, cap):
    locs, dist, acts, want, want_iters = _random_case(b, n, cap)
    tours, iters = _kernel(acts, locs=locs, max_iterations=cap)
    assert torch.equal(tours, want) and torch.equal(iters, want_iters)
    tours, iters = _kernel(acts, distances=dist, max_iterations=cap)
    assert torch.equal(tours, want) and torch.equal(iters, want_iters)


@pytest.mark.parametrize("over", [0, 1])
def test_tier_edge_both_sources(over):
    """N = lds_nodes: the matrix in LDS (built from locs, staged from distances); N = lds_nodes + 1: coordinates in LDS
    and distances computed where used, or entries read from global memory."""
    from rl4co_amd import kernels as K

    n = K.two_opt_lds_nodes() + over
    locs, dist, acts, want, want_iters = _random_case(2, n)
    assert int(want_iters.min()) > 50  # a real search
    for src in (dict(locs=locs), dict(distances=dist)):
        tours, iters = _kernel(acts, **src)
        assert torch.equal(tours, want) and torch.equal(iters, want_iters), list(src)


def test_asymmetric_matrix_beyond_the_lds_tier():
    """The index order of `change` on the global-memory path: an asymmetric matrix, N above the LDS tier, capped."""
    from rl4co_amd import kernels as K

    n = K.two_opt_lds_nodes() + 3
    dist = torch.rand(2, n, n, generator=torch.Generator().manual_seed(7))
    acts = R.random_tours(2, n, seed=8)
    want, want_iters = R.two_opt(dist, acts, 25)
    tours, iters = _kernel(acts, distances=dist, max_iterations=25)
    assert torch.equal(tours, want) and torch.equal(iters, want_iters)


@pytest.mark.parametrize("cap", [0, 1, 3])
def test_max_iterations(cap):
    rec, full = R.record("tsp20"), R.record("tsp20")["iterations"]
    tours, iters = _kernel(rec["in_actions"], locs=rec["in_locs"], max_iterations=cap)
    want, want_iters = R.two_opt(R.record_distances(rec), rec["in_actions"], cap)
    assert torch.equal(tours, want) and torch.equal(iters, want_iters)
    if cap == 0:
        assert torch.equal(tours, rec["in_actions"])
    assert torch.equal(iters[full > cap], torch.full_like(iters[full > cap], cap)) and bool((full > 3).all())


def test_in_place():
    from rl4co_amd import kernels as K

    rec = R.record("tsp50")
    acts = rec["in_actions"].cuda()
    out = K.tsp_two_opt(acts, locs=rec["in_locs"].cuda(), out=acts)
    assert out is acts
    assert torch.equal(acts.cpu(), rec["out_actions"])


def test_properties():
    locs, dist, acts, _, _ = _random_case(7, 100, 1000)
    first, iters = _kernel(acts, locs=locs)
    again, iters2 = _kernel(acts, locs=locs)
    assert torch.equal(first, again) and torch.equal(iters, iters2)  # two runs are bit-identical
    assert torch.equal(first.sort(1).values, acts.sort(1).values)   # every row a permutation of its input row
    before, after = R.tour_length64(dist, acts), R.tour_length64(dist, first)
    assert bool((after <= before).all()) and bool((after < before).any())


def test_bad_index_row_comes_back_unchanged():
    from rl4co_amd import _lib
    from rl4co_amd import kernels as K

    rec = R.record("tsp20")
    acts = rec["in_actions"].clone()
    acts[3, 7] = 20   # == N
    acts[9, 0] = -1
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    tours, iters = _kernel(acts, locs=rec["in_locs"], err=err)
    assert int(err.item()) == _lib.EBIT_TOUR_INDEX
    good = torch.ones(16, dtype=torch.bool)
    good[[3, 9]] = False
    assert torch.equal(tours[~good], acts[~good]) and iters[~good].tolist() == [0, 0]
    assert torch.equal(tours[good], rec["out_actions"][good]) and torch.equal(iters[good], rec["iterations"][good])
    with pytest.raises(AssertionError, match="tour index out of range"):
        K.tsp_two_opt(acts.cuda(), locs=rec["in_locs"].cuda())


def test_after_a_rollout():
    from rl4co_amd.envs import get_env
    from rl4co_amd.policy import AttentionModelPolicy
    from rl4co_amd.tensordict import TensorDict

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    pol = AttentionModelPolicy("tsp").eval().to(dev)
    env = get_env("tsp", generator_params=dict(num_loc=20, device=dev), device=dev)
    td = env.reset(TensorDict({"locs": R.random_locs(8, 20, seed=5).to(dev)}, batch_size=[8]))
    with torch.inference_mode():
        out = pol(td, env, phase="test", decode_type="greedy")
    better = env.local_search(td, out["actions"])
    assert better.device == out["actions"].device and better.dtype == torch.int64
    env.check_solution_validity(td, better)
    reward = env.get_reward(td, better)
    assert bool((reward >= out["reward"]).all()) and bool((reward > out["reward"]).any())
