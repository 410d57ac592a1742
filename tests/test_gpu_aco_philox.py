"""The Ant System kernels' own noise (csrc/aco_tsp.hip, csrc/aco_cvrp.hip with ``ln_noise=None``, the only way the product
launches them) pinned word for word: a Philox launch must write exactly what the same launch writes when ``ln_noise`` is the
stream restated on the host (tests/philox_ref.py, which tests/test_philox_cpu.py pins to the published generator). The
selection rule given the noise is tested exactly elsewhere (tests/test_gpu_aco.py, tests/test_gpu_aco_cvrp.py), so this is
the whole statement "the kernel's noise is the stated function of (seed, offset, iteration, step, row, node)": which step
counter an iteration of a fused launch uses, which row an ant draws from, the second 64-lane pass, both words of the offset,
the device seed word of a captured graph, and the keys ``AntSystem`` hands to its launches. Every comparison is
``torch.equal``."""
from functools import lru_cache

import pytest
import torch

from rl4co_amd import _lib
from tests import aco_cvrp_ref as RC
from tests import aco_ref as R
from tests import philox_ref as P
from tests import test_gpu_aco as T
from tests import test_gpu_aco_cvrp as C

pytestmark = pytest.mark.gpu
SAMPLE = _lib.ACO_SAMPLE
SEED, OFFSET, HIGH_OFFSET = 0x1234ABCD5678, 7, 2**32 + 5
DEV_WORD = 0x0FEDCBA987654321
KW = dict(alpha=1.1, beta=0.8, decay=0.9, Q=0.25)
TSP_KEYS = ("iter_actions", "iter_reward", "actions", "reward", "logps", "final_reward", "final_actions", "final_reward_cache")
CVRP_KEYS = TSP_KEYS + ("iter_lengths", "lengths", "final_iteration")


def _K():
    from rl4co_amd import kernels as K

    return K


def _assert_same(got, want, keys):
    """Two launches' outputs (dicts on the CPU, the pheromone after the launch under "pheromone") agree in every tensor."""
    for k in keys + ("pheromone",):
        assert torch.equal(got[k], want[k]), k


# ---- TSP ---------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _tsp_problem(b, n, ants, iters):
    locs, heu, phe0 = T._instance(b, n, 4000 + n)
    g = torch.Generator().manual_seed(n + ants)
    return locs, heu, phe0, torch.randint(0, n, (iters, ants * b), generator=g)


def _tsp_philox(b, n, ants, iters, seed, offset, seed_dev=None, **kw):
    locs, heu, phe0, starts = _tsp_problem(b, n, ants, iters)
    phe = phe0.cuda()
    out = T._cpu(_K().aco_tsp(phe, n_ants=ants, iterations=iters, log_heuristic=heu.cuda(), locs=locs.cuda(),
                              start_nodes=starts.cuda(), philox_seed=seed, philox_offset=offset, philox_seed_dev=seed_dev,
                              record_iterations=True, **kw))
    out["pheromone"] = phe.cpu()
    return out


def _tsp_parity(b, n, ants, iters, seed, offset, **kw):
    locs, heu, phe0, starts = _tsp_problem(b, n, ants, iters)
    phe = phe0.cuda()
    out = T._fused(phe, ants, iters, heu, locs, starts, P.tsp_stream(seed, offset, iters, n, ants * b), **kw)
    out["pheromone"] = phe.cpu()
    return out


# (B, N (0: one past the LDS tier), ants, iterations): N no multiple of 4 with rows != B != ants and several iterations;
# ants == N; the second 64-lane pass (node 64); the global-memory tier
TSP_SHAPES = [(3, 21, 6, 3), (2, 5, 5, 2), (2, 65, 3, 2), (2, 0, 4, 2)]
FIRST = TSP_SHAPES[0]


@pytest.mark.parametrize("b,n,ants,iters", TSP_SHAPES, ids=["n21", "ants_eq_n", "n65", "global_tier"])
def test_tsp_fused_philox_equals_the_restated_stream(b, n, ants, iters):
    n = n or _K().aco_lds_nodes() + 1
    got = _tsp_philox(b, n, ants, iters, SEED, OFFSET, **KW)
    _assert_same(got, _tsp_parity(b, n, ants, iters, SEED, OFFSET, **KW), TSP_KEYS)
    assert T._is_permutation(got["iter_actions"], n) and not torch.equal(got["pheromone"], _tsp_problem(b, n, ants, iters)[2])


@pytest.mark.parametrize("offset,temperature", [(HIGH_OFFSET, 1.0), (OFFSET, 0.7)], ids=["offset_above_2_32", "temperature"])
def test_tsp_fused_philox_offset_high_word_and_temperature(offset, temperature):
    got = _tsp_philox(*FIRST, SEED, offset, temperature=temperature, **KW)
    _assert_same(got, _tsp_parity(*FIRST, SEED, offset, temperature=temperature, **KW), TSP_KEYS)
    base = _tsp_philox(*FIRST, SEED, OFFSET, **KW)
    assert not torch.equal(got["iter_actions"], base["iter_actions"])
    if offset == HIGH_OFFSET:  # the high word is part of the counter: the low word alone draws other noise
        low = _tsp_philox(*FIRST, SEED, offset & 0xFFFFFFFF, **KW)
        assert not torch.equal(got["iter_actions"], low["iter_actions"])


def test_tsp_iteration_i_draws_at_offset_plus_i_times_n():
    b, n, ants, iters = FIRST
    locs, heu, phe0, starts = _tsp_problem(*FIRST)
    fused = _tsp_philox(*FIRST, SEED, OFFSET, **KW)
    state = R.fresh_state(phe0)

    def sample_only(i, offset):
        return T._cpu(_K().aco_tsp(state["pheromone"].cuda(), n_ants=ants, phases=SAMPLE, log_heuristic=heu.cuda(),
                                   locs=locs.cuda(), start_nodes=starts[i : i + 1].contiguous().cuda(), philox_seed=SEED,
                                   philox_offset=offset, **KW))

    for i in range(iters):
        s = sample_only(i, OFFSET + i * n)
        assert torch.equal(s["actions"], fused["iter_actions"][i]) and torch.equal(s["reward"], fused["iter_reward"][i])
        if i > 0:
            assert not torch.equal(sample_only(i, OFFSET)["actions"], fused["iter_actions"][i])
        R.update(state, fused["iter_actions"][i], fused["iter_reward"][i], KW["decay"], KW["Q"])
    assert torch.equal(state["pheromone"], fused["pheromone"])  # (the states before each iteration were the launch's own)


def _seed_word():
    return torch.tensor([DEV_WORD], dtype=torch.int64, device="cuda")  # rl4co_amd/graph.py: one int64 word on the device


def test_tsp_device_seed_word_is_xored_into_the_seed():
    word = _seed_word()
    got = _tsp_philox(*FIRST, SEED, OFFSET, seed_dev=word, **KW)
    _assert_same(got, _tsp_philox(*FIRST, SEED ^ DEV_WORD, OFFSET, **KW), TSP_KEYS)
    _assert_same(got, _tsp_parity(*FIRST, SEED ^ DEV_WORD, OFFSET, **KW), TSP_KEYS)
    assert not torch.equal(got["iter_actions"], _tsp_philox(*FIRST, SEED, OFFSET, **KW)["iter_actions"])
    assert int(word.item()) == DEV_WORD


# ---- CVRP --------------------------------------------------------------------------------------------------------------------
# (B, n (0: one past the LDS tier), ants, iterations): the sizes of test_fused_equals_split_launches and the global-memory tier
CVRP_SHAPES = [(3, 21, 6, 3), (2, 0, 4, 2)]
CVRP_IDS = ["n21", "global_tier"]
MODES = ["multisample", "multistart"]


@lru_cache(maxsize=None)
def _cvrp_problem(b, n, ants, iters, mode):
    """demand 0.1 .. 0.4 of the capacity (tests/test_gpu_aco_cvrp.py's _problem): a route holds about four customers, so
    every row returns to the depot mid-tour and the rows finish at different steps."""
    n = n or _K().aco_cvrp_lds_nodes() + 1
    prob = C._problem(b, n, 4100 + n)
    g = torch.Generator().manual_seed(n + ants)
    starts = torch.randint(1, n, (iters, ants * b), generator=g) if mode == "multistart" else None
    return n, prob, starts


def _cvrp_philox(shape, mode, seed, offset, seed_dev=None, **kw):
    b, _, ants, iters = shape
    n, prob, starts = _cvrp_problem(*shape, mode)
    locs, heu, phe0, demand, cap = prob
    phe = phe0.cuda()
    out = C._cpu(_K().aco_cvrp(phe, n_ants=ants, iterations=iters, log_heuristic=heu.cuda(), locs=locs.cuda(),
                               demand=demand.cuda(), vehicle_capacity=cap.cuda(),
                               start_nodes=None if starts is None else starts.cuda(), philox_seed=seed, philox_offset=offset,
                               philox_seed_dev=seed_dev, record_iterations=True, **kw))
    out["pheromone"] = phe.cpu()
    return out


def _cvrp_parity(shape, mode, seed, offset, **kw):
    b, _, ants, iters = shape
    n, prob, starts = _cvrp_problem(*shape, mode)
    phe = prob[2].cuda()
    out = C._fused(phe, ants, iters, prob, starts, P.cvrp_stream(seed, offset, iters, n, ants * b), **kw)
    out["pheromone"] = phe.cpu()
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", CVRP_SHAPES, ids=CVRP_IDS)
def test_cvrp_fused_philox_equals_the_restated_stream(shape, mode):
    n, prob, starts = _cvrp_problem(*shape, mode)
    w = _K().aco_cvrp_width(n)
    assert w == P.cvrp_width(n)
    got = _cvrp_philox(shape, mode, SEED, OFFSET, **KW)
    _assert_same(got, _cvrp_parity(shape, mode, SEED, OFFSET, **KW), CVRP_KEYS)
    C._valid(prob[0], prob[3], prob[4], got["iter_actions"].reshape(-1, w))
    lengths, acts = got["iter_lengths"], got["iter_actions"]
    assert int(lengths.min()) < int(lengths.max()) < w  # rows finish at different steps, a zero-filled tail follows each
    inner = torch.arange(w) < (lengths[..., None] - 1)
    assert bool(((acts == 0) & inner)[..., 1:].any(-1).all())  # every row returns to the depot mid-tour
    assert bool((acts[torch.arange(w) >= lengths[..., None]] == 0).all())
    assert not torch.equal(got["pheromone"], prob[2]) and not torch.equal(acts[0], acts[1])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("offset,temperature", [(HIGH_OFFSET, 1.0), (OFFSET, 0.7)], ids=["offset_above_2_32", "temperature"])
def test_cvrp_fused_philox_offset_high_word_and_temperature(offset, temperature, mode):
    shape = CVRP_SHAPES[0]
    got = _cvrp_philox(shape, mode, SEED, offset, temperature=temperature, **KW)
    _assert_same(got, _cvrp_parity(shape, mode, SEED, offset, temperature=temperature, **KW), CVRP_KEYS)
    assert not torch.equal(got["iter_actions"], _cvrp_philox(shape, mode, SEED, OFFSET, **KW)["iter_actions"])
    if offset == HIGH_OFFSET:
        low = _cvrp_philox(shape, mode, SEED, offset & 0xFFFFFFFF, **KW)
        assert not torch.equal(got["iter_actions"], low["iter_actions"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", CVRP_SHAPES, ids=CVRP_IDS)
def test_cvrp_iteration_i_draws_at_offset_plus_i_times_w(shape, mode):
    b, _, ants, iters = shape
    n, prob, starts = _cvrp_problem(*shape, mode)
    locs, heu, phe0, demand, cap = prob
    w = P.cvrp_width(n)
    fused = _cvrp_philox(shape, mode, SEED, OFFSET, **KW)
    state = RC.fresh_state(phe0)

    def sample_only(i, offset):
        return C._cpu(_K().aco_cvrp(state["pheromone"].cuda(), n_ants=ants, phases=SAMPLE, log_heuristic=heu.cuda(),
                                    locs=locs.cuda(), demand=demand.cuda(), vehicle_capacity=cap.cuda(),
                                    start_nodes=None if starts is None else starts[i : i + 1].contiguous().cuda(),
                                    philox_seed=SEED, philox_offset=offset, **KW))

    for i in range(iters):
        s = sample_only(i, OFFSET + i * w)
        assert torch.equal(s["actions"], fused["iter_actions"][i]) and torch.equal(s["reward"], fused["iter_reward"][i])
        assert torch.equal(s["lengths"], fused["iter_lengths"][i])
        if i > 0:
            assert not torch.equal(sample_only(i, OFFSET)["actions"], fused["iter_actions"][i])
            assert not torch.equal(sample_only(i, OFFSET + i * n)["actions"], fused["iter_actions"][i])  # (W, not N)
        RC.update(state, fused["iter_actions"][i], fused["iter_reward"][i], KW["decay"], KW["Q"])
    assert torch.equal(state["pheromone"], fused["pheromone"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", CVRP_SHAPES, ids=CVRP_IDS)
def test_cvrp_device_seed_word_is_xored_into_the_seed(shape, mode):
    got = _cvrp_philox(shape, mode, SEED, OFFSET, seed_dev=_seed_word(), **KW)
    _assert_same(got, _cvrp_philox(shape, mode, SEED ^ DEV_WORD, OFFSET, **KW), CVRP_KEYS)
    _assert_same(got, _cvrp_parity(shape, mode, SEED ^ DEV_WORD, OFFSET, **KW), CVRP_KEYS)
    assert not torch.equal(got["iter_actions"], _cvrp_philox(shape, mode, SEED, OFFSET, **KW)["iter_actions"])


# ---- the class hands out the keys ----------------------------------------------------------------------------------------------
RUN_SEED = 5


def _drawn_keys(seed, count):
    """What AntSystem draws after torch.manual_seed(seed): one key per launch that samples, offset 0."""
    torch.manual_seed(seed)
    return [int(torch.randint(0, 2**62, (1,)).item()) for _ in range(count)]


def _picker(table):
    """A deterministic select_start_nodes_fn: call i returns row i of ``table``."""
    calls = []

    def pick(td_, env_, num_starts):
        calls.append(num_starts)
        return table[len(calls) - 1].cuda()

    return pick


def _start_table(low, n, iters, rows):
    return torch.randint(low, n, (iters, rows), generator=torch.Generator().manual_seed(17))


def test_class_run_tsp_launches_with_the_first_drawn_key():
    from rl4co_amd import AntSystem

    env, td, heu = T._problem()
    iters, ants, b, n = 3, 8, 6, 20
    table = _start_table(0, n, iters, ants * b)
    (key,) = _drawn_keys(RUN_SEED, 1)
    aco = AntSystem(heu, n_ants=ants)
    torch.manual_seed(RUN_SEED)
    aco.run(td, env, iters, dict(T.KW, select_start_nodes_fn=_picker(table), temperature=0.8))
    phe = torch.ones(b, n, n).cuda()
    want = T._fused(phe, ants, iters, heu.cpu(), td["locs"].cpu(), table, P.tsp_stream(key, 0, iters, n, ants * b), alpha=1.0,
                    beta=1.0, decay=float(aco.decay), Q=float(aco.Q), temperature=0.8)
    its = T._cpu(aco.last_iterations)
    assert torch.equal(its["actions"], want["iter_actions"]) and torch.equal(its["reward"], want["iter_reward"])
    assert torch.equal(aco.pheromone, phe) and torch.equal(aco.final_reward.cpu(), want["final_reward"])


def test_class_run_with_local_search_launches_iteration_i_with_the_ith_drawn_key():
    from rl4co_amd import AntSystem

    env, td, heu = T._problem()
    iters, ants, b, n = 3, 8, 6, 20
    table = _start_table(0, n, iters, ants * b)
    keys = _drawn_keys(RUN_SEED, iters)
    assert len(set(keys)) == iters
    aco = AntSystem(heu, n_ants=ants, use_local_search=True)
    torch.manual_seed(RUN_SEED)
    aco.run(td, env, iters, dict(T.KW, select_start_nodes_fn=_picker(table)))
    its = T._cpu(aco.last_iterations)
    state = R.fresh_state(torch.ones(b, n, n))

    def sampled(i, key):
        out = _K().aco_tsp(state["pheromone"].cuda(), n_ants=ants, phases=SAMPLE, log_heuristic=heu, locs=td["locs"],
                           start_nodes=table[i : i + 1].contiguous().cuda(), ln_noise=P.tsp_stream(key, 0, 1, n, ants * b).cuda(),
                           alpha=1.0, beta=1.0)
        return out["reward"].cpu()

    for i in range(iters):
        assert torch.equal(sampled(i, keys[i]), its["sampled_reward"][i]), i
        if i > 0:  # every iteration has a key of its own
            assert not torch.equal(sampled(i, keys[0]), its["sampled_reward"][i])
        R.update(state, its["actions"][i], its["reward"][i], aco.decay, aco.Q)
    assert torch.equal(state["pheromone"], aco.pheromone.cpu())  # (the states before each iteration were the run's own)


@pytest.mark.parametrize("mode", MODES)
def test_class_run_cvrp_launches_with_the_first_drawn_key(mode):
    from rl4co_amd import AntSystem

    env, td, heu = C._class_problem()
    iters, ants, b, n = 3, 8, 6, 21
    table = _start_table(1, n, iters, ants * b) if mode == "multistart" else None
    kw = dict(C.MS) if table is None else dict(multistart=True, num_starts=ants, select_best=False,
                                               select_start_nodes_fn=_picker(table))
    (key,) = _drawn_keys(RUN_SEED, 1)
    aco = AntSystem(heu, n_ants=ants)
    torch.manual_seed(RUN_SEED)
    aco.run(td, env, iters, kw)
    prob = (td["locs"].cpu(), heu.cpu(), None, td["demand"].cpu(), td["vehicle_capacity"].reshape(-1).cpu())
    phe = torch.ones(b, n, n).cuda()
    want = C._fused(phe, ants, iters, prob, table, P.cvrp_stream(key, 0, iters, n, ants * b), alpha=1.0, beta=1.0,
                    decay=float(aco.decay), Q=float(aco.Q))
    its = C._cpu(aco.last_iterations)
    assert torch.equal(its["actions"], want["iter_actions"]) and torch.equal(its["reward"], want["iter_reward"])
    assert torch.equal(its["lengths"], want["iter_lengths"])
    assert torch.equal(aco.pheromone, phe) and torch.equal(aco.final_reward.cpu(), want["final_reward"])
