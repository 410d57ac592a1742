"""Split-delivery VRP without a GPU: the environment and the torch-fp32 restatement against the recorded reference states,
how many recorded greedy trajectories sit at a near-tie, and the envspec record behind the kernel bindings."""
import pytest
import torch

from rl4co_amd import _lib, envspec
from rl4co_amd import kernels as K
from rl4co_amd.tensordict import TensorDict
from tests import sdvrp_ref
from tests.fake_device import cpu_device  # noqa: F401

GREEDY = ["sdvrp20_greedy", "sdvrp50_greedy"]


@pytest.fixture
def sdvrp_cpu(cpu_device, monkeypatch):  # noqa: F811
    """The test plays the device: the step entry is the restatement (itself pinned to the record below)."""
    monkeypatch.setattr(K, "sdvrp_step", sdvrp_ref.step)
    return cpu_device


def _reset(rec, device):
    from rl4co_amd.envs import get_env

    num_loc = rec["in_locs"].shape[1]
    env = get_env("sdvrp", generator_params=dict(num_loc=num_loc), device=device)
    data = TensorDict({k[3:]: v.clone() for k, v in rec.items() if k.startswith("in_")}, batch_size=[rec["in_locs"].shape[0]])
    return env, env.reset(data)


@pytest.mark.parametrize("case", GREEDY)
def test_env_equals_the_recorded_reference_states(sdvrp_cpu, case):
    rec = sdvrp_ref.record(case)
    env, td = _reset(rec, sdvrp_cpu)
    assert env.name == "sdvrp" and env.has_depot
    rows = sdvrp_ref.STATE_ROWS
    acts = rec["actions"]
    for t in range(acts.shape[1] + 1):
        assert torch.equal(td["action_mask"].to(torch.uint8), rec["states_mask"][:, t]), t
        assert torch.equal(td["used_capacity"].reshape(-1), rec["states_used"][:, t]), t  # bit for bit
        assert torch.equal(td["done"].reshape(-1).to(torch.uint8), rec["states_done"][:, t]), t
        assert torch.equal(td["demand_with_depot"][:rows], rec["states_demand"][:, t]), t
        assert torch.equal(env.get_action_mask(td).to(torch.uint8), rec["states_mask"][:, t]), t
        if t < acts.shape[1]:
            td.set("action", acts[:, t].clone())
            td = env.step(td)["next"]
    assert torch.equal(td["demand_with_depot"], rec["demand_with_depot"])
    assert torch.equal(td["used_capacity"].reshape(-1), rec["used_capacity"])
    assert bool(td["done"].all())
    splits = sum(int(((acts == j).sum(1) > 1).sum()) for j in range(1, acts.max().item() + 1))
    assert splits > 50  # the split-delivery path is what these rollouts exercise


@pytest.mark.parametrize("case", GREEDY)
def test_check_solution_validity(sdvrp_cpu, case):
    rec = sdvrp_ref.record(case)
    env, td = _reset(rec, sdvrp_cpu)
    env.check_solution_validity(td, rec["actions"])
    padded = torch.cat((rec["actions"], torch.zeros(rec["actions"].shape[0], 5, dtype=torch.int64)), 1)
    env.check_solution_validity(td, padded)  # trailing depot padding is neutral
    err = torch.zeros(1, dtype=torch.int32)
    env.check_solution_validity(td, rec["actions"], err=err)
    assert int(err) == 0
    # one delivery removed: the first customer visit of row 3 becomes a depot visit
    cut = rec["actions"].clone()
    t = int((cut[3] != 0).nonzero()[0])
    cut[3, t] = 0
    with pytest.raises(AssertionError):
        env.check_solution_validity(td, cut)
    env.check_solution_validity(td, cut, err=err)
    assert int(err) == _lib.EBIT_INVALID_TOUR


@pytest.mark.parametrize("case", GREEDY)
def test_fragile_share_of_the_record(case):
    """A trajectory is fragile if, at some step, the reference's own best and second-best log-prob are closer than twice the
    per-step tolerance of the teacher-forced comparison: there a kernel may legitimately take the other node."""
    rec = sdvrp_ref.record(case)
    fragile = rec["min_gap"] < 2 * sdvrp_ref.STEP_TOL
    print(f"{case}: {int(fragile.sum())} of {fragile.numel()} trajectories fragile, smallest gap {float(rec['min_gap'].min()):.3e}")
    assert int(fragile.sum()) * 16 <= fragile.numel()


def test_envspec_record_and_binding(sdvrp_cpu, monkeypatch):
    from rl4co_amd.policy import AttentionModelPolicy

    sp = envspec.spec("sdvrp")
    assert sp is envspec.SPECS["sdvrp"] and sp.env_id == _lib.ENV_SDVRP == 6 and sp.has_depot
    # ... and the header's value, a plain integer like the other ids
    import pathlib
    import re

    header = (pathlib.Path(__file__).resolve().parents[1] / "include" / "rl4co_amd.h").read_text()
    ids = {k: int(v) for k, v in re.findall(r"#define (RL4CO_ENV_\w+) (\d+)\b", header)}
    assert ids["RL4CO_ENV_SDVRP"] == sp.env_id == 6 and list(ids.values()).count(6) == 1
    # the decode kernels alone serve it: not the unfolded mode, the one-launch replay or the teacher kernels
    assert not sp.unfold and not sp.replay and not sp.teacher and "dynamic embedding" in sp.no_teacher
    assert sp.dynamic == ("demand_with_depot", "projection", "dyn_vectors") and sp.dynamic.key in sp.keys("traj")
    assert sp.length_reward and not sp.state_reward and not sp.fixed_horizon and not sp.ctx_first and sp.init == "depot"
    assert sp.horizon(21) == 126 == AttentionModelPolicy._max_horizon("sdvrp", 21)
    assert sp.features == (("demand", False, 1),) and sp.passthrough == ("locs", "demand")
    assert callable(getattr(K, sp.step[0])) and set(sp.step[1]) <= set(sp.keys())
    decode = {f[0] for f in _lib.AmDecodeArgs._fields_}
    assert all(f.slot in decode for f in sp.fields) and len({f.slot for f in sp.fields}) == len(sp.fields)

    rec = sdvrp_ref.record("sdvrp20_greedy")
    env, td = _reset(rec, sdvrp_cpu)
    for key in sp.keys() + sp.passthrough:
        assert key in td.keys(), key
    policy = AttentionModelPolicy("sdvrp")
    # (the binding refuses host tensors; here the test plays the device)
    monkeypatch.setattr(K, "_dev", lambda t, dtype=None, name="tensor": t)
    monkeypatch.setattr(K, "_u8", lambda t, name: t.view(torch.uint8) if t.dtype == torch.bool else t)
    for starts in (0, 3):
        rows = 64 * max(starts, 1)
        state = policy._initial_state(td, starts)
        assert sorted(state) == sorted(sp.keys())
        a = _lib.AmDecodeArgs()
        assert K.bind_env_state(a, sp, state, rows, 21) == rows  # no instance data: one "instance" per trajectory
        for f in sp.fields:
            assert getattr(a, f.slot) == state[f.key].data_ptr(), f
            assert state[f.key].data_ptr() != td[f.key].data_ptr(), f  # own storage: the kernels write it
            assert state[f.key].shape == ((rows, 21) if f.shape == "BN" else (rows,)), f
        assert a.visited is None and a.demand is None
        final = policy._final_td(td, state, starts)
        assert sorted(final.keys()) == sorted(sp.passthrough + sp.keys("traj"))
        assert final["demand_with_depot"].data_ptr() == state["demand_with_depot"].data_ptr()
    short = dict(state, demand_with_depot=state["demand_with_depot"][:, :20].contiguous())
    with pytest.raises(ValueError):
        K.bind_env_state(_lib.AmDecodeArgs(), sp, short, rows, 21)


def test_policy_module_tree_and_fold():
    """The decoder carries the reference's dynamic embedding under its state-dict key; the cache folds it to [3, 128]."""
    from rl4co_amd.cache import fold_dynamic, fold_weights
    from rl4co_amd.policy import AttentionModelPolicy

    torch.manual_seed(0)
    pol = AttentionModelPolicy("sdvrp")
    sd = pol.state_dict()
    assert tuple(sd["decoder.dynamic_embedding.projection.weight"].shape) == (384, 1)
    assert "decoder.dynamic_embedding.projection.weight" not in AttentionModelPolicy("cvrp").state_dict()
    w_out = pol.decoder.pointer.project_out.weight.detach()
    u = sd["decoder.dynamic_embedding.projection.weight"].reshape(3, 128)
    dyn = fold_dynamic(sd["decoder.dynamic_embedding.projection.weight"], w_out)
    assert dyn.shape == (3, 128) and dyn.dtype == torch.float32
    assert torch.equal(dyn[0], u[0]) and torch.equal(dyn[1], u[1])
    heads = torch.randn(5, 128, dtype=torch.float64)
    # heads . (W_out^T u_l) == project_out(heads) . u_l (the folded vector is rounded to fp32 once)
    torch.testing.assert_close(heads @ dyn[2].double(), (heads @ w_out.double().t()) @ u[2].double(), rtol=1e-5, atol=1e-5)
    assert len(fold_weights("sdvrp", torch.randn(384, 128), w_out, torch.randn(128, 129))) == 4
    with pytest.raises(ValueError):  # the unfolded parity mode stays tsp / cvrp
        pol.decoder.precompute_cache(torch.randn(2, 21, 128), torch.float32, fold=False)
