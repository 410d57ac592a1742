"""Multi-agent TSP (min-max) without a GPU: the environment and the torch-fp32 restatement against the recorded reference
states, the closed form of the reference's padding quirk against the recorded rewards, how many recorded greedy trajectories
sit at a near-tie, the generator's stream, and the envspec record behind the kernel bindings."""
import pathlib
import re

import pytest
import torch

from rl4co_amd import _lib, envspec
from rl4co_amd import kernels as K
from rl4co_amd.tensordict import TensorDict
from tests import mtsp_ref
from tests.fake_device import cpu_device  # noqa: F401

GREEDY = ["mtsp20_greedy", "mtsp50_greedy"]
ALL = list(mtsp_ref.CASES)


@pytest.fixture
def mtsp_cpu(cpu_device, monkeypatch):  # noqa: F811
    """The test plays the device: the step entry is the restatement (itself pinned to the record below)."""
    monkeypatch.setattr(K, "mtsp_step", mtsp_ref.step)
    return cpu_device


def _reset(rec, device, **kw):
    from rl4co_amd.envs import get_env

    num_loc = rec["in_locs"].shape[1]
    env = get_env("mtsp", generator_params=dict(num_loc=num_loc), device=device, **kw)
    data = TensorDict({k[3:]: v.clone() for k, v in rec.items() if k.startswith("in_")}, batch_size=[rec["in_locs"].shape[0]])
    return env, env.reset(data)


def _unpack(bits, n):
    return ((bits[..., None].to(torch.int32) >> torch.arange(8)) & 1).flatten(-2)[..., :n].to(torch.uint8)


@pytest.mark.parametrize("case", GREEDY)
def test_restatement_and_env_equal_the_recorded_reference_states(mtsp_cpu, case):
    rec = mtsp_ref.record(case)
    env, td = _reset(rec, mtsp_cpu)
    assert env.name == "mtsp" and env.has_depot
    st = mtsp_ref.initial_state(rec["in_locs"], rec["in_num_agents"])
    acts = rec["actions"]
    n = acts.new_tensor(rec["in_locs"].shape[1]).item()
    masks = _unpack(rec["states_mask_bits"], n)
    rows = mtsp_ref.STATE_ROWS
    for t in range(acts.shape[1] + 1):
        for state in (st, td):
            assert torch.equal(state["action_mask"].to(torch.uint8), masks[:, t]), t
            assert torch.equal(state["done"].reshape(-1).to(torch.uint8), rec["states_done"][:, t]), t
            assert torch.equal(state["agent_idx"].to(torch.uint8), rec["states_agent"][:, t]), t
            assert torch.equal(state["current_node"].reshape(-1).to(torch.uint8), rec["states_node"][:, t]), t
            assert torch.equal(state["current_length"][:rows], rec["states_length"][:, t]), t  # bit for bit
            assert torch.equal(state["max_subtour_length"][:rows], rec["states_max"][:, t]), t
        if t < acts.shape[1]:
            mtsp_ref.step_state(st, acts[:, t])
            td.set("action", acts[:, t].clone())
            td = env.step(td)["next"]
    # ... every row's reward (the state after the batch's padding steps)
    assert torch.equal(-st["max_subtour_length"], rec["reward"])
    assert torch.equal(env.get_reward(td, acts), rec["reward"])
    assert torch.equal(td["i"], torch.full_like(td["i"], acts.shape[1])) and torch.equal(td["first_node"], acts[:, 0])
    assert bool(td["done"].all())
    assert int((rec["in_num_agents"] == 1).sum()) > 0 or case != "mtsp20_greedy"  # one agent: the depot is never offered


@pytest.mark.parametrize("case", ALL)
def test_closed_form_padding_rule_equals_the_recorded_rewards(case):
    """A rollout kernel stops a row at its done; the reference pads it with depot steps and the first one moves the reward."""
    rec = mtsp_ref.record(case)
    acts = rec["actions"]
    st = mtsp_ref.initial_state(rec["in_locs"], rec["in_num_agents"])
    length_at_done = torch.zeros(acts.shape[0])
    for t in range(acts.shape[1]):
        was_done = st["done"].clone()
        # (current_length AT done, before the agent change of a later step: the finishing action is a customer)
        mtsp_ref.step_state(st, acts[:, t], freeze_done=True)
        length_at_done = torch.where(st["done"] & ~was_done, st["current_length"], length_at_done)
    assert bool(st["done"].all())
    own = mtsp_ref.row_lengths(acts)
    assert int(own.max()) == acts.shape[1] and bool((acts[torch.arange(len(own)), own - 1] != 0).all())
    want = mtsp_ref.padded_reward(rec["in_locs"], acts, st["max_subtour_length"], length_at_done)
    assert torch.equal(want, rec["reward"])
    padded = own < acts.shape[1]
    moved = (-st["max_subtour_length"] != rec["reward"]) & padded
    print(f"{case}: {int(padded.sum())} padded rows, {int(moved.sum())} changed reward")
    assert int(moved.sum()) > 0  # the quirk is what these records exercise
    # horizon: n - 1 customer visits and at most one depot visit after each but the last
    n = rec["in_locs"].shape[1]
    assert acts.shape[1] <= 2 * (n - 1) < envspec.spec("mtsp").horizon(n)


@pytest.mark.parametrize("case", GREEDY)
def test_fragile_share_of_the_record(case):
    """A trajectory is fragile if, at some step, the reference's own best and second-best log-prob are closer than twice the
    per-step tolerance of the teacher-forced comparison: there a kernel may legitimately take the other node."""
    rec = mtsp_ref.record(case)
    fragile = rec["min_gap"] < 2 * mtsp_ref.STEP_TOL
    print(f"{case}: {int(fragile.sum())} of {fragile.numel()} trajectories fragile, smallest gap {float(rec['min_gap'].min()):.3e}")
    assert mtsp_ref.STEP_TOL <= 2e-5 and mtsp_ref.STEP_TOL == 4 * mtsp_ref.MEASURED_STEP_DEV
    assert int(fragile.sum()) * 4 <= fragile.numel()


def test_reset_keys_and_dtypes_equal_the_records(mtsp_cpu):
    rec = mtsp_ref.record("mtsp20_greedy")
    env, td = _reset(rec, mtsp_cpu)
    want = sorted([k[6:] for k in rec if k.startswith("reset_") and k != "reset_dtype_codes"] + ["locs", "num_agents"])
    assert sorted(td.keys()) == want
    codes = rec["reset_dtype_codes"].tolist()
    for key, code in zip(want, codes):
        assert td[key].dtype == mtsp_ref.RESET_DTYPES[code], key
        if key not in ("locs", "num_agents"):
            got = td[key].to(torch.uint8) if td[key].dtype == torch.bool else td[key]
            assert got.shape == rec[f"reset_{key}"].shape and torch.equal(got, rec[f"reset_{key}"]), key
    with pytest.raises(NotImplementedError, match="cost_type"):
        _reset(rec, mtsp_cpu, cost_type="sum")
    with pytest.raises(ValueError):
        _reset(rec, mtsp_cpu, cost_type="median")


@pytest.mark.parametrize("case", ["mtsp20_greedy", "mtsp50_greedy"])
def test_generator_follows_the_reference_stream(case):
    from rl4co_amd.envs import MTSPGenerator

    num_loc, batch, _, lo, hi, seed = mtsp_ref.CASES[case]
    rec = mtsp_ref.record(case)
    torch.manual_seed(seed)
    data = MTSPGenerator(num_loc=num_loc, min_num_agents=lo, max_num_agents=hi)(batch_size=[batch])
    assert torch.equal(data["locs"], rec["in_locs"])
    assert data["num_agents"].dtype == torch.int64 and torch.equal(data["num_agents"], rec["in_num_agents"])
    assert int(rec["in_num_agents"].min()) == lo and int(rec["in_num_agents"].max()) == hi
    default = MTSPGenerator()
    assert (default.num_loc, default.min_num_agents, default.max_num_agents) == (20, 5, 5)


def test_envspec_record_and_binding(mtsp_cpu, monkeypatch):
    from rl4co_amd.policy import AttentionModelPolicy

    sp = envspec.spec("mtsp")
    assert sp is envspec.SPECS["mtsp"] and sp.env_id == _lib.ENV_MTSP == 7 and sp.has_depot
    # ... and the header's value, a plain integer like the other ids
    header = (pathlib.Path(__file__).resolve().parents[1] / "include" / "rl4co_amd.h").read_text()
    ids = {k: int(v) for k, v in re.findall(r"#define (RL4CO_ENV_\w+) (\d+)\b", header)}
    assert ids["RL4CO_ENV_MTSP"] == sp.env_id == 7 and list(ids.values()).count(7) == 1
    assert ids["RL4CO_ENV_SDVRP"] != sp.env_id
    # the decode kernels alone serve it, one trajectory per instance: the reward is carried in the state
    assert not sp.unfold and not sp.replay and not sp.teacher and "four-scalar context" in sp.no_teacher
    assert sp.state_reward and not sp.length_reward and not sp.fixed_horizon and not sp.ctx_first and sp.dynamic is None
    assert sp.init == "depot" and sp.feature_width == 0
    assert sp.horizon(20) == 40 == AttentionModelPolicy._max_horizon("mtsp", 20)
    assert sp.scalar is None and sp.features == () and sp.passthrough == ("locs", "num_agents")
    assert sp.feats.names == ("remaining_agents", "current_length", "max_subtour_length", "depot_distance")
    assert callable(getattr(K, sp.step[0])) and set(sp.step[1]) <= set(sp.keys())
    decode = {f[0] for f in _lib.AmDecodeArgs._fields_}
    assert all(f.slot in decode for f in sp.fields) and len({f.slot for f in sp.fields}) == len(sp.fields)
    names = [f[0] for f in _lib.AmDecodeArgs._fields_]
    # behind the outputs, in front of the context-table strides and the filter (whose place at the tail existing tests pin)
    assert names.index("mtsp_ctx") == names.index("err") + 1 and names.index("num_agents") == names.index("mtsp_ctx") + 1
    assert names.index("ctx_dtype") == names.index("num_agents") + 1

    rec = mtsp_ref.record("mtsp20_greedy")
    env, td = _reset(rec, mtsp_cpu)
    for key in sp.keys() + sp.passthrough:
        assert key in td.keys(), key
    policy = AttentionModelPolicy("mtsp")
    monkeypatch.setattr(K, "_dev", lambda t, dtype=None, name="tensor": t)
    monkeypatch.setattr(K, "_u8", lambda t, name: t.view(torch.uint8) if t.dtype == torch.bool else t)
    state = policy._initial_state(td, 0)
    assert sorted(state) == sorted(sp.keys())
    a = _lib.AmDecodeArgs()
    assert K.bind_env_state(a, sp, state, 64, 20) == 64
    for f in sp.fields:
        assert getattr(a, f.slot) == state[f.key].data_ptr(), f
        if f.kind == "traj":
            assert state[f.key].data_ptr() != td[f.key].data_ptr(), f  # own storage: the kernels write it
            assert state[f.key].shape == ((64, 20) if f.shape == "BN" else (64,)), f
    assert state["num_agents"].dtype == torch.int64 and a.visited is None and a.demand is None
    final = policy._final_td(td, state, 0)
    assert sorted(final.keys()) == sorted(set(sp.passthrough + sp.keys("traj")))
    assert final["done"].shape == (64, 1)
    short = dict(state, action_mask=state["action_mask"][:, :19].contiguous())
    with pytest.raises(ValueError):
        K.bind_env_state(_lib.AmDecodeArgs(), sp, short, 64, 20)
    with pytest.raises(ValueError):
        K.bind_env_state(_lib.AmDecodeArgs(), sp, dict(state, num_agents=state["num_agents"][:, None].contiguous()), 64, 20)


def test_stepwise_replay_tabulates_the_four_scalars(mtsp_cpu):
    rec = mtsp_ref.record("mtsp20_greedy")
    st = mtsp_ref.initial_state(rec["in_locs"], rec["in_num_agents"])
    r = K.env_replay_stepwise("mtsp", {k: v.clone() for k, v in st.items()}, rec["actions"], None,
                              err=torch.zeros(1, dtype=torch.int32))
    assert r["feats"].shape == (64, rec["actions"].shape[1], 4)
    want = mtsp_ref.initial_state(rec["in_locs"], rec["in_num_agents"])
    for t in range(rec["actions"].shape[1]):
        assert torch.equal(r["feats"][:, t], mtsp_ref.features(want)), t
        assert torch.equal(r["masks"][:, t], want["action_mask"]) and torch.equal(r["prev"][:, t], want["current_node"])
        mtsp_ref.step_state(want, rec["actions"][:, t])
    assert torch.equal(r["feats"][:, 0], torch.stack((rec["in_num_agents"].float(), *[torch.zeros(64)] * 3), -1))


def test_policy_module_tree_and_fold():
    """The modules carry the reference's names; the four-scalar context folds to one [4, 128] table."""
    from rl4co_amd.cache import fold_features, fold_weights
    from rl4co_amd.policy import AttentionModelPolicy

    torch.manual_seed(0)
    pol = AttentionModelPolicy("mtsp")
    sd = pol.state_dict()
    assert tuple(sd["encoder.init_embedding.init_embed.weight"].shape) == (128, 2)
    assert tuple(sd["encoder.init_embedding.init_embed_depot.weight"].shape) == (128, 2)
    assert tuple(sd["decoder.context_embedding.project_context.weight"].shape) == (128, 256)
    assert tuple(sd["decoder.context_embedding.proj_dynamic_feats.weight"].shape) == (128, 4)
    assert not any("bias" in k for k in sd if "context_embedding" in k) and not any("dynamic_embedding" in k for k in sd)
    w_ctx, w_dyn = sd["decoder.context_embedding.project_context.weight"], sd["decoder.context_embedding.proj_dynamic_feats.weight"]
    g = fold_features(w_ctx, w_dyn)
    assert g.shape == (4, 128) and g.dtype == torch.float32 and g.is_contiguous()
    f = torch.rand(5, 4, dtype=torch.float64) * 3
    h = torch.randn(5, 128, dtype=torch.float64)
    want = torch.cat((h, f @ w_dyn.double().t()), -1) @ w_ctx.double().t()
    torch.testing.assert_close(h @ w_ctx.double()[:, :128].t() + f @ g.double(), want, rtol=1e-6, atol=1e-6)
    assert len(fold_weights("mtsp", torch.randn(384, 128), torch.randn(128, 128), w_ctx)) == 4
    with pytest.raises(ValueError):  # the unfolded parity mode stays tsp / cvrp
        pol.decoder.precompute_cache(torch.randn(2, 20, 128), torch.float32, fold=False)
    with torch.no_grad():
        cache = pol.decoder.precompute_cache(torch.randn(2, 20, 128), torch.float32)
    assert torch.equal(cache.feat, g) and cache.w_cap is None and cache.w_time is None and cache.dyn is None
