"""rl4co_amd/envspec.py, the one table of per-environment facts, pinned against what it must agree with: the header's
environment ids, the argument structs' field names, the state the environments really produce, the rollout horizons and
what refuses the environments a kernel does not serve."""
import pathlib
import re

import pytest
import torch

from rl4co_amd import _lib, envspec, kernels, teacher
from tests import mtsp_ref, sdvrp_ref
from tests.fake_device import cpu_device  # noqa: F401

ENVS = ["tsp", "cvrp", "op", "pctsp", "pdp", "cvrptw", "sdvrp", "mtsp"]
DECODE_ONLY = ["sdvrp", "mtsp"]  # neither the one-launch replay nor the teacher-forced backward kernels
HEADER = pathlib.Path(__file__).resolve().parents[1] / "include" / "rl4co_amd.h"


def test_the_kernel_environments_and_the_alias():
    assert sorted(envspec.SPECS) == sorted(ENVS)
    assert all(envspec.SPECS[name].name == name for name in ENVS)
    assert envspec.spec("spctsp") is envspec.SPECS["pctsp"]
    assert all(envspec.spec(name) is envspec.SPECS[name] for name in ENVS)  # one table, one lookup
    with pytest.raises(AttributeError):  # frozen records
        envspec.spec("tsp").env_id = 7


def test_env_ids_are_the_headers():
    header = dict(re.findall(r"#define RL4CO_ENV_(\w+) (\d+)", HEADER.read_text()))
    assert sorted(header) == sorted(name.upper() for name in ENVS)
    for name in ENVS:
        assert envspec.spec(name).env_id == int(header[name.upper()]) == getattr(_lib, f"ENV_{name.upper()}")
    assert sorted(envspec.spec(name).env_id for name in ENVS) == list(range(len(ENVS)))
    assert kernels.ENV_IDS == {name: envspec.spec(name).env_id for name in ENVS}


def test_capability_fields():
    """What serves an environment, and the facts the bindings branch on, are fields of its record."""
    served = lambda field: sorted(name for name in ENVS if getattr(envspec.spec(name), field))  # noqa: E731
    assert served("unfold") == ["cvrp", "tsp"]
    assert served("replay") == served("teacher") == sorted(set(ENVS) - set(DECODE_ONLY))
    assert teacher.TEACHER_ENVS == ("tsp", "cvrp", "op", "pctsp", "pdp", "cvrptw")
    assert served("ctx_first") == served("fixed_horizon") == ["tsp"]
    assert served("length_reward") == ["cvrp", "cvrptw", "pdp", "sdvrp", "tsp"]
    assert served("state_reward") == served("feats") == ["mtsp"] and served("dynamic") == ["sdvrp"]
    assert served("depot_flag") == ["pdp"] and envspec.spec("pdp").depot_flag == "force_start_at_depot"
    assert {name: envspec.spec(name).init for name in ENVS} == {
        "tsp": "all", "pdp": "pairs", "cvrp": "depot", "op": "depot", "pctsp": "depot", "cvrptw": "depot", "sdvrp": "depot",
        "mtsp": "depot"}
    assert {name: envspec.spec(name).feature_width for name in ENVS} == {
        "tsp": 0, "pdp": 0, "cvrp": 1, "op": 1, "pctsp": 2, "cvrptw": 4, "sdvrp": 1, "mtsp": 0}
    assert envspec.spec("sdvrp").dynamic == ("demand_with_depot", "projection", "dyn_vectors")
    assert envspec.spec("sdvrp").dynamic.slot in {f[0] for f in _lib.AmDecodeArgs._fields_}
    for name in ENVS:
        sp = envspec.spec(name)
        assert sp.teacher == (sp.no_teacher is None) and (sp.teacher or "not in the backward kernels" in sp.no_teacher)
        assert not (sp.state_reward and sp.length_reward) and not (sp.ctx_first and (sp.scalar or sp.feats))


@pytest.mark.parametrize("env_name", ENVS)
def test_every_slot_is_a_field_of_the_argument_structs(env_name):
    sp = envspec.spec(env_name)
    decode = {f[0] for f in _lib.AmDecodeArgs._fields_}
    replay = {f[0] for f in _lib.EnvReplayArgs._fields_}
    back = {f[0] for f in teacher.AmTeacherArgs._fields_}
    running = sp.scalar.running if sp.scalar is not None else None
    assert (sp.replay, sp.teacher) == ((env_name not in DECODE_ONLY),) * 2
    for f in sp.fields:
        assert f.kind in ("traj", "inst") and f.dtype in ("i64", "f32", "u8")
        assert f.slot in decode, f
        if sp.replay:
            assert ("scalar" if f.key == running else f.slot) in replay, f  # (the replay keeps the running scalar in one slot)
        if sp.teacher and f.key in sp.teacher_keys:
            assert f.slot in back, f
    slots = [f.slot for f in sp.fields]
    assert len(set(slots)) == len(slots), "two state tensors in one slot"
    if sp.scalar is not None:
        assert sp.scalar.running in sp.keys("traj") and sp.scalar.base in sp.keys()
        assert sp.scalar.base_col0 == (sp.scalar.base in sp.keys("inst"))
        assert sp.scalar.clock is None or sp.scalar.clock in sp.keys("traj")
    entry, keys = sp.step
    assert callable(getattr(kernels, entry)) and set(keys) <= set(sp.keys())


@pytest.mark.parametrize("env_name", DECODE_ONLY)
def test_what_does_not_serve_an_environment_refuses_it(env_name):
    """On the host, before any device access: the one-launch replay and the teacher-forced backward kernels."""
    with pytest.raises(NotImplementedError, match="one-launch replay"):
        kernels.env_replay(env_name, {}, None, None)
    assert not teacher.supports(env_name, torch.float32, 20) and teacher.supports("cvrp", torch.float32, 20)
    with pytest.raises(NotImplementedError, match="teacher-forced backward kernels serve tsp, cvrp, op, pctsp, pdp, cvrptw, not"):
        teacher._require_served(env_name)
    teacher._require_served("cvrptw")


@pytest.mark.parametrize("env_name", ENVS)
def test_reset_yields_the_tables_state_and_initial_state_lays_it_out(cpu_device, monkeypatch, env_name):
    from rl4co_amd.envs import get_env
    from rl4co_amd.policy import AttentionModelPolicy

    monkeypatch.setattr(kernels, "sdvrp_step", sdvrp_ref.step)  # (the test plays the device: the restatements)
    monkeypatch.setattr(kernels, "mtsp_step", mtsp_ref.step)
    sp = envspec.spec(env_name)
    b = 4
    env = get_env(env_name, generator_params=dict(num_loc=6), device=cpu_device)
    torch.manual_seed(3)
    td = env.reset(batch_size=[b])
    n = td["action_mask"].shape[-1]
    # (mTSP's num_loc counts the depot: mtsp/generator.py)
    assert n == (6 if env_name in ("tsp", "mtsp") else 7) and sp.has_depot == env.has_depot == (env_name != "tsp")
    for key in sp.keys() + sp.passthrough + tuple(key for key, _, _ in sp.features):
        assert key in td.keys(), key
    if env_name == "sdvrp":
        assert sp.keys("inst") == ()  # no instance data: every state tensor is per trajectory
    policy = AttentionModelPolicy(env_name)
    dtypes = {"i64": (torch.int64,), "f32": (torch.float32,), "u8": (torch.bool, torch.uint8)}
    for starts in (0, 3):
        rows = b * max(starts, 1)
        state = policy._initial_state(td, starts)
        assert sorted(state) == sorted(sp.keys())
        for f in sp.fields:
            t = state[f.key]
            assert t.dtype in dtypes[f.dtype] and t.is_contiguous(), f
            if f.kind == "traj":
                assert t.shape == ((rows, n) if f.shape == "BN" else (rows,)), f
                assert t.data_ptr() != td[f.key].data_ptr(), f  # own storage: the kernels write it
                src = td[f.key] if f.shape == "BN" else td[f.key].reshape(-1)
                assert torch.equal(t.view(max(starts, 1), b, *t.shape[1:]), src.expand(max(starts, 1), *src.shape)), f  # s-major
            else:
                assert t.shape[0] == b and t.shape[1:] == {"N-1": (n - 1,), "N": (n,), "N2": (n, 2), "": ()}[f.shape], f
                if td[f.key].dtype == torch.float32 or f.shape == "":
                    assert t.data_ptr() == td[f.key].data_ptr(), f  # shared with the caller, not a copy
        final = policy._final_td(td, state, starts)
        assert sorted(final.keys()) == sorted(sp.passthrough + sp.keys("traj"))
        for f in sp.fields:
            if f.kind == "traj":
                assert final[f.key].shape == ((rows, 1) if f.shape == "B1" else state[f.key].shape), f
                assert final[f.key].data_ptr() == state[f.key].data_ptr(), f


def test_horizons():
    expected = {  # n (nodes, depot included) -> longest rollout
        "tsp": {2: 2, 20: 20, 100: 100},
        "pctsp": {2: 2, 20: 20, 100: 100},
        "pdp": {2: 2, 20: 20, 100: 100},
        "op": {2: 4, 20: 22, 100: 102},
        "cvrp": {2: 4, 20: 40, 100: 200},
        "cvrptw": {2: 4, 20: 40, 100: 200},
        "sdvrp": {21: 126},
        "mtsp": {20: 40},
    }
    from rl4co_amd.policy import AttentionModelPolicy

    assert sorted(expected) == sorted(ENVS)
    for name, table in expected.items():
        for n, horizon in table.items():
            assert envspec.spec(name).horizon(n) == horizon == AttentionModelPolicy._max_horizon(name, n)
