"""Ant System (OP, PCTSP) without a device: the restatement (tests/aco_prize_ref.py) against the records of the reference's
own AntSystem with its OPEnv / PCTSPEnv under recorded noise (actions, masks, lengths, log-probs, the W-wide reward, update,
the ragged record), the C boundary of rl4co_aco_prize (header == ctypes table, the LDS tier formula, argument refusals) and
the host class's refusals on the new path. Every call of the entry here is refused before a launch."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from rl4co_amd import _lib
from tests import aco_prize_ref as R

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "rl4co_amd.h").read_text()
ERR_ARG = 1
DUMMY = 0x10000  # non-null, never followed
C_TYPES = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64}
RECORDS = [(env, case) for env in R.ENVS for case in R.CASES]


def test_constants_are_the_records():
    for env, case in RECORDS:
        rec = R.record(env, case)
        assert float(rec["noise_floor"]) <= R.NOISE_FLOORS[f"{env}_{case}"] <= R.MEASURED_NOISE_FLOOR
        assert float(rec["noise_floor"]) > 0.99 * R.NOISE_FLOORS[f"{env}_{case}"]
        assert float(rec["reward_ulps"]) == R.REWARD_ULPS_BY_RECORD[f"{env}_{case}"] <= R.REWARD_ULPS
    assert R.STEP_TOL == 4 * max(R.NOISE_FLOORS.values()) and R.REWARD_ULPS == max(R.REWARD_ULPS_BY_RECORD.values())


@pytest.mark.parametrize("env,case", RECORDS)
def test_restatement_follows_the_reference_record(env, case):
    """Under the recorded noise: the reference's actions, masks and lengths bit for bit, its log-probs within STEP_TOL, its
    W-wide reward within REWARD_ULPS of its reward; the update on its reward gives its pheromone, final_reward and ragged
    final_actions bit for bit after every iteration."""
    rec = R.record(env, case)
    c, ants, b, iters, alpha, beta, decay, phe0, _ = R.CASES[case]
    w, data = R.width(c + 1), R.record_data(env, rec)
    assert bool((rec["pheromone0"] == (1 if phe0 is None else phe0)).all())
    state = R.fresh_state(rec["pheromone0"])
    worst = 0.0
    for i in range(iters):
        ref_actions = rec[f"actions_{i}"]
        t_i = ref_actions.shape[1]
        assert ref_actions.shape == (ants * b, int(rec["lengths"][i].max()))  # the reference trims to its longest row
        actions, lengths, logps, _, masks = R.sample(env, state["pheromone"], rec["log_heuristic"], data, rec["ln_noise"][i],
                                                     alpha, beta)
        assert torch.equal(lengths, rec["lengths"][i])
        assert torch.equal(actions[:, :t_i], ref_actions) and bool((actions[:, t_i:] == 0).all())
        steps = torch.arange(w)[None, :] < lengths[:, None]
        assert bool((actions[~steps] == 0).all()) and bool((logps[~steps] == 0).all())  # trailing zeros, log-prob 0
        taken = steps[:, :t_i]
        assert torch.equal(masks[:, :t_i][taken], rec[f"masks_{i}"][taken])
        assert bool((rec[f"logps_{i}"][~taken] == 0).all())  # the reference's padding steps: one feasible node
        assert float((logps[:, :t_i] - rec[f"logps_{i}"]).abs().max()) <= R.STEP_TOL
        assert float((logps[:, :t_i].double() - rec[f"logps64_{i}"]).abs().max()) <= R.STEP_TOL
        forced = R.sample(env, state["pheromone"], rec["log_heuristic"], data, None, alpha, beta, forced=actions)
        assert torch.equal(forced[0], actions) and torch.equal(forced[1], lengths) and torch.equal(forced[2], logps)
        # the reward: the reference's own row bit for bit, the W-wide row within the measured ulps
        assert torch.equal(R.reward_w(env, data, ref_actions), rec["reward"][i])
        reward = R.reward_w(env, data, actions)
        worst = max(worst, float(R.ulps(reward, rec["reward"][i], R.reward_scale(env, data, actions)).max()))
        # the update on the reference's reward (the W-wide reward moves the reward map by those ulps): bit for bit
        # (every row ends at the depot, so the W-wide rows deposit what the reference's trimmed rows deposit)
        R.update(state, actions, rec["reward"][i], decay, float(rec["Q"]), keep=t_i)
        assert bool((ref_actions[torch.arange(ants * b), rec["lengths"][i].long() - 1] == 0).all())
        assert torch.equal(state["pheromone"], rec["pheromone"][i])
        assert torch.equal(state["final_reward"], rec["final_reward"][i])
        want = R.record_finals(rec, i)
        assert all(torch.equal(x, y) for x, y in zip(state["final_actions"], want)) and len(want) == b
    print(f"{env} {case}: reward_w against the recorded reward {worst} ulps (bound {R.REWARD_ULPS})")
    assert worst <= R.REWARD_ULPS
    assert not torch.equal(rec["pheromone"][0], rec["pheromone"][-1])


@pytest.mark.parametrize("case", list(R.CASES))
def test_records_cover_the_cases_the_seeds_were_chosen_for(case):
    assert R.coverage("op", R.record("op", case), case)["early"] >= 1  # a row that ends early on budget
    cov = R.coverage("pctsp", R.record("pctsp", case), case)
    assert bool(cov["short"].any()) and bool(cov["full"].any())


def test_restated_edge_regimes():
    n, b, ants = 6, 2, 3
    phe, heu = torch.ones(b, n, n), torch.zeros(b, n, n)
    noise = R.ln_exp1((n, ants * b, n), seed=1)
    tight = R.random_data("op", b, n, 5, budget=0.0)  # nothing but the depot can be entered
    actions, lengths, logps, _, _ = R.sample("op", phe, heu, tight, noise)
    assert bool((actions == 0).all()) and lengths.tolist() == [2] * (ants * b) and bool((logps == 0).all())
    assert bool((R.reward_w("op", tight, actions) == 0).all())
    poor = R.random_data("pctsp", b, n, 6, prize_scale=0.5)  # total prize < 1: every customer has to be visited
    assert float(poor["prize"].sum(-1).max()) < 1
    actions, lengths, _, _, _ = R.sample("pctsp", phe, heu, poor, noise)
    assert lengths.tolist() == [n] * (ants * b) and bool((actions[:, -1] == 0).all())
    assert all(sorted(row.tolist()) == list(range(n)) for row in actions)
    rich = R.random_data("pctsp", b, n, 7)
    rich["prize"][:, 3] = 1.5  # after customer 3 the depot is feasible
    actions, lengths, _, _, masks = R.sample("pctsp", phe, heu, rich, noise)
    for r in range(ants * b):
        row = actions[r, : int(lengths[r])].tolist()
        for t in range(int(lengths[r])):
            assert bool(masks[r, t, 0]) == (3 not in row[:t] and float(rich["prize"][r % b][row[:t]].sum()) < 1 and t < n - 1)


# ---- the C boundary --------------------------------------------------------------------------------------------------------
def _struct_fields():
    body = re.search(r"typedef struct rl4co_aco_prize_args \{(.*?)\} rl4co_aco_prize_args;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"([\w ]+?)(\*?)\s*(\w+)\s*;", body)


def test_header_ctypes_and_symbols_agree():
    decls = _struct_fields()
    assert [d[2] for d in decls] == [f[0] for f in _lib.AcoPrizeArgs._fields_]
    for (ctype, star, name), (_, mirror) in zip(decls, _lib.AcoPrizeArgs._fields_):
        assert mirror is (ctypes.c_void_p if star else C_TYPES[ctype.strip()]), name
    assert ctypes.sizeof(_lib.AcoPrizeArgs) == 16 * 4 + 2 * 8 + 23 * 8
    assert "int rl4co_aco_prize(const rl4co_aco_prize_args* args, void* stream);" in HEADER
    assert "int rl4co_aco_prize_lds_nodes(int env);" in HEADER
    restype, argtypes = _lib.SYMBOLS["rl4co_aco_prize"]
    assert restype is ctypes.c_int and argtypes == [ctypes.POINTER(_lib.AcoPrizeArgs), ctypes.c_void_p]
    assert _lib.SYMBOLS["rl4co_aco_prize_lds_nodes"] == (ctypes.c_int, [ctypes.c_int])
    assert int(re.search(r"#define RL4CO_ABI_VERSION (\d+)", HEADER).group(1)) >= 22
    assert _lib.ABI_VERSION >= 22 and _lib.lib().rl4co_abi_version() == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.AcoCvrpArgs) == 14 * 4 + 2 * 8 + 23 * 8  # the existing structs keep their sizes
    assert ctypes.sizeof(_lib.AcoTspArgs) == 12 * 4 + 2 * 8 + 18 * 8


def test_struct_layout_is_the_compilers(tmp_path):
    import shutil
    import subprocess

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "rl4co_amd.h"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(rl4co_aco_prize_args));']
    lines += [f'  printf("{f} %zu\\n", offsetof(rl4co_aco_prize_args, {f}));' for f, _ in _lib.AcoPrizeArgs._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    table = dict(row.split() for row in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(table["sizeof"]) == ctypes.sizeof(_lib.AcoPrizeArgs)
    for f, _ in _lib.AcoPrizeArgs._fields_:
        assert int(table[f]) == getattr(_lib.AcoPrizeArgs, f).offset, f


def _args(**over):
    """Valid scalars, every pointer of a fused OP launch set."""
    a = _lib.AcoPrizeArgs()
    a.B, a.N, a.n_ants, a.iterations, a.phases, a.has_best, a.T, a.env = 4, 21, 8, 3, 3, 0, 21, _lib.ENV_OP
    a.alpha, a.beta, a.decay, a.Q, a.temperature = 1.0, 1.0, 0.95, 0.1, 1.0
    for f in ("log_heuristic", "pheromone", "locs", "prize", "penalty", "max_length", "actions", "lengths", "reward", "logps",
              "final_reward", "final_actions", "final_iteration", "err"):
        setattr(a, f, DUMMY)
    for k, v in over.items():
        setattr(a, k, v)
    return a


REFUSALS = [
    (dict(env=_lib.ENV_TSP), b"a.env == RL4CO_ENV_OP || a.env == RL4CO_ENV_PCTSP"),
    (dict(env=_lib.ENV_CVRP), b"a.env == RL4CO_ENV_OP || a.env == RL4CO_ENV_PCTSP"),
    (dict(B=0), b"a.B >= 1"),
    (dict(N=1), b"a.N >= 2"),
    (dict(N=1025), b"a.N <= 1024"),
    (dict(n_ants=0), b"a.n_ants >= 1"),
    (dict(iterations=0), b"a.iterations >= 1"),
    (dict(phases=0), b"a.phases >= 1"),
    (dict(phases=4), b"a.phases <= (RL4CO_ACO_SAMPLE | RL4CO_ACO_UPDATE)"),
    (dict(phases=1, iterations=2), b"(sample && update) || a.iterations == 1"),
    (dict(locs=None), b"a.locs != nullptr"),
    (dict(n_workgroups=-1), b"a.n_workgroups >= 0"),
    (dict(n_workgroups=5), b"a.n_workgroups <= a.B"),
    (dict(T=20), b"a.T == a.N"),
    (dict(phases=2, iterations=1, T=1), b"a.T >= 2"),
    (dict(temperature=0.0), b"a.temperature > 0.0f"),
    (dict(log_heuristic=None), b"a.log_heuristic != nullptr"),
    (dict(prize=None), b"a.prize != nullptr"),
    (dict(max_length=None), b"a.max_length != nullptr"),
    (dict(env=_lib.ENV_PCTSP, penalty=None), b"a.penalty != nullptr"),
    (dict(lengths=None), b"a.lengths != nullptr"),
    (dict(forced_actions=DUMMY), b"a.forced_actions == nullptr"),  # iterations = 3
    (dict(pheromone=None), b"a.pheromone != nullptr"),
    (dict(actions=None), b"a.actions != nullptr"),
    (dict(reward=None), b"a.reward != nullptr"),
    (dict(final_reward=None), b"a.final_reward != nullptr"),
    (dict(err=None), b"a.err != nullptr"),
    (dict(N=142, T=142), b"lds || a.logits_scratch != nullptr"),
    (dict(env=_lib.ENV_PCTSP, N=142, T=142), b"lds || a.logits_scratch != nullptr"),
]


@pytest.mark.parametrize("over,text", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o, _ in REFUSALS])
def test_argument_refusals(over, text):
    assert _lib.lib().rl4co_aco_prize(ctypes.byref(_args(**over)), None) == ERR_ARG
    msg = _lib.lib().rl4co_last_error()
    assert b"requirement failed" in msg and text in msg, msg
    assert _lib.lib().rl4co_aco_prize(None, None) == ERR_ARG and b"args != nullptr" in _lib.lib().rl4co_last_error()


def test_lds_nodes_is_the_headers_formula():
    """8 n^2 (logits + pheromone) + 8 roundup(W + 1, 8) (wave tours) + 4 V roundup(n, 4) (per-node vectors, OP V = 3,
    PCTSP V = 2) + 256 + 64 <= 160 KiB"""
    def fits(n, v):
        return 8 * n * n + 8 * ((R.width(n) + 1 + 7) // 8 * 8) + 4 * v * ((n + 3) // 4 * 4) + 256 + 64 <= 160 * 1024

    for env, v in ((_lib.ENV_OP, 3), (_lib.ENV_PCTSP, 2)):
        want = max(n for n in range(2, 1025) if fits(n, v))
        assert _lib.lib().rl4co_aco_prize_lds_nodes(env) == want == 141
    assert _lib.lib().rl4co_aco_prize_lds_nodes(_lib.ENV_TSP) == -1
    text = (ROOT / "rl4co_amd" / "csrc" / "aco_prize.hip").read_text()
    assert "8 N^2 + 8 roundup(W + 1, 8) + 4 V roundup(N, 4) + 256 + 64 <= 160 KiB" in text and "N <= 141" in text


# ---- the host class ----------------------------------------------------------------------------------------------------------
class _Env:
    def __init__(self, name):
        self.name = name


MS = dict(multisample=True, num_samples=5, select_best=False)


def _system(env="op", **kw):
    from rl4co_amd import AntSystem

    rec = R.record(env, "c10_a5")
    return AntSystem(rec["log_heuristic"], n_ants=5, **kw), {"locs": rec["locs"]}  # (no prize: refused before it is read)


@pytest.mark.parametrize("name", ["op", "pctsp", "spctsp"])
def test_host_refusals_on_the_prize_path(name):
    aco, td = _system("op" if name == "op" else "pctsp")
    env = _Env(name)
    with pytest.raises(NotImplementedError, match=f"rl4co_aco_prize.*{name}"):  # CPU tensors; a td without prize: no KeyError
        aco.run(td, env, 2, MS)
    with pytest.raises(NotImplementedError, match=f"rl4co_aco_prize.*{name}"):
        aco._one_step(td, env, MS)
    with pytest.raises(NotImplementedError, match="use_local_search"):
        _system(use_local_search=True)[0].run(td, env, 2, MS)
    with pytest.raises(NotImplementedError, match="multistart"):
        aco.run(td, env, 2, dict(multistart=True, num_starts=5, select_best=False))
    with pytest.raises(NotImplementedError, match="multistart"):
        aco.run(td, env, 2, dict(MS, multistart=True))
    with pytest.raises(NotImplementedError, match="multisample"):
        aco.run(td, env, 2, dict(select_best=False))
    with pytest.raises(NotImplementedError, match="num_samples"):
        aco.run(td, env, 2, dict(MS, num_samples=7))
    for key, value in (("top_k", 5), ("top_p", 0.9), ("tanh_clipping", 10.0), ("num_starts", 5)):
        with pytest.raises(NotImplementedError, match=key):
            aco.run(td, env, 2, dict(MS, **{key: value}))
    with pytest.raises(NotImplementedError, match="select_best"):
        aco.run(td, env, 2, dict(MS, select_best=True))
    with pytest.raises(NotImplementedError, match="pdp"):
        aco.run(td, _Env("pdp"), 2, MS)


def test_binding_refuses_cpu_tensors_and_other_environments():
    from rl4co_amd import kernels as K

    rec = R.record("op", "c10_a5")
    for env in ("op", "pctsp", "spctsp"):
        with pytest.raises(NotImplementedError, match="rl4co_aco_prize"):
            K.aco_prize(rec["pheromone0"].clone(), env=env, n_ants=5)
    with pytest.raises(NotImplementedError, match="rl4co_aco_prize"):
        K.aco_prize(rec["pheromone0"].clone(), env="cvrp", n_ants=5)

