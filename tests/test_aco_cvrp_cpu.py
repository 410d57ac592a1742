"""Ant System (CVRP) without a device: the restatement (tests/aco_cvrp_ref.py) against the records of the reference's own
AntSystem with its CVRPEnv (update, masks, lengths, the W-wide reward), the C boundary of rl4co_aco_cvrp (header == ctypes
table, the LDS tier formula, argument refusals) and the host class's refusals on the CVRP path. Every call of the entry here
is refused before a launch."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from rl4co_amd import _lib
from tests import aco_cvrp_ref as R

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "rl4co_amd.h").read_text()
ERR_ARG = 1
DUMMY = 0x10000  # non-null, never followed
C_TYPES = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64}


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_update_equals_the_reference_record(case):
    rec = R.record(case)
    c, ants, b, iters, alpha, beta, decay, phe0, _, mode = R.CASES[case]
    assert float(rec["noise_floor"]) <= R.MEASURED_NOISE_FLOOR
    assert bool((rec["pheromone0"] == (1 if phe0 is None else phe0)).all())
    state = R.fresh_state(rec["pheromone0"])
    for i in range(iters):
        actions = rec[f"actions_{i}"]
        assert actions.shape == (ants * b, int(rec["lengths"][i].max()))  # the reference trims to its longest row
        if mode == "multistart":
            assert torch.equal(actions[:, 0], rec["start_nodes"][i])
        R.update(state, actions, rec["reward"][i], decay, float(rec["Q"]))
        assert torch.equal(state["pheromone"], rec["pheromone"][i])
        assert torch.equal(state["final_reward"], rec["final_reward"][i])
        want = R.record_finals(rec, i)
        assert all(torch.equal(x, y) for x, y in zip(state["final_actions"], want)) and len(want) == b
        # one more trailing zero changes nothing but the closing edge of the rows that had none (the longest ones that end
        # at a customer): (0, 0) edges deposit nothing
        before = (rec["pheromone"][i - 1] if i else rec["pheromone0"]).clone()
        wide = R.update(R.fresh_state(before), R.pad(actions, R.width(c + 1)), rec["reward"][i], decay, float(rec["Q"]),
                        keep=actions.shape[1])
        open_rows = (actions[:, -1] != 0).nonzero()[:, 0]
        same = torch.ones_like(before, dtype=torch.bool)
        same[open_rows % b, actions[open_rows, -1], 0] = False
        assert torch.equal(wide["pheromone"][same], rec["pheromone"][i][same])
        assert all(torch.equal(x, y) for x, y in zip(wide["final_actions"], R.update(
            R.fresh_state(before), actions, rec["reward"][i], decay, float(rec["Q"]))["final_actions"]))
    assert not torch.equal(rec["pheromone"][0], rec["pheromone"][-1])


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_masks_lengths_and_logps_follow_the_record(case):
    rec = R.record(case)
    c, ants, b, iters, alpha, beta, decay, phe0, _, mode = R.CASES[case]
    w = R.width(c + 1)
    phe = rec["pheromone0"]
    for i in range(iters):
        ref_actions = rec[f"actions_{i}"]
        t_i = ref_actions.shape[1]
        starts = rec["start_nodes"][i] if mode == "multistart" else None
        actions, lengths, logps, _, masks = R.sample(phe, rec["log_heuristic"], rec["demand"], rec["vehicle_capacity"], starts,
                                                     None, alpha, beta, forced=R.pad(ref_actions, w))
        assert torch.equal(lengths, rec["lengths"][i]) and int(lengths.max()) == t_i
        assert torch.equal(actions[:, :t_i], ref_actions) and bool((actions[:, t_i:] == 0).all())
        steps = torch.arange(w)[None, :] < lengths[:, None]
        assert bool((actions[~steps] == 0).all()) and bool((logps[~steps] == 0).all())  # trailing zeros, log-prob 0
        taken = steps[:, :t_i]
        assert torch.equal(masks[:, :t_i][taken], rec[f"masks_{i}"][taken])
        assert bool((rec[f"logps_{i}"][~taken] == 0).all())  # the reference's padding steps: one feasible node
        assert float((logps[:, :t_i] - rec[f"logps_{i}"]).abs().max()) <= R.STEP_TOL
        assert float((logps[:, :t_i].double() - rec[f"logps64_{i}"]).abs().max()) <= R.STEP_TOL
        phe = rec["pheromone"][i]


def test_reward_w_is_within_the_measured_ulps_of_the_recorded_reward():
    worst = 0.0
    for case in R.CASES:
        rec = R.record(case)
        w = R.width(rec["locs"].shape[1])
        for i in range(R.CASES[case][3]):
            trimmed = rec[f"actions_{i}"]
            assert torch.equal(R.reward_w(rec["locs"], trimmed), rec["reward"][i])  # the reference's own row, bit for bit
            got = R.reward_w(rec["locs"], R.pad(trimmed, w))
            ulp = torch.finfo(torch.float32).eps * 2.0 ** torch.floor(torch.log2(rec["reward"][i].abs()))
            worst = max(worst, float(((got - rec["reward"][i]).abs() / ulp).max()))
    print(f"reward_w against the recorded (trimmed) reward: {worst} ulps of the tour length (bound {R.REWARD_ULPS})")
    assert worst <= R.REWARD_ULPS


def test_capacity_regimes_give_the_lengths_the_width_is_built_from():
    n, b = 6, 1
    c = n - 1
    phe, heu = torch.ones(b, n, n), torch.zeros(b, n, n)
    heu[:, 1:, 0] = -50.0  # a customer's way back to the depot is taken only when nothing else is feasible
    noise = R.ln_exp1((R.width(n), 3, n), seed=1)
    cap = torch.ones(b)
    _, lengths, _, _, _ = R.sample(phe, heu, torch.full((b, c), 0.01), cap, None, noise)
    assert lengths.tolist() == [c + 1] * 3  # capacity never binds: one closing depot visit
    actions, lengths, _, _, _ = R.sample(phe, heu, torch.full((b, c), 0.6), cap, torch.tensor([1, 2, 3]), noise)
    assert lengths.tolist() == [2 * c - 1] * 3 == [R.width(n)] * 3  # a depot return between any two customers
    assert bool((actions[:, 1::2] == 0).all()) and bool((actions[:, 0::2] > 0).all())


def _struct_fields():
    body = re.search(r"typedef struct rl4co_aco_cvrp_args \{(.*?)\} rl4co_aco_cvrp_args;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"([\w ]+?)(\*?)\s*(\w+)\s*;", body)


def test_header_ctypes_and_symbols_agree():
    decls = _struct_fields()
    assert [d[2] for d in decls] == [f[0] for f in _lib.AcoCvrpArgs._fields_]
    for (ctype, star, name), (_, mirror) in zip(decls, _lib.AcoCvrpArgs._fields_):
        assert mirror is (ctypes.c_void_p if star else C_TYPES[ctype.strip()]), name
    assert ctypes.sizeof(_lib.AcoCvrpArgs) == 14 * 4 + 2 * 8 + 23 * 8
    assert "int rl4co_aco_cvrp(const rl4co_aco_cvrp_args* args, void* stream);" in HEADER
    assert "int rl4co_aco_cvrp_lds_nodes(void);" in HEADER
    restype, argtypes = _lib.SYMBOLS["rl4co_aco_cvrp"]
    assert restype is ctypes.c_int and argtypes == [ctypes.POINTER(_lib.AcoCvrpArgs), ctypes.c_void_p]
    assert _lib.SYMBOLS["rl4co_aco_cvrp_lds_nodes"] == (ctypes.c_int, [])
    assert _lib.ABI_VERSION >= 19 and _lib.lib().rl4co_abi_version() == _lib.ABI_VERSION


def test_struct_layout_is_the_compilers(tmp_path):
    import shutil
    import subprocess

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "rl4co_amd.h"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(rl4co_aco_cvrp_args));']
    lines += [f'  printf("{f} %zu\\n", offsetof(rl4co_aco_cvrp_args, {f}));' for f, _ in _lib.AcoCvrpArgs._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    table = dict(row.split() for row in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(table["sizeof"]) == ctypes.sizeof(_lib.AcoCvrpArgs)
    for f, _ in _lib.AcoCvrpArgs._fields_:
        assert int(table[f]) == getattr(_lib.AcoCvrpArgs, f).offset, f


def _args(**over):
    """Valid scalars, every pointer of a fused multistart launch set."""
    a = _lib.AcoCvrpArgs()
    a.B, a.N, a.n_ants, a.iterations, a.phases, a.has_best, a.T = 4, 21, 8, 3, 3, 0, 39
    a.alpha, a.beta, a.decay, a.Q, a.temperature = 1.0, 1.0, 0.95, 0.1, 1.0
    for f in ("log_heuristic", "pheromone", "locs", "demand", "vehicle_capacity", "start_nodes", "actions", "lengths", "reward",
              "logps", "final_reward", "final_actions", "final_iteration", "err"):
        setattr(a, f, DUMMY)
    for k, v in over.items():
        setattr(a, k, v)
    return a


REFUSALS = [
    (dict(B=0), b"a.B >= 1"),
    (dict(N=1), b"a.N >= 2"),
    (dict(N=1025), b"a.N <= 1024"),
    (dict(n_ants=0), b"a.n_ants >= 1"),
    (dict(iterations=0), b"a.iterations >= 1"),
    (dict(phases=0), b"a.phases >= 1"),
    (dict(phases=4), b"a.phases <= (RL4CO_ACO_SAMPLE | RL4CO_ACO_UPDATE)"),
    (dict(phases=1, iterations=2), b"(sample && update) || a.iterations == 1"),
    (dict(locs=None), b"!(sample && update) || a.locs != nullptr"),
    (dict(T=38), b"a.T == cvrp_width(a.N)"),
    (dict(phases=2, iterations=1, T=1), b"a.T >= 2"),
    (dict(temperature=0.0), b"a.temperature > 0.0f"),
    (dict(log_heuristic=None), b"a.log_heuristic != nullptr"),
    (dict(demand=None), b"a.demand != nullptr"),
    (dict(vehicle_capacity=None), b"a.vehicle_capacity != nullptr"),
    (dict(lengths=None), b"a.lengths != nullptr"),
    (dict(forced_actions=DUMMY), b"a.forced_actions == nullptr"),  # iterations = 3
    (dict(pheromone=None), b"a.pheromone != nullptr"),
    (dict(actions=None), b"a.actions != nullptr"),
    (dict(reward=None), b"a.reward != nullptr"),
    (dict(final_reward=None), b"a.final_reward != nullptr"),
    (dict(err=None), b"a.err != nullptr"),
    (dict(N=142, T=281), b"lds || a.logits_scratch != nullptr"),
]


@pytest.mark.parametrize("over,text", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o, _ in REFUSALS])
def test_argument_refusals(over, text):
    assert _lib.lib().rl4co_aco_cvrp(ctypes.byref(_args(**over)), None) == ERR_ARG
    msg = _lib.lib().rl4co_last_error()
    assert b"requirement failed" in msg and text in msg, msg
    assert _lib.lib().rl4co_aco_cvrp(None, None) == ERR_ARG and b"args != nullptr" in _lib.lib().rl4co_last_error()


def test_lds_nodes_is_the_headers_formula():
    """8 n^2 (logits + pheromone) + 8 roundup(W + 1, 8) (wave tours) + 4 roundup(n, 4) (demands) + 256 + 64 <= 160 KiB"""
    def fits(n):
        return 8 * n * n + 8 * ((R.width(n) + 1 + 7) // 8 * 8) + 4 * ((n + 3) // 4 * 4) + 256 + 64 <= 160 * 1024

    want = max(n for n in range(2, 1025) if fits(n))
    assert _lib.lib().rl4co_aco_cvrp_lds_nodes() == want == 141
    text = (ROOT / "rl4co_amd" / "csrc" / "aco_cvrp.hip").read_text()
    assert "8 N^2 + 8 roundup(W + 1, 8) + 4 roundup(N, 4) + 256 + 64 <= 160 KiB" in text and "N <= 141" in text


class _Env:
    def __init__(self, name):
        self.name = name


MS = dict(multisample=True, num_samples=5, select_best=False)


def _system(**kw):
    from rl4co_amd import AntSystem

    rec = R.record("c10_a5")
    return AntSystem(rec["log_heuristic"], n_ants=5, **kw), {"locs": rec["locs"]}  # (no demand: refused before it is read)


def test_host_refusals_on_the_cvrp_path():
    aco, td = _system()
    env = _Env("cvrp")
    for kw in (MS, dict(multistart=True, num_starts=5, select_best=False)):
        with pytest.raises(NotImplementedError, match="rl4co_aco_cvrp"):  # CPU tensors
            aco.run(td, env, 2, kw)
        with pytest.raises(NotImplementedError, match="rl4co_aco_cvrp"):
            aco._one_step(td, env, kw)
    with pytest.raises(NotImplementedError, match="use_local_search"):
        _system(use_local_search=True)[0].run(td, env, 2, MS)
    with pytest.raises(NotImplementedError, match="num_samples"):
        aco.run(td, env, 2, dict(MS, num_samples=7))
    with pytest.raises(NotImplementedError, match="num_starts"):
        aco.run(td, env, 2, dict(multistart=True, num_starts=7))
    with pytest.raises(NotImplementedError, match="exactly one of"):
        aco.run(td, env, 2, dict(MS, multistart=True))
    with pytest.raises(NotImplementedError, match="exactly one of"):
        aco.run(td, env, 2, dict(select_best=False))
    for key, value in (("top_k", 5), ("top_p", 0.9), ("tanh_clipping", 10.0)):
        with pytest.raises(NotImplementedError, match=key):
            aco.run(td, env, 2, dict(MS, **{key: value}))
    with pytest.raises(NotImplementedError, match="select_best"):
        aco.run(td, env, 2, dict(MS, select_best=True))
    with pytest.raises(NotImplementedError, match="op"):
        aco.run(td, _Env("op"), 2, MS)


def test_binding_refuses_cpu_tensors():
    from rl4co_amd import kernels as K

    rec = R.record("c10_a5")
    with pytest.raises(NotImplementedError, match="rl4co_aco_cvrp"):
        K.aco_cvrp(rec["pheromone0"].clone(), n_ants=5)
    assert K.aco_cvrp_width(11) == R.width(11) == 19 and K.aco_cvrp_width(2) == 2 and K.aco_cvrp_width(3) == 3
