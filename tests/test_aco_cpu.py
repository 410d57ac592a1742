"""Ant System (TSP) without a device: the restatement's update (tests/aco_ref.py) against the records of the reference's own
AntSystem, the C boundary of rl4co_aco_tsp (header == ctypes table, the argument refusals, the LDS tier formula) and the
host class's refusals. Every call of the entry here is refused before a launch."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from rl4co_amd import _lib
from tests import aco_ref as R

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "rl4co_amd.h").read_text()
ERR_ARG = 1
DUMMY = 0x10000  # non-null, never followed
C_TYPES = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64}


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_update_equals_the_reference_record(case):
    rec = R.record(case)
    n, ants, b, iters, alpha, beta, decay, phe0, _ = R.CASES[case]
    assert rec["actions"].shape == (iters, ants * b, n) and float(rec["noise_floor"]) <= R.MEASURED_NOISE_FLOOR
    assert bool((rec["pheromone0"] == (1 if phe0 is None else phe0)).all())
    state = R.fresh_state(rec["pheromone0"])
    for i in range(iters):
        # the record is what it is meant to be: permutations from the recorded start nodes, rewards of those tours
        assert torch.equal(rec["actions"][i].sort(1).values, torch.arange(n).expand(ants * b, n))
        assert torch.equal(rec["actions"][i][:, 0], rec["start_nodes"][i])
        assert torch.equal(R.tour_reward(rec["locs"], rec["actions"][i]), rec["reward"][i])
        R.update(state, rec["actions"][i], rec["reward"][i], decay, float(rec["Q"]))
        assert torch.equal(state["pheromone"], rec["pheromone"][i])
        assert torch.equal(state["final_reward"], rec["final_reward"][i])
        assert torch.equal(state["final_actions"], rec["final_actions"][i])
    assert not torch.equal(rec["pheromone"][0], rec["pheromone"][-1])


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_logps_are_within_the_noise_floor_of_the_record(case):
    rec = R.record(case)
    n, ants, b, iters, alpha, beta, decay, phe0, _ = R.CASES[case]
    phe = rec["pheromone0"]
    for i in range(iters):
        _, logps, _ = R.sample(phe, rec["log_heuristic"], rec["start_nodes"][i], None, alpha, beta, forced=rec["actions"][i])
        assert float((logps - rec["logps"][i]).abs().max()) <= R.STEP_TOL
        assert float((logps.double() - rec["logps64"][i]).abs().max()) <= R.STEP_TOL
        phe = rec["pheromone"][i]


def test_all_equal_rewards_deposit_nan_and_selection_takes_the_lowest_index():
    state = R.fresh_state(torch.ones(1, 4, 4))
    acts = torch.tensor([[0, 1, 2, 3], [1, 0, 3, 2]])
    R.update(state, acts, torch.tensor([-2.0, -2.0]), 0.5, 1.0)
    want_nan = torch.zeros(4, 4, dtype=torch.bool)
    for f, t in [(0, 1), (1, 2), (2, 3), (1, 0), (0, 3), (3, 2)]:
        want_nan[f, t] = True
    assert torch.equal(torch.isnan(state["pheromone"][0]), want_nan)
    assert bool((state["pheromone"][0][~want_nan] == 0.5).all())
    assert state["final_actions"].tolist() == [[0, 1, 2, 3]]  # the lowest ant on equal rewards
    lp = torch.log(torch.tensor([0.25, 0.25, 0.25, 0.25]))
    assert R.select(lp, torch.zeros(4), torch.tensor([True, False, False, False])) == 1


def _struct_fields():
    body = re.search(r"typedef struct rl4co_aco_tsp_args \{(.*?)\} rl4co_aco_tsp_args;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"([\w ]+?)(\*?)\s*(\w+)\s*;", body)


def test_header_ctypes_and_symbols_agree():
    decls = _struct_fields()
    assert [d[2] for d in decls] == [f[0] for f in _lib.AcoTspArgs._fields_]
    for (ctype, star, name), (_, mirror) in zip(decls, _lib.AcoTspArgs._fields_):
        assert mirror is (ctypes.c_void_p if star else C_TYPES[ctype.strip()]), name
    assert ctypes.sizeof(_lib.AcoTspArgs) == 12 * 4 + 2 * 8 + 18 * 8
    assert "int rl4co_aco_tsp(const rl4co_aco_tsp_args* args, void* stream);" in HEADER
    assert "int rl4co_aco_tsp_lds_nodes(void);" in HEADER
    restype, argtypes = _lib.SYMBOLS["rl4co_aco_tsp"]
    assert restype is ctypes.c_int and argtypes == [ctypes.POINTER(_lib.AcoTspArgs), ctypes.c_void_p]
    assert _lib.SYMBOLS["rl4co_aco_tsp_lds_nodes"] == (ctypes.c_int, [])
    assert _lib.ABI_VERSION >= 18 and _lib.lib().rl4co_abi_version() == _lib.ABI_VERSION
    assert (_lib.ACO_SAMPLE, _lib.ACO_UPDATE) == (1, 2)
    assert "#define RL4CO_ACO_SAMPLE 1" in HEADER and "#define RL4CO_ACO_UPDATE 2" in HEADER


def test_struct_layout_is_the_compilers(tmp_path):
    import shutil
    import subprocess

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "rl4co_amd.h"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(rl4co_aco_tsp_args));']
    lines += [f'  printf("{f} %zu\\n", offsetof(rl4co_aco_tsp_args, {f}));' for f, _ in _lib.AcoTspArgs._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    table = dict(row.split() for row in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(table["sizeof"]) == ctypes.sizeof(_lib.AcoTspArgs)
    for f, _ in _lib.AcoTspArgs._fields_:
        assert int(table[f]) == getattr(_lib.AcoTspArgs, f).offset, f


def _args(**over):
    """Valid scalars, every pointer of a fused launch set."""
    a = _lib.AcoTspArgs()
    a.B, a.N, a.n_ants, a.iterations, a.phases, a.has_best = 4, 20, 8, 3, 3, 0
    a.alpha, a.beta, a.decay, a.Q, a.temperature = 1.0, 1.0, 0.95, 0.1, 1.0
    for f in ("log_heuristic", "pheromone", "locs", "start_nodes", "actions", "reward", "logps", "final_reward", "final_actions",
              "err"):
        setattr(a, f, DUMMY)
    for k, v in over.items():
        setattr(a, k, v)
    return a


REFUSALS = [
    (dict(B=0), b"a.B >= 1"),
    (dict(N=1), b"a.N >= 2"),
    (dict(N=1025), b"a.N <= 1024"),
    (dict(n_ants=0), b"a.n_ants >= 1"),
    (dict(n_ants=1 << 30, B=4), b"a.n_ants * a.B <= 2147483647LL"),
    (dict(iterations=0), b"a.iterations >= 1"),
    (dict(phases=0), b"a.phases >= 1"),
    (dict(phases=4), b"a.phases <= (RL4CO_ACO_SAMPLE | RL4CO_ACO_UPDATE)"),
    (dict(phases=1, iterations=2), b"(sample && update) || a.iterations == 1"),
    (dict(phases=2, iterations=2), b"(sample && update) || a.iterations == 1"),
    (dict(locs=None), b"!(sample && update) || a.locs != nullptr"),
    (dict(temperature=0.0), b"a.temperature > 0.0f"),
    (dict(temperature=-1.0), b"a.temperature > 0.0f"),
    (dict(temperature=float("nan")), b"a.temperature > 0.0f"),
    (dict(log_heuristic=None), b"a.log_heuristic != nullptr"),
    (dict(start_nodes=None), b"a.start_nodes != nullptr"),
    (dict(forced_actions=DUMMY), b"a.forced_actions == nullptr"),  # iterations = 3
    (dict(pheromone=None), b"a.pheromone != nullptr"),
    (dict(actions=None), b"a.actions != nullptr"),
    (dict(reward=None), b"a.reward != nullptr"),
    (dict(final_reward=None), b"a.final_reward != nullptr"),
    (dict(err=None), b"a.err != nullptr"),
    (dict(N=140), b"lds || a.logits_scratch != nullptr"),
]


@pytest.mark.parametrize("over,text", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o, _ in REFUSALS])
def test_argument_refusals(over, text):
    assert _lib.lib().rl4co_aco_tsp(ctypes.byref(_args(**over)), None) == ERR_ARG
    msg = _lib.lib().rl4co_last_error()
    assert b"requirement failed" in msg and text in msg, msg


def test_null_args_refused():
    assert _lib.lib().rl4co_aco_tsp(None, None) == ERR_ARG
    assert b"args != nullptr" in _lib.lib().rl4co_last_error()


def test_lds_nodes_is_the_headers_formula():
    """8 N^2 (logits + pheromone) + 8192 (wave tours) + 256 (scratch) + 64 (static allowance) <= 160 KiB"""
    want = max(n for n in range(2, 1025) if 8 * n * n + 8192 + 256 + 64 <= 160 * 1024)
    assert _lib.lib().rl4co_aco_tsp_lds_nodes() == want == 139
    text = (ROOT / "rl4co_amd" / "csrc" / "aco_tsp.hip").read_text()
    assert "8 N^2 + 8192 + 256 + 64 <= 160 KiB" in text and "N <= 139" in text


class _Env:
    def __init__(self, name):
        self.name = name


KW = dict(multistart=True, num_starts=5, select_best=False)


def _system(**kw):
    from rl4co_amd import AntSystem

    rec = R.record("tsp12_a5")
    return AntSystem(rec["log_heuristic"], n_ants=5, **kw), {"locs": rec["locs"]}


def test_constructor_is_the_references():
    aco, _ = _system()
    assert (aco.n_ants, aco.alpha, aco.beta, aco.decay, aco.use_local_search, aco.use_nls, aco.n_perturbations) == \
        (5, 1.0, 1.0, 0.95, False, False, 1)
    assert aco.Q == 1 / 5 / 0.95 and aco.batch_size == 4 and bool((aco.pheromone == 1).all())
    assert aco.final_actions is None and aco.final_reward is None and aco.final_reward_cache == {}
    assert bool((_system(pheromone=2)[0].pheromone == 2).all())
    params = {"max_iterations": 5}
    other, _ = _system(Q=0.5, use_local_search=True, local_search_params=params)
    assert other.Q == 0.5 and other.local_search_params == params and other.local_search_params is not params


def test_host_refusals():
    aco, td = _system()
    with pytest.raises(NotImplementedError, match="rl4co_aco_tsp"):  # CPU tensors
        aco.run(td, _Env("tsp"), 2, KW)
    with pytest.raises(NotImplementedError, match="rl4co_aco_tsp"):
        aco._one_step(td, _Env("tsp"), KW)
    for key, value in (("top_k", 5), ("top_p", 0.9), ("multisample", True), ("tanh_clipping", 10.0)):
        with pytest.raises(NotImplementedError, match=key):
            aco.run(td, _Env("tsp"), 2, dict(KW, **{key: value}))
    with pytest.raises(NotImplementedError, match="cvrp"):
        aco.run(td, _Env("cvrp"), 2, KW)
    with pytest.raises(NotImplementedError, match="num_starts"):
        aco.run(td, _Env("tsp"), 2, dict(KW, num_starts=7))
    with pytest.raises(NotImplementedError, match="multistart"):
        aco.run(td, _Env("tsp"), 2, dict(select_best=False))
    with pytest.raises(NotImplementedError, match="select_best"):
        aco.run(td, _Env("tsp"), 2, dict(KW, select_best=True))
    with pytest.raises(NotImplementedError, match="use_nls"):
        _system(use_local_search=True, use_nls=True)
    with pytest.raises(AssertionError, match="use_nls requires use_local_search"):
        _system(use_nls=True)


def test_binding_refuses_cpu_tensors():
    from rl4co_amd import kernels as K

    rec = R.record("tsp12_a5")
    with pytest.raises(_lib.Rl4coLibraryError, match="no CPU fallback"):
        K.aco_tsp(rec["pheromone0"].clone(), n_ants=5)
