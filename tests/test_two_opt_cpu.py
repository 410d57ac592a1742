"""TSP 2-opt local search without a device: the restatement (tests/two_opt_ref.py) against the records of the reference's
own local_search.py, the C boundary of rl4co_tsp_two_opt (header == ctypes table, the argument refusals, the LDS tier
formula) and the environment methods' refusals. Every call of the entry here is refused before a launch."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from rl4co_amd import _lib
from tests import two_opt_ref as R

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "rl4co_amd.h").read_text()
ERR_ARG = 1
DUMMY = 0x10000  # non-null, never followed


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_equals_the_reference_record(case):
    rec = R.record(case)
    cap = R.CASES[case][3]
    tours, iters = R.two_opt(R.record_distances(rec), rec["in_actions"], cap)
    assert torch.equal(tours, rec["out_actions"])
    assert torch.equal(iters, rec["iterations"])
    # the records are what they are meant to be: the search did something, the cap binds where it should
    assert not torch.equal(rec["out_actions"], rec["in_actions"]) and int(rec["iterations"].max()) <= cap
    assert torch.equal(rec["out_actions"].sort(1).values, rec["in_actions"].sort(1).values)
    if case == "tsp20_cap2":
        full = R.record("tsp20")
        assert torch.equal(rec["in_locs"], full["in_locs"]) and torch.equal(rec["in_actions"], full["in_actions"])
        assert bool((full["iterations"] > 2).all()) and bool((rec["iterations"] == 2).all())


def test_lattice_record_has_ties_the_rule_decides():
    """On the 4 x 4 grid the smallest change of a scan is shared by several pairs: the first in (i, j) order is taken."""
    rec = R.record("lattice16")
    d = R.with_diagonal(R.record_distances(rec))
    pairs = R.pair_list(16)
    i, j = pairs
    tied = 0
    for b in range(rec["in_actions"].shape[0]):
        tour = rec["in_actions"][b].numpy().copy()
        for _ in range(int(rec["iterations"][b]) - 1):  # every improving scan of the recorded search
            change = ((d[b][tour[i - 1], tour[j]] + d[b][tour[i], tour[(j + 1) % 16]]) - d[b][tour[i - 1], tour[i]]) \
                - d[b][tour[j], tour[(j + 1) % 16]]
            move = R.best_move(d[b], tour, pairs)
            hits = (change == move[0]).nonzero()[0]
            tied += hits.size > 1
            assert (int(i[hits[0]]), int(j[hits[0]])) == move[1:]
            tour[move[1] : move[2] + 1] = tour[move[1] : move[2] + 1][::-1].copy()
        assert tour.tolist() == rec["out_actions"][b].tolist()
    assert tied > 0


def test_header_ctypes_and_symbols_agree():
    body = re.search(r"typedef struct rl4co_tsp_two_opt_args \{(.*?)\} rl4co_tsp_two_opt_args;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = re.findall(r"([\w ]+?)(\*?)\s*(\w+)\s*;", body)
    assert [d[2] for d in decls] == [f[0] for f in _lib.TspTwoOptArgs._fields_]
    for (ctype, star, name), (_, mirror) in zip(decls, _lib.TspTwoOptArgs._fields_):
        assert mirror is (ctypes.c_void_p if star else ctypes.c_int32), name
        assert star or ctype.strip() == "int32_t", name
    assert ctypes.sizeof(_lib.TspTwoOptArgs) == 4 * 4 + 6 * 8
    assert "int rl4co_tsp_two_opt(const rl4co_tsp_two_opt_args* args, void* stream);" in HEADER
    assert "int rl4co_tsp_two_opt_lds_nodes(void);" in HEADER
    restype, argtypes = _lib.SYMBOLS["rl4co_tsp_two_opt"]
    assert restype is ctypes.c_int and argtypes == [ctypes.POINTER(_lib.TspTwoOptArgs), ctypes.c_void_p]
    assert _lib.SYMBOLS["rl4co_tsp_two_opt_lds_nodes"] == (ctypes.c_int, [])
    assert _lib.ABI_VERSION >= 17 and _lib.lib().rl4co_abi_version() == _lib.ABI_VERSION
    assert _lib.EBIT_TOUR_INDEX == 262144 and "#define RL4CO_EBIT_TOUR_INDEX 262144" in HEADER
    with pytest.raises(AssertionError, match="tour index out of range"):
        _lib.raise_for_error_bits(_lib.EBIT_TOUR_INDEX)


def _args(**over):
    """Valid scalars, every required pointer set, `locs` as the distance source."""
    a = _lib.TspTwoOptArgs()
    a.B, a.N, a.T, a.max_iterations = 4, 20, 20, 10
    a.locs, a.distances = DUMMY, None
    a.actions, a.out_actions, a.iterations, a.err = DUMMY, DUMMY, None, DUMMY
    for k, v in over.items():
        setattr(a, k, v)
    return a


REFUSALS = [
    (dict(B=0), b"a.B >= 1"),
    (dict(N=1), b"a.N >= 2"),
    (dict(N=1025), b"a.N <= 1024"),
    (dict(T=0), b"a.T >= 1"),
    (dict(T=1025), b"a.T <= 1024"),
    (dict(max_iterations=-1), b"a.max_iterations >= 0"),
    (dict(distances=DUMMY), b"a.locs != nullptr) != (a.distances != nullptr"),  # both sources
    (dict(locs=None), b"a.locs != nullptr) != (a.distances != nullptr"),       # neither
    (dict(actions=None), b"a.actions != nullptr"),
    (dict(out_actions=None), b"a.out_actions != nullptr"),
    (dict(err=None), b"a.err != nullptr"),
]


@pytest.mark.parametrize("over,text", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o, _ in REFUSALS])
def test_argument_refusals(over, text):
    fn = _lib.lib().rl4co_tsp_two_opt
    assert fn(ctypes.byref(_args(**over)), None) == ERR_ARG
    msg = _lib.lib().rl4co_last_error()
    assert b"requirement failed" in msg and text in msg, msg


def test_null_args_refused():
    assert _lib.lib().rl4co_tsp_two_opt(None, None) == ERR_ARG
    assert b"args != nullptr" in _lib.lib().rl4co_last_error()


def test_lds_nodes_is_the_headers_formula():
    """4 N^2 (matrix) + 2 * 1024 (tour) + 64 (reduction scratch) + 64 (static allowance) <= 160 KiB"""
    want = max(n for n in range(2, 1025) if 4 * n * n + 2 * 1024 + 64 + 64 <= 160 * 1024)
    assert _lib.lib().rl4co_tsp_two_opt_lds_nodes() == want == 201
    text = (ROOT / "rl4co_amd" / "csrc" / "tsp_two_opt.hip").read_text()
    assert "4 N^2 + 2 * 1024 + 64 + 64 <= 160 KiB" in text and "N <= 201" in text


def test_local_search_on_cpu_tensors_names_the_kernel():
    from rl4co_amd.envs import TSPEnv

    rec = R.record("tsp20")
    with pytest.raises(NotImplementedError, match="rl4co_tsp_two_opt"):
        TSPEnv.local_search({"locs": rec["in_locs"]}, rec["in_actions"])
    with pytest.raises(NotImplementedError, match="rl4co_tsp_two_opt"):
        TSPEnv.local_search({"locs": rec["in_locs"], "distances": R.record_distances(rec)}, rec["in_actions"], max_iterations=5,
                            num_threads=4)


def test_other_environments_have_no_local_search():
    from rl4co_amd.envs import get_env

    rec = R.record("tsp20")
    with pytest.raises(NotImplementedError, match="cvrp"):
        get_env("cvrp").local_search({"locs": rec["in_locs"]}, rec["in_actions"])


def test_host_binding_refuses_bad_shapes_before_the_device():
    from rl4co_amd import kernels as K

    rec = R.record("tsp20")
    acts, locs = rec["in_actions"], rec["in_locs"]
    with pytest.raises(ValueError, match="exactly one"):
        K.tsp_two_opt(acts)
    with pytest.raises(ValueError, match="exactly one"):
        K.tsp_two_opt(acts, locs=locs, distances=R.record_distances(rec))
    with pytest.raises(TypeError, match="int64"):
        K.tsp_two_opt(acts.int(), locs=locs)
    with pytest.raises(TypeError, match="float32"):
        K.tsp_two_opt(acts, locs=locs.double())
    with pytest.raises(ValueError, match=r"\[B, N, 2\]"):
        K.tsp_two_opt(acts, locs=locs[:3])
    with pytest.raises(ValueError, match=r"\[B, N, N\]"):
        K.tsp_two_opt(acts, distances=R.record_distances(rec)[:, :, :5])
    with pytest.raises(_lib.Rl4coLibraryError, match="no CPU fallback"):
        K.tsp_two_opt(acts, locs=locs)
