"""Neural-guided local search without a device: the restatement (tests/nls_ref.py) against the records of the reference's
own AntSystem.local_search(use_nls=True), the C boundary of rl4co_tsp_nls (header == ctypes table == the compiler's layout,
the argument refusals, the LDS tier), the host binding's refusals and the class surface that needs no kernel. Every call of
the entry here is refused before a launch."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from rl4co_amd import _lib
from tests import nls_ref as R
from tests import two_opt_ref as T
from tests.aco_ref import tour_reward

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "rl4co_amd.h").read_text()
ERR_ARG = 1
DUMMY = 0x10000  # non-null, never followed


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_equals_the_reference_record(case):
    rec = R.record(case)
    acts, rews, scans, accepted = R.nls(rec["locs"], rec["heuristic_dist"], rec["in_actions"], **R.case_params(case))
    assert torch.equal(acts, rec["best_actions"])
    assert torch.equal(rews, rec["best_rewards"])
    assert torch.equal(accepted, rec["accepted"])
    # the records are what they are meant to be: a perturbed tour was taken somewhere and a round was turned down somewhere
    p = R.case_params(case)["n_perturbations"]
    assert int(accepted.max()) > 0 and int(accepted.min()) < p
    assert torch.equal(acts.sort(1).values, rec["in_actions"].sort(1).values)
    assert torch.equal(rews, tour_reward(rec["locs"], acts))
    assert scans.shape == (acts.shape[0], 1 + 2 * p)
    # the inputs are the seeded ones and the recorded perturbation matrix is the reference formula of the recorded heatmap
    data = R.case_inputs(case)
    assert all(torch.equal(data[k], rec[k]) for k in data)
    assert torch.equal(R.heuristic_dist(rec["log_heuristic"]), rec["heuristic_dist"])
    if case == "tsp12_a3_p3_cap":  # the caps bind: every search over the real distances stopped at 2 scans somewhere
        assert int(scans[:, 0::2].max()) == 2 and bool((scans[:, 0] == 2).any())
        assert int(scans[:, 1::2].max()) <= 5


def test_no_perturbation_is_the_two_opt_and_its_reward():
    rec = R.record("tsp20_a4_p1")
    acts, rews, scans, accepted = R.nls(rec["locs"], rec["heuristic_dist"], rec["in_actions"], 0)
    rows = rec["in_actions"].shape[0]
    real = T.distance_matrix(rec["locs"])[torch.arange(rows) % rec["locs"].shape[0]]
    tours, iters = T.two_opt(real, rec["in_actions"])
    assert torch.equal(acts, tours) and torch.equal(scans, iters[:, None]) and not bool(accepted.any())
    assert torch.equal(rews, tour_reward(rec["locs"], tours))


def test_a_round_that_cannot_move_is_turned_down():
    """perturb_max_iterations = 0: the tour comes back from the repair as it went in, equal rewards do not win."""
    rec = R.record("tsp12_a5_p2")
    first = R.nls(rec["locs"], rec["heuristic_dist"], rec["in_actions"], 0)
    acts, rews, scans, accepted = R.nls(rec["locs"], rec["heuristic_dist"], rec["in_actions"], 2, perturb_max_iterations=0)
    assert torch.equal(acts, first[0]) and torch.equal(rews, first[1]) and not bool(accepted.any())
    assert bool((scans[:, 1::2] == 0).all()) and bool((scans[:, 2::2] == 1).all())


C_TYPES = {"int32_t": ctypes.c_int32}


def _struct_fields():
    body = re.search(r"typedef struct rl4co_tsp_nls_args \{(.*?)\} rl4co_tsp_nls_args;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"([\w ]+?)(\*?)\s*(\w+)\s*;", body)


def test_header_ctypes_and_symbols_agree():
    decls = _struct_fields()
    assert [d[2] for d in decls] == [f[0] for f in _lib.TspNlsArgs._fields_]
    for (ctype, star, name), (_, mirror) in zip(decls, _lib.TspNlsArgs._fields_):
        assert mirror is (ctypes.c_void_p if star else C_TYPES[ctype.strip()]), name
    assert ctypes.sizeof(_lib.TspNlsArgs) == 8 * 4 + 8 * 8
    assert "int rl4co_tsp_nls(const rl4co_tsp_nls_args* args, void* stream);" in HEADER
    assert "int rl4co_tsp_nls_lds_nodes(void);" in HEADER
    restype, argtypes = _lib.SYMBOLS["rl4co_tsp_nls"]
    assert restype is ctypes.c_int and argtypes == [ctypes.POINTER(_lib.TspNlsArgs), ctypes.c_void_p]
    assert _lib.SYMBOLS["rl4co_tsp_nls_lds_nodes"] == (ctypes.c_int, [])
    assert _lib.ABI_VERSION >= 20 and _lib.lib().rl4co_abi_version() == _lib.ABI_VERSION
    assert re.search(r"^ \*\s+20: rl4co_tsp_nls", HEADER, re.M)


def test_struct_layout_is_the_compilers(tmp_path):
    import shutil
    import subprocess

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "rl4co_amd.h"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(rl4co_tsp_nls_args));']
    lines += [f'  printf("{f} %zu\\n", offsetof(rl4co_tsp_nls_args, {f}));' for f, _ in _lib.TspNlsArgs._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    table = dict(row.split() for row in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(table["sizeof"]) == ctypes.sizeof(_lib.TspNlsArgs)
    for f, _ in _lib.TspNlsArgs._fields_:
        assert int(table[f]) == getattr(_lib.TspNlsArgs, f).offset, f


def _args(**over):
    """Valid scalars, every required pointer set."""
    a = _lib.TspNlsArgs()
    a.R, a.n_instances, a.N, a.T = 8, 4, 20, 20
    a.ls_max_iterations, a.perturb_max_iterations, a.n_perturbations = 10, 5, 2
    for f in ("locs", "perturb_distances", "actions", "out_actions", "out_reward", "err"):
        setattr(a, f, DUMMY)
    for k, v in over.items():
        setattr(a, k, v)
    return a


REFUSALS = [
    (dict(R=0), b"a.R >= 1"),
    (dict(n_instances=0), b"a.n_instances >= 1"),
    (dict(n_instances=3), b"a.R % a.n_instances == 0"),
    (dict(N=1), b"a.N >= 2"),
    (dict(N=1025), b"a.N <= 1024"),
    (dict(T=0), b"a.T >= 1"),
    (dict(T=1025), b"a.T <= 1024"),
    (dict(ls_max_iterations=-1), b"a.ls_max_iterations >= 0"),
    (dict(perturb_max_iterations=-1), b"a.perturb_max_iterations >= 0"),
    (dict(n_perturbations=-1), b"a.n_perturbations >= 0"),
    (dict(n_perturbations=1 << 30), b"a.n_perturbations <= (1 << 30) - 1"),
    (dict(locs=None), b"a.locs != nullptr"),
    (dict(perturb_distances=None), b"a.perturb_distances != nullptr"),
    (dict(actions=None), b"a.actions != nullptr"),
    (dict(out_actions=None), b"a.out_actions != nullptr"),
    (dict(out_reward=None), b"a.out_reward != nullptr"),
    (dict(err=None), b"a.err != nullptr"),
]


@pytest.mark.parametrize("over,text", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o, _ in REFUSALS])
def test_argument_refusals(over, text):
    assert _lib.lib().rl4co_tsp_nls(ctypes.byref(_args(**over)), None) == ERR_ARG
    msg = _lib.lib().rl4co_last_error()
    assert b"requirement failed" in msg and text in msg, msg


def test_null_args_refused():
    assert _lib.lib().rl4co_tsp_nls(None, None) == ERR_ARG
    assert b"args != nullptr" in _lib.lib().rl4co_last_error()


def test_lds_nodes_is_the_two_opt_kernels():
    """4 N^2 (one matrix slot) + 2 * 1024 (tour) + 64 (scratch, the reward word in it) + 64 (static) <= 160 KiB"""
    want = max(n for n in range(2, 1025) if 4 * n * n + 2 * 1024 + 64 + 64 <= 160 * 1024)
    assert _lib.lib().rl4co_tsp_nls_lds_nodes() == want == 201 == _lib.lib().rl4co_tsp_two_opt_lds_nodes()
    text = (ROOT / "rl4co_amd" / "csrc" / "tsp_nls.hip").read_text()
    assert "4 N^2 + 2 * 1024 + 64 + 64 <= 160 KiB" in text and "N <= 201" in text


def test_both_kernels_call_one_text_of_the_search():
    """The scan / reduce / reverse loop and the LDS-tour reward exist once, in headers both users include."""
    csrc = ROOT / "rl4co_amd" / "csrc"
    two_opt, nls, aco = ((csrc / f).read_text() for f in ("tsp_two_opt.hip", "tsp_nls.hip", "aco_tsp.hip"))
    for text in (two_opt, nls):
        assert '#include "tsp_two_opt_search.h"' in text and " search(" in text
        assert "uint64_t bfly_min_u64(" not in text and "ord_key(" not in text  # no second definition, no second scan
    for text in (nls, aco):
        assert '#include "lds_tour_reward.h"' in text and "ant_reward(" in text
        assert "float lane_row_sum(" not in text and "float seg(" not in text
    assert "change both together" in (csrc / "lds_tour_reward.h").read_text()
    assert "change both together" in (csrc / "tour_length.hip").read_text()


def test_host_binding_refuses_bad_arguments_before_the_device():
    from rl4co_amd import kernels as K

    rec = R.record("tsp12_a5_p2")
    acts, locs, pert = rec["in_actions"], rec["locs"], rec["heuristic_dist"]
    with pytest.raises(TypeError, match="int64"):
        K.tsp_nls(acts.int(), locs=locs, perturb_distances=pert, n_perturbations=1)
    with pytest.raises(TypeError, match="locs must be torch.float32"):
        K.tsp_nls(acts, locs=locs.double(), perturb_distances=pert, n_perturbations=1)
    with pytest.raises(TypeError, match="perturb_distances must be torch.float32"):
        K.tsp_nls(acts, locs=locs, perturb_distances=pert.double(), n_perturbations=1)
    with pytest.raises(ValueError, match=r"\[R, T\]"):
        K.tsp_nls(acts[0], locs=locs, perturb_distances=pert, n_perturbations=1)
    with pytest.raises(ValueError, match=r"\[I, N, 2\]"):
        K.tsp_nls(acts, locs=locs[:, :, :1], perturb_distances=pert, n_perturbations=1)
    with pytest.raises(ValueError, match=r"\[I, N, N\]"):
        K.tsp_nls(acts, locs=locs, perturb_distances=pert[:, :, :5], n_perturbations=1)
    with pytest.raises(ValueError, match=r"\[I, N, N\]"):
        K.tsp_nls(acts, locs=locs, perturb_distances=pert[:1], n_perturbations=1)
    with pytest.raises(ValueError, match="R % I == 0"):
        K.tsp_nls(acts[:9], locs=locs, perturb_distances=pert, n_perturbations=1)
    for name in ("n_perturbations", "ls_max_iterations", "perturb_max_iterations"):
        with pytest.raises(ValueError, match=name):
            K.tsp_nls(acts, locs=locs, perturb_distances=pert, **dict(dict(n_perturbations=1), **{name: -1}))
    with pytest.raises(_lib.Rl4coLibraryError, match="no CPU fallback"):
        K.tsp_nls(acts, locs=locs, perturb_distances=pert, n_perturbations=1)


def _system(**kw):
    from rl4co_amd import AntSystem

    rec = R.record("tsp12_a5_p2")
    return AntSystem(rec["log_heuristic"], n_ants=5, **kw), rec


def test_use_nls_on_a_cpu_heatmap_is_refused_by_the_constructor():
    """The class builds heuristic_dist and searches on the heatmap's device: the constructor, the unknown-key TypeError and
    the CVRP refusal of a constructed object are checked on the device (tests/test_gpu_nls.py)."""
    with pytest.raises(NotImplementedError, match="use_nls.*rl4co_tsp_nls"):
        _system(use_local_search=True, use_nls=True, n_perturbations=2)
    with pytest.raises(AssertionError, match="use_nls requires use_local_search"):
        _system(use_nls=True)
    aco, rec = _system(use_local_search=True, n_perturbations=2, perturbation_params={"max_iterations": 5})
    assert not aco.use_nls and aco.n_perturbations == 2 and aco.perturbation_params == {"max_iterations": 5}
    # heuristic_dist is the reference's cached property with the reference's formula, whatever use_nls says
    assert aco.heuristic_dist.dtype == torch.float32 and torch.equal(aco.heuristic_dist, rec["heuristic_dist"])
    assert aco.heuristic_dist is aco.heuristic_dist


def test_local_search_parameter_rule():
    """env.local_search(td, actions, max_iterations=1000, num_threads=...): any other key is a TypeError."""
    from rl4co_amd import AntSystem

    assert AntSystem._max_iterations({}, "local_search_params") == 1000
    assert AntSystem._max_iterations({"max_iterations": 5, "num_threads": 4}, "perturbation_params") == 5
    with pytest.raises(TypeError, match="depth.*perturbation_params"):
        AntSystem._max_iterations({"max_iterations": 5, "depth": 3}, "perturbation_params")
