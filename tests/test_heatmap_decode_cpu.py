"""Greedy and top-k / top-p decoding of a heatmap, the parts that need no GPU: the options struct across header, ctypes and
compiler, the host checks of the five *_opts entry points, ``filter_f64`` against the reference's recorded ``process_logits``
on heatmap rows with masks, the recorded ``NARGNNPolicy`` rollouts against the float64 restatement, ``NARGNNPolicy``'s
refusals (before the encoder runs), the ``strict=True`` load of a reference state dict and the pinned signature of
``heatmap_rollout``."""
import ctypes
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from rl4co_amd import _lib
from tests import heatmap_decode_ref as H
from tests.topkp_ref import filter_f64

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "rl4co_amd.h").read_text()
DUMMY = 0x1000  # a non-NULL pointer the host checks never read through
SYMBOLS = {"rl4co_aco_tsp_opts": _lib.AcoTspArgs, "rl4co_aco_cvrp_opts": _lib.AcoCvrpArgs, "rl4co_aco_prize_opts": _lib.AcoPrizeArgs,
           "rl4co_aco_tsp_logp_grad_opts": _lib.AcoTspGradArgs, "rl4co_aco_depot_logp_grad_opts": _lib.AcoDepotGradArgs}


# ---- the options struct and the five symbols ---------------------------------------------------------------------------------------
def test_header_ctypes_and_symbols_agree():
    body = re.search(r"typedef struct rl4co_heatmap_decode_opts \{(.*?)\} rl4co_heatmap_decode_opts;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = re.findall(r"(\w+)\s+(\w+)\s*;", body)
    assert decls == [("int32_t", "greedy"), ("int32_t", "top_k"), ("float", "top_p"), ("int32_t", "reserved0")]
    assert [f[0] for f in _lib.HeatmapDecodeOpts._fields_] == [d[1] for d in decls]
    assert [f[1] for f in _lib.HeatmapDecodeOpts._fields_] == [ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_int32]
    for symbol, args in SYMBOLS.items():
        restype, argtypes = _lib.SYMBOLS[symbol]
        assert restype is ctypes.c_int
        assert argtypes == [ctypes.POINTER(args), ctypes.POINTER(_lib.HeatmapDecodeOpts), ctypes.c_void_p]
        assert re.search(r"^int %s\(const \w+\* args, const rl4co_heatmap_decode_opts\* opts,\s+void\* stream\);" % symbol,
                         HEADER, re.M), symbol
        assert getattr(_lib.lib(), symbol) is not None
    assert int(re.search(r"#define RL4CO_ABI_VERSION (\d+)", HEADER).group(1)) == _lib.ABI_VERSION == _lib.lib().rl4co_abi_version()
    assert _lib.ABI_VERSION >= 29


def test_struct_layout_is_the_compilers(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "rl4co_amd.h"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(rl4co_heatmap_decode_opts));']
    lines += [f'  printf("{f} %zu\\n", offsetof(rl4co_heatmap_decode_opts, {f}));' for f, _ in _lib.HeatmapDecodeOpts._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    table = dict(row.split() for row in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(table["sizeof"]) == ctypes.sizeof(_lib.HeatmapDecodeOpts) == 16
    for f, _ in _lib.HeatmapDecodeOpts._fields_:
        assert int(table[f]) == getattr(_lib.HeatmapDecodeOpts, f).offset, f


def _tsp_args(**over):
    a = _lib.AcoTspArgs()
    a.B, a.N, a.n_ants, a.iterations, a.phases = 4, 20, 8, 1, _lib.ACO_SAMPLE
    a.alpha, a.beta, a.decay, a.Q, a.temperature = 1.0, 1.0, 0.95, 0.1, 1.0
    for f in ("log_heuristic", "pheromone", "locs", "start_nodes", "actions", "reward", "logps", "err"):
        setattr(a, f, DUMMY)
    for k, v in over.items():
        setattr(a, k, v)
    return a


REFUSED = [(dict(greedy=2), {}, b"o->greedy == 0 || o->greedy == 1"), (dict(greedy=-1), {}, b"o->greedy == 0 || o->greedy == 1"),
           (dict(top_k=-1), {}, b"o->top_k >= 0"), (dict(top_p=-0.1), {}, b"o->top_p >= 0.0f && o->top_p <= 1.0f"),
           (dict(top_p=1.5), {}, b"o->top_p >= 0.0f && o->top_p <= 1.0f"), (dict(reserved0=1), {}, b"o->reserved0 == 0"),
           (dict(greedy=1), dict(ln_noise=DUMMY), b"o->greedy != 0 && ln_noise != nullptr")]


@pytest.mark.parametrize("opts,args,text", REFUSED)
def test_host_checks_refuse_before_any_launch(opts, args, text):
    handle = _lib.lib()
    st = handle.rl4co_aco_tsp_opts(ctypes.byref(_tsp_args(**args)), ctypes.byref(_lib.HeatmapDecodeOpts(**opts)), None)
    assert st == 1 and text in handle.rl4co_last_error()


def test_every_symbol_refuses_a_null_or_bad_options_struct():
    handle = _lib.lib()
    for symbol, args in SYMBOLS.items():
        a = _tsp_args() if args is _lib.AcoTspArgs else args()
        assert getattr(handle, symbol)(ctypes.byref(a), None, None) == 1, symbol
    g = _lib.AcoTspGradArgs()
    g.B, g.N, g.n_ants, g.row_split, g.temperature = 1, 5, 1, 1, 1.0
    for f in ("heatmap", "actions", "grad_ll", "grad_heatmap", "err"):
        setattr(g, f, DUMMY)
    st = handle.rl4co_aco_tsp_logp_grad_opts(ctypes.byref(g), ctypes.byref(_lib.HeatmapDecodeOpts(top_k=-3)), None)
    assert st == 1 and b"o->top_k >= 0" in handle.rl4co_last_error()


def test_binding_options_are_normalised_by_decoding_filter():
    from rl4co_amd import kernels as K

    assert K.heatmap_decode_opts(False, 0, 0.0, 20) is None and K.heatmap_decode_opts(False, 20, 1.0, 20) is None
    o = K.heatmap_decode_opts(True, 25, 0.5, 20)
    assert (o.greedy, o.top_k, o.top_p, o.reserved0) == (1, 0, 0.5, 0)
    with pytest.raises(AssertionError, match=r"top-p should be in \(0, 1\]"):
        K.heatmap_decode_opts(False, 0, 1.5, 20)


# ---- filter_f64 once more against the reference's process_logits, on heatmap rows with masks --------------------------------------
def test_filter_f64_is_the_references_process_logits_on_masked_heatmap_rows():
    rec = H.process_logits_record()
    logits, mask = rec["logits"], rec["mask"]
    assert len(H.PROCESS_CASES) >= 6
    for i, (k, p, t) in enumerate(H.PROCESS_CASES):
        z = logits.masked_fill(~mask, float("-inf")) / t
        assert torch.equal(filter_f64(z, k, p), rec[f"kept{i}"]), (k, p, t)
    assert not torch.equal(rec["kept1"], rec["kept0"]) and bool((rec["kept0"].sum(-1) >= 1).all())


# ---- the recorded reference rollouts against the float64 restatement -------------------------------------------------------------
def _record_data(env, rec):
    if env == "tsp":
        return {"locs": rec["locs"]}
    return {"locs": rec["locs"], "demand": rec["demand"], "vehicle_capacity": rec["vehicle_capacity"]}


@pytest.mark.parametrize("env", list(H.RECORD_ENVS))
def test_recorded_greedy_rollouts_are_the_float64_greedy_rollout(env):
    val, test = H.record(env, "val"), H.record(env, "test")
    assert torch.equal(val["heatmap"], test["heatmap"]) and torch.equal(val["start_nodes"], test["start_nodes"])
    b, n, _ = val["heatmap"].shape
    ants = val["start_nodes"].numel() // b
    want = H.greedy_rollout(env, val["heatmap"], _record_data(env, val), ants, val["start_nodes"])
    w = val["actions"].shape[1]
    assert torch.equal(want[:, :w], val["actions"]) and bool((want[:, w:] == 0).all())
    # phase="test" with select_best: the best row of every instance (ant-major rows)
    best = val["reward"].view(ants, b).t().max(-1)[1]
    rows = best * b + torch.arange(b)
    assert torch.equal(test["reward"], val["reward"][rows]) and torch.equal(test["log_likelihood"], val["log_likelihood"][rows])
    assert torch.equal(test["actions"], val["actions"][rows][:, : test["actions"].shape[1]])


@pytest.mark.parametrize("env", list(H.RECORD_ENVS))
@pytest.mark.parametrize("case", ["k3", "k5_p08"])
def test_recorded_filtered_rollouts_stay_inside_filter_f64s_kept_sets(env, case):
    rec = H.record(env, case)
    kw = H.RECORD_CASES[case]
    n = rec["heatmap"].shape[1]
    actions = torch.nn.functional.pad(rec["actions"], (0, H.width(env, n) - rec["actions"].shape[1]))
    starts = rec["start_nodes"]
    assert torch.equal(actions[:, 0], starts)
    cur, infeasible, live = H.step_table(env, rec["heatmap"], _record_data(env, rec), actions, starts if env == "cvrp" else None)
    kept, _ = H.kept_sets(H.step_logits(rec["heatmap"], cur, infeasible, 1.0), kw["top_k"], kw.get("top_p", 0.0))
    taken = kept.gather(2, actions[:, :, None]).squeeze(2)
    assert bool(taken[live].all())
    assert int(kept[live].sum(-1).max()) <= kw["top_k"]  # (the recorded heatmaps hold no ties at the k-th value)
    lp64, _ = H.filtered_logp_grad(rec["heatmap"], actions, cur, live, kept, torch.ones(actions.shape[0]))
    assert float((lp64.sum(1) - rec["log_likelihood"].double()).abs().max()) <= 1e-4


# ---- NARGNNPolicy ----------------------------------------------------------------------------------------------------------------------
class _Never(torch.nn.Module):
    def forward(self, td):
        raise AssertionError("the encoder ran before the refusal")


def test_policy_is_exported_with_the_references_constructor():
    import rl4co_amd
    from rl4co_amd import nargnn

    assert "NARGNNPolicy" in rl4co_amd.__all__ and rl4co_amd.NARGNNPolicy is nargnn.NARGNNPolicy
    sig = inspect.signature(nargnn.NARGNNPolicy.__init__)
    assert list(sig.parameters)[1:] == ["encoder", "decoder", "embed_dim", "env_name", "init_embedding", "edge_embedding",
                                        "graph_network", "heatmap_generator", "num_layers_heatmap_generator",
                                        "num_layers_graph_encoder", "act_fn", "agg_fn", "linear_bias", "train_decode_type",
                                        "val_decode_type", "test_decode_type", "constructive_policy_kw"]
    p = nargnn.NARGNNPolicy()
    assert (p.train_decode_type, p.val_decode_type, p.test_decode_type) == ("multistart_sampling", "multistart_greedy",
                                                                           "multistart_greedy")
    assert type(p.encoder) is nargnn.TrainableNARGNNEncoder
    for env in ("cvrp", "op", "pctsp"):
        assert type(nargnn.NARGNNPolicy(env_name=env).encoder) is nargnn.TrainableNARGNNDepotEncoder


REFUSALS = [
    ("tsp", dict(phase="val", tanh_clipping=10.0), "tanh_clipping"),
    ("tsp", dict(phase="val", mask_logits=False), "mask_logits=False"),
    ("tsp", dict(phase="val", return_entropy=True), "return_entropy"),
    ("tsp", dict(phase="test", decode_type="beam_search"), "beam_search"),
    ("tsp", dict(phase="test", decode_type="greedy"), "serves tsp with multistart"),
    ("tsp", dict(phase="val", beam_width=4), "beam_width"),
    ("tsp", dict(phase="predict"), "phase"),
    ("op", dict(phase="val"), r"decoding_kwargs\['multistart'\] is not served for op: every ant starts at the depot"),
    ("pctsp", dict(phase="test"), r"decoding_kwargs\['multistart'\] is not served for pctsp: every ant starts at the depot"),
    ("cvrp", dict(phase="val"), "runs inside the MI355X kernels only"),  # CPU tensors
]


@pytest.mark.parametrize("env,kw,text", REFUSALS)
def test_policy_refusals_come_before_the_encoder_runs(env, kw, text):
    from rl4co_amd import NARGNNPolicy

    policy = NARGNNPolicy(encoder=_Never(), env_name=env)
    td = {"locs": torch.rand(2, 6, 2)}
    with pytest.raises(NotImplementedError, match=text):
        policy(td, **kw)
    with pytest.raises(AssertionError, match=r"top-p should be in \(0, 1\]"):
        policy(td, phase="val", top_p=1.5)


def test_policy_constructor_refusals():
    from rl4co_amd import NARGNNPolicy

    with pytest.raises(NotImplementedError, match="decoder"):
        NARGNNPolicy(decoder=torch.nn.Identity())
    with pytest.raises(NotImplementedError, match="env_name"):
        NARGNNPolicy(env_name="pdp")


@pytest.mark.parametrize("env", H.ENVS)
def test_a_reference_state_dict_loads_strictly(env):
    from rl4co_amd import NARGNNPolicy

    shapes = H.recorded_state_dict_shapes()[env]
    g = torch.Generator().manual_seed(3)
    sd = {k: (torch.zeros(s, dtype=torch.int64) if k.endswith("num_batches_tracked") else torch.rand(*s, generator=g))
          for k, s in shapes.items()}
    policy = NARGNNPolicy(env_name=env)
    assert list(policy.state_dict().keys()) == list(shapes)
    policy.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in policy.state_dict().items())


def test_heatmap_rollout_keeps_its_signature_and_heatmap_decode_adds_the_options():
    from rl4co_amd.aco import heatmap_decode, heatmap_rollout

    assert str(inspect.signature(heatmap_rollout)) == ("(heatmap: 'Tensor', locs: 'Tensor', *, n_ants: 'int', start_nodes: "
                                                       "'Tensor | None' = None, actions: 'Tensor | None' = None, temperature: "
                                                       "'float' = 1.0, seed: 'int | None' = None, err: 'Tensor | None' = None, "
                                                       "env_name: 'str' = 'tsp', td=None) -> 'dict'")
    extra = [p for p in inspect.signature(heatmap_decode).parameters if p not in inspect.signature(heatmap_rollout).parameters]
    assert extra == ["decode_type", "top_k", "top_p"]
    d = inspect.signature(heatmap_decode).parameters
    assert (d["decode_type"].default, d["top_k"].default, d["top_p"].default) == ("sampling", 0, 0.0)
    with pytest.raises(NotImplementedError, match="decode_type"):
        heatmap_decode(torch.zeros(1, 3, 3), torch.zeros(1, 3, 2), n_ants=1, decode_type="beam_search")
    with pytest.raises(NotImplementedError, match="MI355X"):
        heatmap_decode(torch.zeros(1, 3, 3), torch.zeros(1, 3, 2), n_ants=1, decode_type="greedy")
