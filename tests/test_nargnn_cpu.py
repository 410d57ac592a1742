"""DeepACO's heatmap encoder without a GPU: the dense restatement (tests/nargnn_ref.py) against the records of the
reference's own NARGNNEncoder, the module's ``state_dict`` keys against the reference's recorded list, the C boundary of
``rl4co_nargnn_heatmap``, and every refusal of the encoder and of DeepACOPolicy."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from tests import nargnn_ref as R

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "rl4co_amd.h").read_text()


# ---- 1. the restatement against the records -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_matches_the_recorded_reference(case):
    rec = R.record(case)
    n, k_sparse, layers, mlp_layers, wseed, _ = R.CASES[case]
    sd = R.case_state_dict(case)
    assert R.state_hash(sd) == bytes(rec["weights_sha256"].tolist()).hex() and int(rec["weight_seed"]) == wseed
    if case in R.STORES_STATE_DICT:
        stored = {k[3:]: v for k, v in rec.items() if k.startswith("sd/")}
        assert sorted(stored) == sorted(sd) and all(torch.equal(stored[k], sd[k]) for k in sd)
    assert R.count_layers(sd) == (layers, mlp_layers)
    locs = rec["locs"]
    nbr_ref = R.edge_index_to_neighbors(rec["edge_index"], R.BATCH, n)
    assert nbr_ref.shape[2] == R.num_neighbors(n, k_sparse)
    # the graph: the same neighbour set per node, finite entries exactly on it
    got32, embed32, nbr, _ = R.encode(sd, locs, k_sparse, torch.float32, return_edges=True)
    assert torch.equal(nbr.sort(-1).values, nbr_ref.sort(-1).values)
    on = torch.zeros(R.BATCH, n, n, dtype=torch.bool).scatter_(2, nbr_ref, True)
    fill = torch.log(torch.tensor(R.SMALL))
    for heat in (rec["heatmap32"], got32):
        assert torch.equal(heat[~on], fill.expand(int((~on).sum()))) and bool((heat[on] > fill).all())
    # float64 against float64, then float32 within twice the reference's own float32 error
    got64, _ = R.encode(sd, locs, k_sparse, torch.float64, neighbors=nbr_ref)
    assert float((got64 - rec["heatmap64"])[on].abs().max()) <= 1e-10
    floor = R.floor32(rec)
    assert 0 < floor < 1e-5
    err = float((got32.double() - rec["heatmap64"])[on].abs().max())
    print(f"{case}: reference fp32 floor {floor:.3e}, restatement fp32 error {err:.3e} ({err / floor:.2f} x)")
    assert err <= 2 * floor
    assert torch.allclose(embed32, rec["node_embed32"], rtol=0, atol=4 * 2.0 ** -24 * 3)


# ---- 2. the module tree -----------------------------------------------------------------------------------------------------
def test_state_dict_keys_are_the_reference_s_and_the_strict_load_passes():
    from rl4co_amd import NARGNNEncoder

    enc = NARGNNEncoder()
    assert list(enc.state_dict().keys()) == R.recorded_keys()
    sd = R.case_state_dict("n20_full")
    assert sorted(sd) == sorted(R.recorded_keys())
    enc.load_state_dict(sd, strict=True)
    small = NARGNNEncoder(num_layers_graph_encoder=1, num_layers_heatmap_generator=2)
    small.load_state_dict(R.case_state_dict("n11"), strict=True)
    nobias = NARGNNEncoder(num_layers_graph_encoder=1, num_layers_heatmap_generator=3, linear_bias=False)
    assert sorted(nobias.state_dict()) == sorted(R.make_state_dict(1, 1, 3, linear_bias=False))
    with pytest.raises(RuntimeError):
        small.load_state_dict(sd, strict=True)


def test_packed_parameters_fold_the_batch_norms():
    from rl4co_amd import NARGNNEncoder

    sd = R.case_state_dict("n50")
    enc = NARGNNEncoder(num_layers_graph_encoder=3, num_layers_heatmap_generator=3).eval()
    enc.load_state_dict(sd, strict=True)
    got, want = enc.packed_parameters("cpu"), R.kernel_parameters(sd, "cpu")
    assert sorted(got) == sorted(want)
    for key in want:
        assert (got[key] is None and want[key] is None) or torch.equal(got[key], want[key].reshape(got[key].shape)), key
    assert got["lin_w"].shape == (3, 5, 64, 64) and got["bn"].shape == (3, 2, 2, 64) and got["mlp_w"].shape == (2, 64, 64)
    assert enc.packed_parameters("cpu") is got  # cached until a parameter changes
    with torch.no_grad():
        enc.graph_network.layers[0].v_bn.module.running_var.add_(1.0)
    assert not torch.equal(enc.packed_parameters("cpu")["bn"], got["bn"])
    y = torch.randn(5, 64)
    bn = enc.graph_network.layers[1].e_bn.module
    folded = enc.packed_parameters("cpu")["bn"][1, 1]
    assert torch.allclose(bn(y), y * folded[0] + folded[1], atol=1e-5)


def test_lazy_exports():
    import rl4co_amd
    from rl4co_amd import nargnn

    assert rl4co_amd.NARGNNEncoder is nargnn.NARGNNEncoder and rl4co_amd.DeepACOPolicy is nargnn.DeepACOPolicy


# ---- 3. the C boundary --------------------------------------------------------------------------------------------------------
def test_header_ctypes_and_symbols_agree():
    from rl4co_amd import _lib

    assert int(re.search(r"#define RL4CO_ABI_VERSION (\d+)", HEADER).group(1)) >= 21 and _lib.ABI_VERSION >= 21
    body = re.search(r"typedef struct rl4co_nargnn_args \{(.*?)\} rl4co_nargnn_args;", HEADER, re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.NargnnArgs._fields_]
    assert ctypes.sizeof(_lib.NargnnArgs) == 10 * 4 + 19 * 8
    handle = _lib.lib()
    assert handle.rl4co_abi_version() == _lib.ABI_VERSION
    # the tiers: 272-byte rows, 64 bytes of head, 64 of static allowance, 160 KiB
    for k in (1, 10, 16, 17, 20, 40):
        n = handle.rl4co_nargnn_lds_nodes(k)
        assert 64 + 272 * (2 + k) * n + 64 <= 160 * 1024 < 64 + 272 * (2 + k) * (n + 1) + 64
    assert handle.rl4co_nargnn_lds_nodes(10) == 50 and handle.rl4co_nargnn_lds_nodes(0) == 0
    assert handle.rl4co_nargnn_scratch_bytes(50, 10) == 272 * 3 * 50            # edge state in LDS
    assert handle.rl4co_nargnn_scratch_bytes(51, 10) == 272 * (3 * 51 + 510)     # edge state in scratch
    assert handle.rl4co_nargnn_scratch_bytes(301, 10) == 272 * (5 * 301 + 3010)  # every plane in scratch
    assert handle.rl4co_nargnn_scratch_bytes(1025, 10) == 0
    # arguments are checked on the host before any launch
    args = _lib.NargnnArgs()
    assert handle.rl4co_nargnn_heatmap(ctypes.byref(args), None) == 1 and b"requirement failed" in handle.rl4co_last_error()
    args.D, args.B, args.N, args.K, args.H, args.n_workgroups = 32, 1, 12, 10, 1, 1
    assert handle.rl4co_nargnn_heatmap(ctypes.byref(args), None) == 1 and b"a.D == kD" in handle.rl4co_last_error()


# ---- 4. the refusals ------------------------------------------------------------------------------------------------------------
def _td(n=12, b=2):
    return {"locs": torch.rand(b, n, 2), "action_mask": torch.ones(b, n, dtype=torch.bool)}


def test_encoder_refusals():
    from rl4co_amd import NARGNNEncoder

    with pytest.raises(NotImplementedError, match="inference only"):
        NARGNNEncoder(num_layers_graph_encoder=1)(_td())
    with pytest.raises(NotImplementedError, match="td\\['locs'\\] on cpu"):
        NARGNNEncoder(num_layers_graph_encoder=1).eval()(_td())
    for kw, why in ((dict(env_name="cvrp"), "tsp environment only"), (dict(act_fn="relu"), "act_fn='silu'"),
                    (dict(agg_fn="max"), "agg_fn='mean'"), (dict(embed_dim=32), "embed_dim=64"),
                    (dict(graph_network=torch.nn.Identity()), "custom graph_network"),
                    (dict(heatmap_generator=torch.nn.Identity()), "custom heatmap_generator"),
                    (dict(init_embedding=torch.nn.Identity()), "custom init_embedding"),
                    (dict(edge_embedding=torch.nn.Identity()), "custom edge_embedding")):
        with pytest.raises(NotImplementedError, match=why):
            NARGNNEncoder(num_layers_graph_encoder=1, **kw).eval()(_td())


def test_kernel_binding_refusals():
    from rl4co_amd import kernels as K

    p = R.kernel_parameters(R.case_state_dict("n11"), "cpu")
    locs = torch.rand(2, 12, 2)

    def call(n=12, k=10, **over):
        return K.nargnn_heatmap(torch.rand(2, n, 2), torch.zeros(2, n, k, dtype=torch.int32), torch.rand(2, n, k), **{**p, **over})

    with pytest.raises(NotImplementedError, match="embed_dim = 64"):
        call(init_w=torch.rand(32, 2))
    with pytest.raises(NotImplementedError, match="K <= min"):
        call(n=12, k=12)
    with pytest.raises(NotImplementedError, match="N <= 1024"):
        call(n=1025, k=10)
    with pytest.raises(ValueError, match="edge_cost"):
        K.nargnn_heatmap(locs, torch.zeros(2, 12, 10, dtype=torch.int32), torch.rand(2, 12, 9), **p)
    with pytest.raises(ValueError, match="lin_b"):
        call(lin_b=torch.rand(1, 4, 64))
    from rl4co_amd import _lib

    with pytest.raises(_lib.Rl4coLibraryError, match="no CPU fallback"):
        call()


def test_policy_refusals_and_defaults():
    from rl4co_amd import DeepACOPolicy
    from rl4co_amd.aco import AntSystem

    with pytest.raises(NotImplementedError, match="k_sparse"):
        DeepACOPolicy(k_sparse=10)
    with pytest.raises(NotImplementedError, match="top_k"):
        DeepACOPolicy(top_k=5)
    with pytest.raises(NotImplementedError, match="top_k"):
        DeepACOPolicy(top_p=0.9)
    pol = DeepACOPolicy(n_ants=8, n_iterations=dict(test=3), num_layers_graph_encoder=1, k_sparse=None,
                        aco_kwargs=dict(alpha=0.5)).eval()
    assert pol.n_ants == dict(train=8, val=8, test=8) and pol.n_iterations == dict(train=1, val=5, test=3)
    assert DeepACOPolicy(num_layers_graph_encoder=0).n_ants == dict(train=30, val=48, test=48)
    assert pol.aco_class is AntSystem and pol.decode_type == "multistart_sampling"
    assert pol.default_decoding_kwargs["multistart"] is True and pol.default_decoding_kwargs["select_best"] is False
    assert len(pol.encoder.graph_network.layers) == 1
    with pytest.raises(NotImplementedError, match="phase='train'"):
        pol(_td(), None, phase="train")
    with pytest.raises(NotImplementedError, match="phase='train'"):
        pol(_td())
    with pytest.raises(NotImplementedError, match="on cpu"):
        pol(_td(), "tsp", phase="test")
    # select_start_node_fn is the reference's: a fixed start node for tsp, else a draw from the mask
    class Env:
        name = "tsp"

    td = _td(6, 3)
    assert torch.equal(DeepACOPolicy.select_start_node_fn(td, Env, 4, start_node=2), torch.full((12,), 2))
    td["action_mask"][:, 1:] = False
    assert torch.equal(DeepACOPolicy.select_start_node_fn(td, Env, 4), torch.zeros(12, dtype=torch.long))
    fixed = DeepACOPolicy(start_node=3, num_layers_graph_encoder=0).default_decoding_kwargs["select_start_nodes_fn"]
    assert torch.equal(fixed(td, Env, 2), torch.full((6,), 3))


# ---- 5. the recorder itself (needs the reference checkout) ---------------------------------------------------------------------
def test_recorder_reproduces_a_record():
    from oracle import ref_import

    if not ref_import.available():
        pytest.skip("the reference checkout is not here")
    rec, again = R.record("n11"), R.reference_run("n11")
    for key in ("locs", "edge_index", "heatmap32", "heatmap64"):
        assert torch.equal(rec[key], torch.as_tensor(again[key])), key
    assert list(R.reference_encoder_class()(num_layers_graph_encoder=15).state_dict().keys()) == R.recorded_keys()
