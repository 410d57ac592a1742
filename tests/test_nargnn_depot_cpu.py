"""DeepACO's heatmap encoder for the depot graphs (CVRP, OP, PCTSP) without a GPU: the edge-list restatement
(tests/nargnn_depot_ref.py) against the records of the reference's own NARGNNEncoder(env_name=...), the module's
``state_dict`` keys against the reference's recorded lists, DeepACOPolicy's choice of encoder, the C boundary of
``rl4co_nargnn_depot_heatmap``, and every refusal of the binding and of the encoder."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from tests import nargnn_depot_ref as R

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "rl4co_amd.h").read_text()
ENVS = ("cvrp", "op", "pctsp")


# ---- 1. the restatement against the records -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_matches_the_recorded_reference(case):
    rec = R.record(case)
    env, n, k_sparse, layers, mlp_layers, wseed, _ = R.CASES[case]
    sd = R.case_state_dict(case)
    assert R.state_hash(sd) == bytes(rec["weights_sha256"].tolist()).hex() and int(rec["weight_seed"]) == wseed
    if case in R.STORES_STATE_DICT:
        stored = {k[3:]: v for k, v in rec.items() if k.startswith("sd/")}
        assert sorted(stored) == sorted(sd) and all(torch.equal(stored[k], sd[k]) for k in sd)
    assert R.count_layers(sd) == (layers, mlp_layers)
    locs, feats = rec["locs"], rec["feats"]
    assert feats.shape == (R.BATCH, n - 1, R.FEATURES[env])
    nbr_ref = R.edge_index_to_neighbors(rec["edge_index"], R.BATCH, n)  # (asserts the reference's edge order)
    assert nbr_ref.shape == (R.BATCH, n - 1, R.num_neighbors(n, k_sparse))
    assert rec["edge_index"].shape[1] == R.BATCH * (n - 1) * (nbr_ref.shape[2] + 2)
    # the graph: fp32 and fp64 select the same neighbour set per customer, finite entries exactly on it
    nbr32, _, _ = R.select_neighbors(locs, nbr_ref.shape[2])
    nbr64, _, _ = R.select_neighbors(locs.double(), nbr_ref.shape[2])
    assert torch.equal(nbr32.sort(-1).values, nbr_ref.sort(-1).values) and torch.equal(nbr64.sort(-1).values, nbr_ref.sort(-1).values)
    on = R.on_graph(nbr_ref, n)
    assert int(on.sum()) == rec["edge_index"].shape[1] and bool(on[:, 0, 1:].all()) and bool(on[:, 1:, 0].all())
    assert not bool(on.diagonal(dim1=1, dim2=2).any())
    got32, embed32 = R.encode(sd, locs, feats, k_sparse, torch.float32)
    fill = torch.log(torch.tensor(R.SMALL))
    for heat in (rec["heatmap32"], got32):
        assert torch.equal(heat[~on], fill.expand(int((~on).sum()))) and bool((heat[on] > fill).all())
    # float64 against float64, then float32 within twice the reference's own float32 error
    got64, _ = R.encode(sd, locs, feats, k_sparse, torch.float64, neighbors=nbr_ref)
    assert float((got64 - rec["heatmap64"])[on].abs().max()) <= 1e-12
    floor = R.floor32(rec)
    assert 0 < floor < 1e-5
    err = float((got32.double() - rec["heatmap64"])[on].abs().max())
    print(f"{case}: reference fp32 floor {floor:.3e}, restatement fp32 error {err:.3e} ({err / floor:.2f} x)")
    assert err <= 2 * floor
    # node_embed: (2 + F) products and as many additions, every value below 4: 2 (2 + F) roundings of 2^-23 at the most
    assert torch.allclose(embed32, rec["node_embed32"], rtol=0, atol=2 * (2 + R.FEATURES[env]) * 2.0 ** -23)


# ---- 2. the module tree -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ENVS)
def test_state_dict_keys_are_the_reference_s_and_the_strict_load_passes(env):
    from rl4co_amd import NARGNNDepotEncoder

    enc = NARGNNDepotEncoder(env_name=env)
    assert list(enc.state_dict().keys()) == R.recorded_keys()[env]
    sd = R.make_state_dict(env, 5, 15, 5)
    assert sorted(sd) == sorted(R.recorded_keys()[env])
    enc.load_state_dict(sd, strict=True)
    assert enc.init_embedding.init_embed.weight.shape == (64, 2 + R.FEATURES[env])
    assert enc.init_embedding.init_embed_depot.weight.shape == (64, 2) and enc.edge_embedding.edge_embed.weight.shape == (64, 1)
    small = NARGNNDepotEncoder(env_name=env, num_layers_graph_encoder=1, num_layers_heatmap_generator=2)
    small.load_state_dict(R.make_state_dict(env, 6, 1, 2), strict=True)
    got, want = small.eval().packed_parameters("cpu"), R.kernel_parameters(R.make_state_dict(env, 6, 1, 2), "cpu")
    assert sorted(got) == sorted(want)
    for key in want:
        assert (got[key] is None and want[key] is None) or torch.equal(got[key], want[key].reshape(got[key].shape)), key
    with pytest.raises(RuntimeError):
        small.load_state_dict(sd, strict=True)


def test_lazy_export_and_policy_builds_the_right_encoder():
    import rl4co_amd
    from rl4co_amd import DeepACOPolicy, NARGNNDepotEncoder, NARGNNEncoder, nargnn

    assert rl4co_amd.NARGNNDepotEncoder is nargnn.NARGNNDepotEncoder and issubclass(NARGNNDepotEncoder, NARGNNEncoder)
    for env in ENVS:
        pol = DeepACOPolicy(env_name=env, num_layers_graph_encoder=1, n_ants=8)
        assert type(pol.encoder) is NARGNNDepotEncoder and pol.encoder.env_name == env
        assert len(pol.encoder.graph_network.layers) == 1
        assert pol.decode_type == "sampling" and pol.default_decoding_kwargs == {"select_best": False, "multisample": True}
    multi = DeepACOPolicy(env_name="cvrp", multistart=True, num_layers_graph_encoder=0)
    assert type(multi.encoder) is NARGNNDepotEncoder and multi.decode_type == "multistart_sampling"
    assert multi.default_decoding_kwargs["multistart"] is True and "select_start_nodes_fn" in multi.default_decoding_kwargs
    tsp = DeepACOPolicy(num_layers_graph_encoder=0)
    assert type(tsp.encoder) is NARGNNEncoder and tsp.decode_type == "multistart_sampling"
    assert type(DeepACOPolicy(env_name="spctsp", num_layers_graph_encoder=0).encoder) is NARGNNEncoder  # out of scope: refused at forward


# ---- 3. the C boundary --------------------------------------------------------------------------------------------------------
def test_header_ctypes_and_symbols_agree():
    from rl4co_amd import _lib

    assert int(re.search(r"#define RL4CO_ABI_VERSION (\d+)", HEADER).group(1)) >= 23 and _lib.ABI_VERSION >= 23
    body = re.search(r"typedef struct rl4co_nargnn_depot_args \{(.*?)\} rl4co_nargnn_depot_args;", HEADER, re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.NargnnDepotArgs._fields_]
    assert ctypes.sizeof(_lib.NargnnDepotArgs) == 10 * 4 + 23 * 8
    for name in ("rl4co_nargnn_depot_heatmap", "rl4co_nargnn_depot_lds_nodes", "rl4co_nargnn_depot_scratch_bytes"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, HEADER)
    handle = _lib.lib()
    assert handle.rl4co_abi_version() == _lib.ABI_VERSION
    # the tiers: 272-byte rows, 64 bytes of head, 64 of static allowance, 160 KiB; 2 N node rows and (N - 1)(K + 2) edge rows
    def lds(n, k):
        return 64 + 272 * (2 * n + (n - 1) * (k + 2)) + 64

    for k in (1, 10, 14, 15, 16, 20, 40, 256):
        n = handle.rl4co_nargnn_depot_lds_nodes(k)
        assert lds(n, k) <= 160 * 1024 < lds(n + 1, k), k
    assert handle.rl4co_nargnn_depot_lds_nodes(10) == 43 and handle.rl4co_nargnn_depot_lds_nodes(20) == 25
    assert handle.rl4co_nargnn_depot_lds_nodes(0) == 0
    from rl4co_amd import kernels as K

    assert K.nargnn_depot_lds_nodes(10) == 43
    # the scratch: x, x1, x3 and the eight depot partials always; the edge rows above the LDS tier; x2, x4 above 300 nodes
    assert handle.rl4co_nargnn_depot_scratch_bytes(43, 10) == 272 * (3 * 43 + 8)
    assert handle.rl4co_nargnn_depot_scratch_bytes(44, 10) == 272 * (3 * 44 + 8 + 43 * 12)
    assert handle.rl4co_nargnn_depot_scratch_bytes(300, 10) == 272 * (3 * 300 + 8 + 299 * 12)
    assert handle.rl4co_nargnn_depot_scratch_bytes(301, 10) == 272 * (5 * 301 + 8 + 300 * 12)
    assert handle.rl4co_nargnn_depot_scratch_bytes(1024, 256) == 272 * (5 * 1024 + 8 + 1023 * 258)
    for n, k in ((2, 1), (1025, 10), (12, 11), (300, 257)):
        assert handle.rl4co_nargnn_depot_scratch_bytes(n, k) == 0
    # arguments are checked on the host before any launch
    args = _lib.NargnnDepotArgs()
    assert handle.rl4co_nargnn_depot_heatmap(ctypes.byref(args), None) == 1 and b"requirement failed" in handle.rl4co_last_error()
    args.D, args.B, args.N, args.K, args.F, args.H, args.n_workgroups = 32, 1, 12, 10, 1, 1, 1
    assert handle.rl4co_nargnn_depot_heatmap(ctypes.byref(args), None) == 1 and b"a.D == kD" in handle.rl4co_last_error()
    args.D = 64
    for n, k, why in ((2, 1, b"a.N >= 3"), (1025, 10, b"a.N >= 3"), (12, 11, b"a.K <= a.N - 2")):
        args.N, args.K = n, k
        assert handle.rl4co_nargnn_depot_heatmap(ctypes.byref(args), None) == 1 and why in handle.rl4co_last_error(), (n, k)
    args.N, args.K, args.F = 12, 10, 3
    assert handle.rl4co_nargnn_depot_heatmap(ctypes.byref(args), None) == 1 and b"a.F == 1" in handle.rl4co_last_error()


# ---- 4. the refusals ------------------------------------------------------------------------------------------------------------
def test_kernel_binding_refusals():
    from rl4co_amd import _lib
    from rl4co_amd import kernels as K

    p = R.kernel_parameters(R.case_state_dict("cvrp_n12"), "cpu")

    def call(n=12, k=10, f=1, **over):
        c = n - 1
        return K.nargnn_depot_heatmap(torch.rand(2, n, 2), torch.rand(2, c, f), torch.ones(2, c, k, dtype=torch.int32),
                                      torch.rand(2, c, k), torch.rand(2, c), **{**p, **over})

    with pytest.raises(NotImplementedError, match="embed_dim = 64"):
        call(init_w=torch.rand(32, 3))
    with pytest.raises(NotImplementedError, match="K <= min"):
        call(n=12, k=11)  # K = C
    with pytest.raises(NotImplementedError, match="3 <= N <= 1024"):
        call(n=1025, k=10)
    with pytest.raises(NotImplementedError, match="3 <= N <= 1024"):
        call(n=2, k=1)
    with pytest.raises(NotImplementedError, match="F = 1 or 2"):
        call(f=3, init_w=torch.rand(64, 5))
    with pytest.raises(ValueError, match="init_w"):
        call(f=2)  # the customers' linear is [64, 3]
    with pytest.raises(ValueError, match="depot_w"):
        call(depot_w=torch.rand(64, 3))
    with pytest.raises(ValueError, match="lin_b"):
        call(lin_b=torch.rand(1, 4, 64))
    locs, feats, nbr = torch.rand(2, 12, 2), torch.rand(2, 11, 1), torch.ones(2, 11, 10, dtype=torch.int32)
    with pytest.raises(ValueError, match="feats"):
        K.nargnn_depot_heatmap(locs, torch.rand(2, 12, 1), nbr, torch.rand(2, 11, 10), torch.rand(2, 11), **p)
    with pytest.raises(ValueError, match="neighbors"):
        K.nargnn_depot_heatmap(locs, feats, torch.ones(2, 12, 10, dtype=torch.int32), torch.rand(2, 11, 10), torch.rand(2, 11), **p)
    with pytest.raises(ValueError, match="edge_cost"):
        K.nargnn_depot_heatmap(locs, feats, nbr, torch.rand(2, 11, 9), torch.rand(2, 11), **p)
    with pytest.raises(ValueError, match="depot_cost"):
        K.nargnn_depot_heatmap(locs, feats, nbr, torch.rand(2, 11, 10), torch.rand(2, 12), **p)
    with pytest.raises(_lib.Rl4coLibraryError, match="no CPU fallback"):
        call()


def _td(env, n=12, b=2):
    locs, feats = R.make_instance(env, b, n, 1)
    return R.td_of(env, locs, feats)


@pytest.mark.parametrize("env", ENVS)
def test_encoder_refusals(env):
    from rl4co_amd import NARGNNDepotEncoder, NARGNNEncoder

    with pytest.raises(NotImplementedError, match="inference only"):
        NARGNNDepotEncoder(env_name=env, num_layers_graph_encoder=1)(_td(env))
    with pytest.raises(NotImplementedError, match="rl4co_nargnn_depot_heatmap\\) only: td\\['locs'\\] on cpu"):
        NARGNNDepotEncoder(env_name=env, num_layers_graph_encoder=1).eval()(_td(env))
    for kw, why in ((dict(act_fn="relu"), "act_fn='silu'"), (dict(agg_fn="max"), "agg_fn='mean'"),
                    (dict(embed_dim=32), "embed_dim=64"), (dict(graph_network=torch.nn.Identity()), "custom graph_network"),
                    (dict(heatmap_generator=torch.nn.Identity()), "custom heatmap_generator"),
                    (dict(init_embedding=torch.nn.Identity()), "custom init_embedding"),
                    (dict(edge_embedding=torch.nn.Identity()), "custom edge_embedding")):
        with pytest.raises(NotImplementedError, match=why):
            NARGNNDepotEncoder(env_name=env, num_layers_graph_encoder=1, **kw).eval()(_td(env))
    for other in ("tsp", "spctsp"):
        with pytest.raises(NotImplementedError, match="cvrp / op / pctsp environment only"):
            NARGNNDepotEncoder(env_name=other, num_layers_graph_encoder=1).eval()(_td(env))
    # the regular-graph class keeps refusing these environments, and names the class that serves them
    with pytest.raises(NotImplementedError, match="tsp environment only .*NARGNNDepotEncoder"):
        NARGNNEncoder(env_name=env, num_layers_graph_encoder=1).eval()(_td(env))


def test_module_neighbour_selection_is_the_reference_s():
    from rl4co_amd import NARGNNDepotEncoder

    for case in R.CASES:
        env, n, k_sparse, _, _, _, _ = R.CASES[case]
        rec = R.record(case)
        enc = NARGNNDepotEncoder(env_name=env, num_layers_graph_encoder=0, k_sparse=k_sparse)
        nbr, cost, depot_cost = enc.neighbors(rec["locs"])
        want = R.edge_index_to_neighbors(rec["edge_index"], R.BATCH, n)
        assert nbr.dtype == torch.int32 and torch.equal(nbr.long().sort(-1).values, want.sort(-1).values)
        dist = R.distances(rec["locs"])
        assert torch.equal(cost, dist[:, 1:].gather(2, nbr.long())) and torch.equal(depot_cost, dist[:, 1:, 0])


# ---- 5. the recorder itself (needs the reference checkout) ---------------------------------------------------------------------
def test_recorder_reproduces_a_record():
    from oracle import ref_import

    if not ref_import.available():
        pytest.skip("the reference checkout is not here")
    rec, again = R.record("cvrp_n12"), R.reference_run("cvrp_n12")
    for key in ("locs", "feats", "edge_index", "heatmap32", "heatmap64"):
        assert torch.equal(rec[key], torch.as_tensor(again[key])), key
    assert R.reference_keys() == R.recorded_keys()
