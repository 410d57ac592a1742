"""The trainable depot-graph heatmap encoder without a GPU: the edge-list train-mode restatement
(tests/nargnn_depot_train_ref.py) against the records of the reference's own ``NARGNNEncoder(env_name=...)`` in ``.train()``,
the depot graph's CSR against a brute-force loop, the module's ``state_dict`` keys and refusals, and the C boundary of
``rl4co_nargnn_depot_train_*``."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from tests import nargnn_depot_ref as R
from tests import nargnn_depot_train_ref as T

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "rl4co_amd.h").read_text()
SYMBOLS = ("rl4co_nargnn_depot_train_forward", "rl4co_nargnn_depot_train_backward", "rl4co_nargnn_depot_train_workspace_bytes")


# ---- 1. the class surface ------------------------------------------------------------------------------------------------
def test_state_dict_keys_and_strict_loads():
    import rl4co_amd
    from rl4co_amd import NARGNNDepotEncoder, TrainableNARGNNDepotEncoder, nargnn

    assert "TrainableNARGNNDepotEncoder" in rl4co_amd.__all__
    assert rl4co_amd.TrainableNARGNNDepotEncoder is nargnn.TrainableNARGNNDepotEncoder
    assert issubclass(TrainableNARGNNDepotEncoder, NARGNNDepotEncoder)
    recorded = R.recorded_keys()
    for env in R.FEATURES:
        enc = TrainableNARGNNDepotEncoder(env_name=env)
        assert list(enc.state_dict().keys()) == list(NARGNNDepotEncoder(env_name=env).state_dict().keys()) == recorded[env]
    for case, (env, _, k_sparse, layers, mlp_layers, _, _) in T.CASES.items():
        enc = TrainableNARGNNDepotEncoder(env_name=env, num_layers_graph_encoder=layers, num_layers_heatmap_generator=mlp_layers,
                                          k_sparse=k_sparse)
        enc.load_state_dict(T.case_state_dict(case), strict=True)
        assert enc.training and enc.edge_embedding.k_sparse == k_sparse


# ---- 2. the C boundary -----------------------------------------------------------------------------------------------------
def test_header_ctypes_and_symbols_agree():
    from rl4co_amd import _lib

    assert int(re.search(r"#define RL4CO_ABI_VERSION (\d+)", HEADER).group(1)) >= 27 and _lib.ABI_VERSION >= 27
    body = re.search(r"typedef struct rl4co_nargnn_depot_train_args \{(.*?)\} rl4co_nargnn_depot_train_args;", HEADER, re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.NargnnDepotTrainArgs._fields_]
    assert ctypes.sizeof(_lib.NargnnDepotTrainArgs) == 8 * 4 + 23 * 8
    handle = _lib.lib()
    assert int(re.search(r"#define RL4CO_ABI_VERSION (\d+)", HEADER).group(1)) == handle.rl4co_abi_version() == _lib.ABI_VERSION
    for name in SYMBOLS:
        assert name in _lib.SYMBOLS and getattr(handle, name) is not None
    args = _lib.NargnnDepotTrainArgs()
    for fn in (handle.rl4co_nargnn_depot_train_forward, handle.rl4co_nargnn_depot_train_backward):
        assert fn(ctypes.byref(args), None) == 1 and b"a.D == kD" in handle.rl4co_last_error()
    args.D, args.B, args.N, args.K, args.L = 64, 1, 12, 11, 1  # K = N - 1: one more than the customers' other customers
    assert handle.rl4co_nargnn_depot_train_forward(ctypes.byref(args), None) == 1 and b"a.K <= 64" in handle.rl4co_last_error()
    args.N, args.K = 2, 1
    assert handle.rl4co_nargnn_depot_train_forward(ctypes.byref(args), None) == 1 and b"a.N >=" in handle.rl4co_last_error()


def test_workspace_formula():
    from rl4co_amd import kernels as K

    def want(b, n, k, layers):  # the header's layout with E = (N - 1)(K + 2) in place of N K
        rows_v, rows_e = b * n, b * (n - 1) * (k + 2)
        nv, ne = 64 * rows_v, 64 * rows_e
        pv, pe = min(-(-rows_v // 64), 1024), min(-(-rows_e // 64), 1024)
        floats = (64 + max(layers - 1, 0) * (nv + ne) + layers * (2 * nv + ne) + 5 * nv + 2 * ne + 192 * (pv + pe)
                  + 4160 * (4 * pv + pe) + 512)
        return 4 * floats

    for shape in ((3, 21, 10, 15), (128, 101, 20, 15), (1, 3, 1, 1), (1, 1024, 10, 1)):
        assert K.nargnn_depot_train_workspace_bytes(*shape) == want(*shape), shape
    for shape in ((0, 12, 10, 1), (1, 2, 1, 1), (1, 1025, 10, 1), (1, 12, 11, 1), (1, 100, 65, 1), (1, 12, 10, 0), (4096, 1024, 64, 1)):
        assert K.nargnn_depot_train_workspace_bytes(*shape) == 0, shape


# ---- 3. the CSR ------------------------------------------------------------------------------------------------------------
def test_depot_csr_equals_the_brute_force_loop():
    from rl4co_amd import kernels as K

    gen = torch.Generator().manual_seed(3)
    b, c, k = 2, 5, 2
    nbr = torch.stack([torch.stack([torch.randperm(c - 1, generator=gen)[:k] + 2 for _ in range(c)]) for _ in range(b)])
    nbr[:, :, 0] = 2  # customer 2 is in every list (its own included), customer 1 in none
    ptr, src = K.depot_incoming_csr(nbr.to(torch.int32))
    want_ptr, want_src = T.incoming_csr_bruteforce(nbr)
    assert torch.equal(ptr, want_ptr) and torch.equal(src, want_src) and ptr.dtype == src.dtype == torch.int32
    n, e = c + 1, c * (k + 2)
    degree = (ptr[1:] - ptr[:-1]).view(b, n)
    assert bool((degree[:, 0] == c).all()) and bool((degree[:, 1] == 1).all()) and bool((degree[:, 2] >= c + 1).all())
    assert int(ptr[-1]) == b * e
    for j in range(b * n):  # ascending edge rows inside a node's run
        run = src[int(ptr[j]):int(ptr[j + 1])]
        assert bool((run[1:] > run[:-1]).all())
    # the depot's incoming rows are the i -> 0 rows of its instance, in order
    assert src[:c].tolist() == list(range(c * k, c * k + c))


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals():
    from rl4co_amd import TrainableNARGNNDepotEncoder as E

    def td(env="cvrp", n=12, b=2, **kw):
        locs, feats = torch.rand(b, n, 2, **kw), torch.rand(b, n - 1, R.FEATURES.get(env, 2), **kw)
        return R.td_of(env if env in R.FEATURES else "pctsp", locs, feats)

    with pytest.raises(NotImplementedError, match="td\\['locs'\\] on cpu"):
        E(num_layers_graph_encoder=1)(td())
    with pytest.raises(NotImplementedError, match="td\\['locs'\\] on cpu"):  # eval: the parent's refusal
        E(num_layers_graph_encoder=1).eval()(td())
    with pytest.raises(NotImplementedError, match="cvrp / op / pctsp environment only, got 'spctsp'"):
        E(env_name="spctsp", num_layers_graph_encoder=1)(td("spctsp"))
    for kw, why in ((dict(env_name="tsp"), "environment only"), (dict(act_fn="relu"), "act_fn='silu'"),
                    (dict(agg_fn="max"), "agg_fn='mean'"), (dict(embed_dim=32), "embed_dim=64"),
                    (dict(graph_network=torch.nn.Identity()), "custom graph_network"),
                    (dict(heatmap_generator=torch.nn.Identity()), "custom heatmap_generator")):
        with pytest.raises(NotImplementedError, match=why):
            E(num_layers_graph_encoder=1, **kw)(td())

    # the checks that come behind the device: through _check on a stand-in that claims to be on the card
    class OnCard:
        is_cuda, device = True, "cuda:0"

        def __init__(self, shape, dtype=torch.float32):
            self.shape, self.dtype = shape, dtype

        def dim(self):
            return len(self.shape)

    enc = E(num_layers_graph_encoder=1)
    with pytest.raises(NotImplementedError, match="N >= 3 nodes"):
        enc._check(OnCard((4, 2, 2)))
    with pytest.raises(NotImplementedError, match="fp32 only"):
        enc._check(OnCard((2, 12, 2), torch.float64))
    with pytest.raises(NotImplementedError, match="fp32 only"):  # the features count too
        enc._check(OnCard((2, 12, 2)), OnCard((2, 11, 1), torch.float64))
    with pytest.raises(NotImplementedError, match="fp32 only"):
        E(num_layers_graph_encoder=1).double()._check(OnCard((2, 12, 2)))
    enc._check(OnCard((2, 3, 2)), OnCard((2, 2, 1)))


def test_kernel_binding_refusals():
    from rl4co_amd import _lib
    from rl4co_amd import kernels as K

    b, n, k = 2, 12, 10
    c, e = n - 1, (n - 1) * (k + 2)
    nbr = torch.ones(b, c, k, dtype=torch.int32)
    ptr, src = torch.zeros(b * n + 1, dtype=torch.int32), torch.zeros(b * e, dtype=torch.int32)
    p = dict(lin_w=torch.rand(1, 5, 64, 64), lin_b=torch.rand(1, 5, 64), bn_w=torch.rand(1, 2, 64), bn_b=torch.rand(1, 2, 64))
    x, w = torch.rand(b, n, 64), torch.rand(b, e, 64)
    with pytest.raises(NotImplementedError, match="embed_dim = 64"):
        K.nargnn_depot_train_forward(nbr, ptr, src, torch.rand(b, n, 32), w, **p)
    with pytest.raises(NotImplementedError, match="K <= min\\(N - 2, 64\\)"):
        K.nargnn_depot_train_forward(torch.ones(b, c, 11, dtype=torch.int32), ptr, src, x, w, **p)
    with pytest.raises(ValueError, match="w_in"):
        K.nargnn_depot_train_forward(nbr, ptr, src, x, torch.rand(b, c, k, 64), **p)
    with pytest.raises(ValueError, match="csr_src"):
        K.nargnn_depot_train_forward(nbr, ptr, src[:-1], x, w, **p)
    with pytest.raises(_lib.Rl4coLibraryError, match="no CPU fallback"):
        K.nargnn_depot_train_forward(nbr, ptr, src, x, w, **p)


# ---- 5. the restatement against the records ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(T.CASES))
def test_restatement_matches_the_recorded_reference(case):
    """Both sides are float64 of the same math: every recorded tensor lies within the record's floor, ``bound / 4``."""
    rec = T.record(case)
    env, n, k_sparse, layers, mlp_layers, _, _ = T.CASES[case]
    sd = T.case_state_dict(case)
    assert R.state_hash(sd) == bytes(rec["weights_sha256"].tolist()).hex() and R.count_layers(sd) == (layers, mlp_layers)
    nbr = R.edge_index_to_neighbors(rec["edge_index"], T.BATCH, n)
    assert nbr.shape[2] == R.num_neighbors(n, k_sparse) and rec["feats"].shape[2] == R.FEATURES[env]
    on = R.on_graph(nbr, n)
    got = T.run(sd, rec["locs"], rec["feats"], nbr, torch.float64)
    pairs = T.record_pairs(rec)
    assert sorted(pairs) == sorted(got) and "grad/init_embedding.init_embed_depot.weight" in pairs
    worst = 0.0
    for name, (ref32, ref64) in pairs.items():
        a = got[name]
        if name.endswith("num_batches_tracked"):
            assert int(a) == int(ref64) == int(ref32) == 8  # 7 in the state dict, + 1
            continue
        if name == "heatmap":
            a, ref32, ref64 = a[on], ref32[on], ref64[on]
        floor = T.bound(ref32, ref64) / 4
        err = float((a - ref64).abs().max())
        worst = max(worst, err / floor if floor else 0.0)
        assert err <= floor, f"{name}: the float64 restatement is {err:.3e} from the float64 record, the floor is {floor:.3e}"
    print(f"{case}: the float64 restatement is at most {worst:.2e} x the floor from the float64 record")


# ---- 6. the recorder itself (needs the reference checkout) ---------------------------------------------------------------------
def test_recorder_reproduces_a_record():
    from oracle import ref_import

    if not ref_import.available():
        pytest.skip("the reference checkout is not here")
    rec, again = T.record("cvrp_n12"), T.reference_run("cvrp_n12")
    assert sorted(rec) == sorted(again)
    for key in ("locs", "feats", "edge_index", "heatmap32", "heatmap64", "grad/graph_network.layers.0.e_lin.weight/64"):
        assert torch.equal(rec[key], torch.as_tensor(again[key])), key
