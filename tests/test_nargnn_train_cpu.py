"""The trainable heatmap encoder without a GPU: the dense train-mode restatement (tests/nargnn_train_ref.py) against the
records of the reference's own NARGNNEncoder in ``.train()``, the incoming-edge CSR against a brute-force loop, the running
statistics' update, the module's ``state_dict`` keys and refusals, and the C boundary of ``rl4co_nargnn_train_*``."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from tests import nargnn_ref as R
from tests import nargnn_train_ref as T

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "rl4co_amd.h").read_text()


# ---- 1. the restatement against the records -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(T.CASES))
def test_restatement_matches_the_recorded_reference(case):
    rec = T.record(case)
    n, k_sparse, layers, mlp_layers, _, _ = T.CASES[case]
    sd = T.case_state_dict(case)
    assert R.state_hash(sd) == bytes(rec["weights_sha256"].tolist()).hex() and R.count_layers(sd) == (layers, mlp_layers)
    nbr = R.edge_index_to_neighbors(rec["edge_index"], T.BATCH, n)
    assert nbr.shape[2] == R.num_neighbors(n, k_sparse)
    on = T.graph_mask(nbr, n)
    got64, got32 = T.run(sd, rec["locs"], nbr, torch.float64), T.run(sd, rec["locs"], nbr, torch.float32)
    pairs = T.record_pairs(rec)
    assert sorted(pairs) == sorted(got64)
    worst = 0.0
    for name, (ref32, ref64) in pairs.items():
        a64, a32 = got64[name], got32[name]
        if name.endswith("num_batches_tracked"):
            assert int(a64) == int(ref64) == 8 and int(a32) == 8  # 7 in the state dict, + 1
            continue
        if name == "heatmap":
            a64, a32, ref32, ref64 = a64[on], a32[on], ref32[on], ref64[on]
        scale = float(ref64.abs().max())
        if scale == 0.0:  # the last layer's node update reaches no output
            assert float(a64.abs().max()) == 0.0 and float(a32.abs().max()) == 0.0, name
            continue
        # float64: 1e-12 of the tensor's scale, or of the scale of the terms of a sum that cancels to nothing (the bias of
        # a linear directly ahead of a batch norm has a zero gradient in exact arithmetic)
        assert float((a64 - ref64).abs().max()) <= 1e-12 * max(scale, 1.0), name
        floor = float((ref32.double() - ref64).abs().max())
        err = float((a32.double() - ref64).abs().max())
        worst = max(worst, err / floor if floor else 0.0)
        assert err <= 4 * max(floor, 2.0 ** -23 * scale), f"{name}: {err:.3e} against a floor of {floor:.3e}"
    print(f"{case}: the fp32 restatement is at most {worst:.2f} x the fp32 reference's own distance from float64")


# ---- 2. the CSR, the running statistics, the module tree ----------------------------------------------------------------------
def test_incoming_csr_equals_the_brute_force_loop():
    from rl4co_amd import kernels as K

    gen = torch.Generator().manual_seed(2)
    nbr = torch.stack([torch.stack([torch.randperm(6, generator=gen)[:3] + 1 for _ in range(7)]) for _ in range(3)])
    nbr[:, :, 0] = 2  # node 2 of every instance is in every list (its own included), node 0 in none
    ptr, src = K.incoming_csr(nbr.to(torch.int32))
    want_ptr, want_src = T.incoming_csr_bruteforce(nbr)
    assert torch.equal(ptr, want_ptr) and torch.equal(src, want_src) and ptr.dtype == src.dtype == torch.int32
    degree = (ptr[1:] - ptr[:-1]).view(3, 7)
    assert bool((degree[:, 0] == 0).all()) and bool((degree[:, 2] >= 7).all()) and int(ptr[-1]) == nbr.numel()
    for j in range(21):  # ascending edge rows inside a node's run
        run = src[int(ptr[j]):int(ptr[j + 1])]
        assert bool((run[1:] > run[:-1]).all())


def test_running_statistics_update():
    from rl4co_amd import TrainableNARGNNEncoder

    enc = TrainableNARGNNEncoder(num_layers_graph_encoder=2, num_layers_heatmap_generator=2)
    enc.load_state_dict(R.make_state_dict(5, 2, 2), strict=True)
    bns = [bn.module for layer in enc.graph_network.layers for bn in (layer.v_bn, layer.e_bn)]
    before = [(bn.running_mean.clone(), bn.running_var.clone()) for bn in bns]
    stats = torch.rand(2, 6, 64, generator=torch.Generator().manual_seed(1))
    node_rows, k = 12, 5
    enc._update_running_statistics(bns, stats, node_rows, k, 0.1)
    for i, bn in enumerate(bns):
        layer, side = divmod(i, 2)
        n = node_rows * (k if side else 1)
        mean, var = stats[layer, 3 * side], stats[layer, 3 * side + 2]
        assert torch.allclose(bn.running_mean, 0.9 * before[i][0] + 0.1 * mean, rtol=1e-6, atol=1e-7)
        assert torch.allclose(bn.running_var, 0.9 * before[i][1] + 0.1 * var * n / (n - 1), rtol=1e-6, atol=1e-7)
        assert int(bn.num_batches_tracked) == 8
    # the restatement's update is BatchNorm1d's own
    bn = torch.nn.BatchNorm1d(64).train()
    sd = R.make_state_dict(6, 1, 2)
    t = torch.randn(40, 64)
    bn.load_state_dict({k.rsplit(".", 1)[1]: v for k, v in sd.items() if ".layers.0.v_bn." in k})
    bn(t)
    mean, var = t.mean(0), t.var(0, unbiased=True)
    assert torch.allclose(bn.running_mean, 0.9 * sd["graph_network.layers.0.v_bn.module.running_mean"] + 0.1 * mean, atol=1e-6)
    assert torch.allclose(bn.running_var, 0.9 * sd["graph_network.layers.0.v_bn.module.running_var"] + 0.1 * var, atol=1e-6)


def test_state_dict_keys_and_strict_loads_both_ways():
    import rl4co_amd
    from rl4co_amd import NARGNNEncoder, TrainableNARGNNEncoder, nargnn

    assert "TrainableNARGNNEncoder" in rl4co_amd.__all__ and rl4co_amd.TrainableNARGNNEncoder is nargnn.TrainableNARGNNEncoder
    assert issubclass(TrainableNARGNNEncoder, NARGNNEncoder)
    enc, parent = TrainableNARGNNEncoder(), NARGNNEncoder()
    assert list(enc.state_dict().keys()) == list(parent.state_dict().keys()) == R.recorded_keys()
    assert any(key.endswith("num_batches_tracked") for key in enc.state_dict())
    enc.load_state_dict(T.case_state_dict("n20_full"), strict=True)
    parent.load_state_dict(enc.state_dict(), strict=True)
    enc.load_state_dict(parent.state_dict(), strict=True)
    nobias = TrainableNARGNNEncoder(num_layers_graph_encoder=1, num_layers_heatmap_generator=3, linear_bias=False)
    assert sorted(nobias.state_dict()) == sorted(R.make_state_dict(1, 1, 3, linear_bias=False))


def _td(n=12, b=2, **kw):
    return {"locs": torch.rand(b, n, 2, **kw)}


def test_refusals():
    from rl4co_amd import TrainableNARGNNEncoder as E

    with pytest.raises(NotImplementedError, match="td\\['locs'\\] on cpu"):
        E(num_layers_graph_encoder=1)(_td())
    with pytest.raises(NotImplementedError, match="td\\['locs'\\] on cpu"):  # eval: the parent's refusal
        E(num_layers_graph_encoder=1).eval()(_td())
    for kw, why in ((dict(env_name="cvrp"), "tsp environment only"), (dict(act_fn="relu"), "act_fn='silu'"),
                    (dict(agg_fn="max"), "agg_fn='mean'"), (dict(embed_dim=32), "embed_dim=64"),
                    (dict(graph_network=torch.nn.Identity()), "custom graph_network"),
                    (dict(heatmap_generator=torch.nn.Identity()), "custom heatmap_generator"),
                    (dict(init_embedding=torch.nn.Identity()), "custom init_embedding"),
                    (dict(edge_embedding=torch.nn.Identity()), "custom edge_embedding")):
        with pytest.raises(NotImplementedError, match=why):
            E(num_layers_graph_encoder=1, **kw)(_td())
    # the checks that come behind the device: through _check on a stand-in that claims to be on the card
    class OnCard:
        is_cuda, device = True, "cuda:0"

        def __init__(self, shape, dtype=torch.float32):
            self.shape, self.dtype = shape, dtype

        def dim(self):
            return len(self.shape)

    enc = E(num_layers_graph_encoder=1)
    with pytest.raises(NotImplementedError, match="B N >= 2"):
        enc._check(OnCard((1, 1, 2)))
    with pytest.raises(NotImplementedError, match="fp32 only"):
        enc._check(OnCard((2, 12, 2), torch.float64))
    with pytest.raises(NotImplementedError, match="fp32 only"):
        E(num_layers_graph_encoder=1).double()._check(OnCard((2, 12, 2)))
    enc._check(OnCard((2, 12, 2)))


def test_kernel_binding_refusals():
    from rl4co_amd import _lib
    from rl4co_amd import kernels as K

    b, n, k = 2, 12, 10
    nbr = torch.zeros(b, n, k, dtype=torch.int32)
    ptr, src = torch.zeros(b * n + 1, dtype=torch.int32), torch.zeros(b * n * k, dtype=torch.int32)
    p = dict(lin_w=torch.rand(1, 5, 64, 64), lin_b=torch.rand(1, 5, 64), bn_w=torch.rand(1, 2, 64), bn_b=torch.rand(1, 2, 64))
    x, w = torch.rand(b, n, 64), torch.rand(b, n, k, 64)
    with pytest.raises(NotImplementedError, match="embed_dim = 64"):
        K.nargnn_train_forward(nbr, ptr, src, torch.rand(b, n, 32), w, **p)
    with pytest.raises(NotImplementedError, match="K <= min"):
        K.nargnn_train_forward(torch.zeros(b, n, 12, dtype=torch.int32), ptr, src, x, w, **p)
    with pytest.raises(ValueError, match="lin_b"):
        K.nargnn_train_forward(nbr, ptr, src, x, w, **{**p, "lin_b": torch.rand(1, 4, 64)})
    with pytest.raises(ValueError, match="csr_ptr"):
        K.nargnn_train_forward(nbr, ptr[:-1], src, x, w, **p)
    with pytest.raises(_lib.Rl4coLibraryError, match="no CPU fallback"):
        K.nargnn_train_forward(nbr, ptr, src, x, w, **p)


# ---- 3. the C boundary --------------------------------------------------------------------------------------------------------
def test_header_ctypes_and_symbols_agree():
    from rl4co_amd import _lib

    assert int(re.search(r"#define RL4CO_ABI_VERSION (\d+)", HEADER).group(1)) >= 26 and _lib.ABI_VERSION >= 26
    body = re.search(r"typedef struct rl4co_nargnn_train_args \{(.*?)\} rl4co_nargnn_train_args;", HEADER, re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.NargnnTrainArgs._fields_]
    assert ctypes.sizeof(_lib.NargnnTrainArgs) == 8 * 4 + 23 * 8
    handle = _lib.lib()
    assert handle.rl4co_abi_version() == _lib.ABI_VERSION
    for name in ("rl4co_nargnn_train_forward", "rl4co_nargnn_train_backward", "rl4co_nargnn_train_workspace_bytes"):
        assert name in _lib.SYMBOLS and getattr(handle, name) is not None
    args = _lib.NargnnTrainArgs()
    for fn in (handle.rl4co_nargnn_train_forward, handle.rl4co_nargnn_train_backward):
        assert fn(ctypes.byref(args), None) == 1 and b"a.D == kD" in handle.rl4co_last_error()
    args.D, args.B, args.N, args.K, args.L = 64, 1, 12, 65, 1
    assert handle.rl4co_nargnn_train_forward(ctypes.byref(args), None) == 1 and b"a.K <= 64" in handle.rl4co_last_error()


def test_workspace_formula():
    from rl4co_amd import kernels as K

    def want(b, n, k, layers):
        nv, ne = 64 * b * n, 64 * b * n * k
        pv, pe = min(-(-b * n // 64), 1024), min(-(-b * n * k // 64), 1024)
        floats = (64 + max(layers - 1, 0) * (nv + ne) + layers * (2 * nv + ne) + 5 * nv + 2 * ne + 192 * (pv + pe)
                  + 4160 * (4 * pv + pe) + 512)
        return 4 * floats

    for shape in ((1, 2, 1, 1), (3, 20, 10, 15), (128, 100, 20, 15), (512, 50, 10, 15), (1, 1024, 10, 1), (2, 200, 40, 3)):
        assert K.nargnn_train_workspace_bytes(*shape) == want(*shape), shape
    # the edge-sized saves dominate: (2 L - 1) planes of B N K 256 bytes, plus two edge-sized temporaries
    big = K.nargnn_train_workspace_bytes(128, 100, 20, 15)
    assert 31 * 128 * 100 * 20 * 256 < big < 1.1 * 31 * 128 * 100 * 20 * 256
    for shape in ((0, 12, 10, 1), (1, 1, 1, 1), (1, 1025, 10, 1), (1, 12, 12, 1), (1, 100, 65, 1), (1, 12, 10, 0), (4096, 1024, 64, 1)):
        assert K.nargnn_train_workspace_bytes(*shape) == 0, shape


# ---- 4. the recorder itself (needs the reference checkout) ---------------------------------------------------------------------
def test_recorder_reproduces_a_record():
    from oracle import ref_import

    if not ref_import.available():
        pytest.skip("the reference checkout is not here")
    rec, again = T.record("n11"), T.reference_run("n11")
    assert sorted(rec) == sorted(again)
    for key in ("locs", "edge_index", "heatmap32", "heatmap64", "grad/graph_network.layers.0.e_lin.weight/64"):
        assert torch.equal(rec[key], torch.as_tensor(again[key])), key
