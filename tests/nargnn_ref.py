"""DeepACO's heatmap encoder (NARGNNEncoder for TSP, inference): a plain-torch restatement in the dense [B, N, K, D] form the
kernel uses (any dtype: fp32 for the bench baseline, fp64 as the yardstick), a seeded generator of ``state_dict``s under the
reference's key names, and the recorder of the reference's own classes (tests/golden/reference/nargnn_<case>.npz).

The recorder runs the reference's ``NARGNNEncoder`` itself through oracle/ref_import.py with a stand-in ``torch_geometric``
defined here (``Data``, ``Batch.from_data_list`` / ``to_data_list``, ``nn.global_mean_pool``, ``nn.BatchNorm``: containers
and one segment mean, no reference text) and two extra empty package shells. The weights of every case come from
``make_state_dict(seed)`` and are loaded into the reference module with ``strict=True`` (which pins the key names from the
reference's side); the record keeps the seed and a hash, and for the smallest case the state dict itself. Every batch norm
gets random running statistics and affine terms: a fresh one is nearly the identity and would hide a wrong fold."""
import hashlib
import json
import sys
import types

import numpy as np
import torch

D = 64
SMALL = 1e-12
BATCH = 3
# case -> (N, k_sparse, GNN layers, heatmap MLP layers, weight seed, data seed)
CASES = {"n11": (11, None, 1, 2, 101, 201), "n20_full": (20, None, 15, 5, 102, 202), "n50": (50, None, 3, 3, 103, 203),
         "n60_k17": (60, 17, 2, 2, 104, 204)}
STORES_STATE_DICT = ("n11",)
LIN_NAMES = ("v_lin1", "v_lin2", "v_lin3", "v_lin4", "e_lin")


def num_neighbors(n, k_sparse=None):
    return min(max(n // 5, 10) if k_sparse is None else k_sparse, n - 1)


# ---- weights --------------------------------------------------------------------------------------------------------------
def make_state_dict(seed, layers, mlp_layers, linear_bias=True, d=D):
    """A float32 ``state_dict`` under the reference's keys: linears U(-1 / sqrt(in), 1 / sqrt(in)), batch norms with random
    running statistics and affine terms."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def linear(name, fan_out, fan_in, bias=True):
        bound = fan_in ** -0.5
        sd[f"{name}.weight"] = (torch.rand(fan_out, fan_in, generator=g) * 2 - 1) * bound
        if bias:
            sd[f"{name}.bias"] = (torch.rand(fan_out, generator=g) * 2 - 1) * bound

    linear("init_embedding.init_embed", d, 2)
    linear("edge_embedding.edge_embed", d, 1)
    for i in range(layers):
        p = f"graph_network.layers.{i}"
        for name in LIN_NAMES:
            linear(f"{p}.{name}", d, d)
        for bn in ("v_bn", "e_bn"):
            sd[f"{p}.{bn}.module.weight"] = torch.rand(d, generator=g) + 0.5
            sd[f"{p}.{bn}.module.bias"] = torch.randn(d, generator=g) * 0.3
            sd[f"{p}.{bn}.module.running_mean"] = torch.randn(d, generator=g) * 0.5
            sd[f"{p}.{bn}.module.running_var"] = torch.rand(d, generator=g) + 0.5
            sd[f"{p}.{bn}.module.num_batches_tracked"] = torch.tensor(7, dtype=torch.int64)
    for i in range(mlp_layers - 1):
        linear(f"heatmap_generator.linears.{i}", d, d, linear_bias)
    linear("heatmap_generator.output", 1, d, linear_bias)
    return sd


def state_hash(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def case_state_dict(case):
    _, _, layers, mlp_layers, wseed, _ = CASES[case]
    return make_state_dict(wseed, layers, mlp_layers)


def count_layers(sd):
    layers = len({k.split(".")[2] for k in sd if k.startswith("graph_network.layers.")})
    hidden = len({k.split(".")[2] for k in sd if k.startswith("heatmap_generator.linears.")})
    return layers, hidden + 1


# ---- the restatement --------------------------------------------------------------------------------------------------------
def select_neighbors(locs, k):
    """edge.py:88-104, ops.py:93-100, 169-199 for a batch: (neighbors [B, N, K] int64, cost [B, N, K])."""
    cost = (locs[..., :, None, :] - locs[..., None, :, :]).norm(p=2, dim=-1)
    cost.diagonal(dim1=1, dim2=2).fill_(torch.inf)
    values, indices = torch.topk(cost, k=k, dim=-1, largest=False, sorted=False)
    return indices, values


def gather_nodes(x, nbr):
    """x [B, N, D], nbr [B, N, K] -> x[b, nbr[b, u, k]] [B, N, K, D]"""
    b, n, k = nbr.shape
    return x.gather(1, nbr.reshape(b, n * k, 1).expand(-1, -1, x.shape[-1])).view(b, n, k, -1)


def encode(sd, locs, k_sparse=None, dtype=torch.float32, neighbors=None, eps=1e-5, return_edges=False):
    """(heatmap_logits [B, N, N], node_embed [B, N, D]) of the encoder in ``dtype``. ``neighbors`` [B, N, K] fixes the graph
    (then the costs are the distances to those neighbours); otherwise it is selected from ``locs`` in ``dtype``."""
    sd = {k: (v.to(device=locs.device, dtype=dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    locs = locs.to(dtype)
    layers, mlp_layers = count_layers(sd)
    silu, sigmoid = torch.nn.functional.silu, torch.sigmoid

    def lin(name, t):
        y = t @ sd[f"{name}.weight"].t()
        return y + sd[f"{name}.bias"] if f"{name}.bias" in sd else y

    def bn(name, t):
        scale = sd[f"{name}.module.weight"] / torch.sqrt(sd[f"{name}.module.running_var"] + eps)
        return (t - sd[f"{name}.module.running_mean"]) * scale + sd[f"{name}.module.bias"]

    if neighbors is None:
        nbr, cost = select_neighbors(locs, num_neighbors(locs.shape[1], k_sparse))
    else:
        nbr = neighbors.to(torch.int64)
        cost = (locs[:, :, None, :] - gather_nodes(locs, nbr)).norm(p=2, dim=-1)
    node_embed = lin("init_embedding.init_embed", locs)
    x = silu(node_embed)
    w = silu(lin("edge_embedding.edge_embed", cost[..., None]))
    for i in range(layers):
        p = f"graph_network.layers.{i}"
        x1, x2, x3, x4 = (lin(f"{p}.v_lin{j}", x) for j in (1, 2, 3, 4))
        agg = (sigmoid(w) * gather_nodes(x2, nbr)).mean(2)
        x_new = x + silu(bn(f"{p}.v_bn", x1 + agg))
        w = w + silu(bn(f"{p}.e_bn", lin(f"{p}.e_lin", w) + x3[:, :, None, :] + gather_nodes(x4, nbr)))
        x = x_new
    h = w
    for i in range(mlp_layers - 1):
        h = silu(lin(f"heatmap_generator.linears.{i}", h))
    prob = sigmoid(lin("heatmap_generator.output", h))[..., 0]  # [B, N, K]
    heat = torch.zeros(locs.shape[0], locs.shape[1], locs.shape[1], dtype=dtype, device=locs.device).scatter_(2, nbr, prob)
    logits = torch.log(heat + SMALL)
    return (logits, node_embed, nbr, prob) if return_edges else (logits, node_embed)


def edge_index_to_neighbors(edge_index, b, n):
    """The reference's batched edge_index [2, B N K] (sources ascending, K per node) -> neighbors [B, N, K] int64."""
    k = edge_index.shape[1] // (b * n)
    src = edge_index[0].view(b, n, k)
    want = (torch.arange(b)[:, None, None] * n + torch.arange(n)[None, :, None]).expand(b, n, k)
    assert torch.equal(src, want), "the reference's edges are not K per node in node order"
    return edge_index[1].view(b, n, k) - torch.arange(b)[:, None, None] * n


def kernel_parameters(sd, device="cuda"):
    """The state dict as kernels.nargnn_heatmap takes it (batch norms folded in float64, rounded once)."""
    layers, mlp_layers = count_layers(sd)

    def f(t):
        return t.to(device=device, dtype=torch.float32).contiguous()

    def fold(name, eps=1e-5):
        scale = sd[f"{name}.module.weight"].double() / torch.sqrt(sd[f"{name}.module.running_var"].double() + eps)
        return torch.stack((scale, sd[f"{name}.module.bias"].double() - sd[f"{name}.module.running_mean"].double() * scale), 0)

    p = dict(init_w=f(sd["init_embedding.init_embed.weight"]), init_b=f(sd["init_embedding.init_embed.bias"]),
             edge_w=f(sd["edge_embedding.edge_embed.weight"]), edge_b=f(sd["edge_embedding.edge_embed.bias"]),
             lin_w=None, lin_b=None, bn=None, mlp_w=None, mlp_b=None, out_w=f(sd["heatmap_generator.output.weight"]),
             out_b=f(sd["heatmap_generator.output.bias"]) if "heatmap_generator.output.bias" in sd else None)
    if layers:
        pre = [f"graph_network.layers.{i}" for i in range(layers)]
        p["lin_w"] = f(torch.stack([torch.stack([sd[f"{q}.{n}.weight"] for n in LIN_NAMES], 0) for q in pre], 0))
        p["lin_b"] = f(torch.stack([torch.stack([sd[f"{q}.{n}.bias"] for n in LIN_NAMES], 0) for q in pre], 0))
        p["bn"] = f(torch.stack([torch.stack((fold(f"{q}.v_bn"), fold(f"{q}.e_bn")), 0) for q in pre], 0))
    if mlp_layers > 1:
        p["mlp_w"] = f(torch.stack([sd[f"heatmap_generator.linears.{i}.weight"] for i in range(mlp_layers - 1)], 0))
        if "heatmap_generator.linears.0.bias" in sd:
            p["mlp_b"] = f(torch.stack([sd[f"heatmap_generator.linears.{i}.bias"] for i in range(mlp_layers - 1)], 0))
    return p


# ---- the stand-in torch_geometric (containers and one segment mean) ----------------------------------------------------------
def _install_torch_geometric():
    if "torch_geometric" in sys.modules:
        return

    class Data:
        def __init__(self, x=None, edge_index=None, edge_attr=None):
            self.x, self.edge_index, self.edge_attr = x, edge_index, edge_attr

    class Batch(Data):
        @classmethod
        def from_data_list(cls, graphs):
            nodes = [g.x.shape[0] for g in graphs]
            offsets = [sum(nodes[:i]) for i in range(len(graphs))]
            out = cls(torch.cat([g.x for g in graphs], 0), torch.cat([g.edge_index + o for g, o in zip(graphs, offsets)], 1),
                      torch.cat([g.edge_attr for g in graphs], 0))
            out._nodes, out._edges, out._offsets = nodes, [g.edge_index.shape[1] for g in graphs], offsets
            return out

        def to_data_list(self):
            xs, idx, attr = self.x.split(self._nodes, 0), self.edge_index.split(self._edges, 1), self.edge_attr.split(self._edges, 0)
            return [Data(x, i - o, a) for x, i, a, o in zip(xs, idx, attr, self._offsets)]

    def global_mean_pool(x, batch, size=None):
        size = int(batch.max()) + 1 if size is None else size
        total = torch.zeros(size, x.shape[1], dtype=x.dtype).index_add_(0, batch, x)
        return total / torch.bincount(batch, minlength=size).clamp(min=1).to(x.dtype)[:, None]

    class BatchNorm(torch.nn.Module):
        def __init__(self, in_channels, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
            super().__init__()
            self.module = torch.nn.BatchNorm1d(in_channels, eps, momentum, affine, track_running_stats)

        def forward(self, x):
            return self.module(x)

    root, data, nn_ = (types.ModuleType(n) for n in ("torch_geometric", "torch_geometric.data", "torch_geometric.nn"))
    data.Data, data.Batch = Data, Batch
    nn_.global_mean_pool, nn_.BatchNorm = global_mean_pool, BatchNorm
    root.data, root.nn = data, nn_
    sys.modules.update({"torch_geometric": root, "torch_geometric.data": data, "torch_geometric.nn": nn_})


def reference_encoder_class():
    """The reference's NARGNNEncoder, its file executed verbatim; two more empty package shells keep the package
    ``__init__`` files (and what they import) out."""
    import importlib

    from oracle import ref_import

    ref_import.install()
    _install_torch_geometric()
    for pkg, lazy in (("rl4co.models.nn.env_embeddings", {"env_edge_embedding": "rl4co.models.nn.env_embeddings.edge",
                                                           "env_init_embedding": "rl4co.models.nn.env_embeddings.init"}),
                      ("rl4co.models.zoo.nargnn", {})):
        if pkg not in sys.modules:
            mod = ref_import._Shell(pkg)
            mod.__path__ = [str(ref_import.REFERENCE_ROOT / pkg.replace(".", "/"))]
            mod.__package__ = pkg
            sys.modules[pkg] = mod
            setattr(sys.modules[pkg.rpartition(".")[0]], pkg.rpartition(".")[2], mod)
            ref_import._LAZY[pkg] = lazy
    # a module that was imported before the stand-in existed holds None in its optional torch_geometric names
    edge = importlib.import_module("rl4co.models.nn.env_embeddings.edge")
    edge.Data, edge.Batch = sys.modules["torch_geometric.data"].Data, sys.modules["torch_geometric.data"].Batch
    importlib.import_module("rl4co.models.nn.graph.gnn").gnn = sys.modules["torch_geometric.nn"]
    return importlib.import_module("rl4co.models.zoo.nargnn.encoder").NARGNNEncoder


def reference_run(case):
    n, k_sparse, layers, mlp_layers, wseed, dseed = CASES[case]
    cls = reference_encoder_class()
    sd = make_state_dict(wseed, layers, mlp_layers)
    locs = torch.rand(BATCH, n, 2, generator=torch.Generator().manual_seed(dseed))
    seen = {}

    def build(dtype):
        enc = cls(embed_dim=D, env_name="tsp", num_layers_heatmap_generator=mlp_layers, num_layers_graph_encoder=layers,
                  k_sparse=k_sparse).eval()
        enc.load_state_dict(sd, strict=True)
        enc = enc.to(dtype)
        inner = enc.edge_embedding._cost_matrix_to_graph

        def keep(cost, emb):
            graph = inner(cost, emb)
            seen[dtype] = graph.edge_index.clone()
            return graph

        enc.edge_embedding._cost_matrix_to_graph = keep
        return enc

    with torch.no_grad():
        enc32 = build(torch.float32)
        heat32, embed32 = enc32({"locs": locs.clone()})
        # float64: the reference's heatmap generator refuses the dtype at its last step (log(heatmap + small_value)), so the
        # module runs up to the edge probabilities and that one step is taken here
        enc64 = build(torch.float64)
        enc64.heatmap_generator._make_heatmap_logits = lambda graph: graph
        graph, _ = enc64({"locs": locs.double()})
        nbr64 = edge_index_to_neighbors(seen[torch.float64], BATCH, n)
        heat64 = torch.log(torch.zeros(BATCH, n, n, dtype=torch.float64).scatter_(2, nbr64, graph.edge_attr.view(BATCH, n, -1))
                           + SMALL)
    nbr32 = edge_index_to_neighbors(seen[torch.float32], BATCH, n)
    assert torch.equal(nbr32.sort(-1).values, nbr64.sort(-1).values), "fp32 and fp64 select different neighbours: another seed"
    rec = {"locs": locs, "edge_index": seen[torch.float32], "heatmap32": heat32, "heatmap64": heat64, "node_embed32": embed32,
           "weight_seed": torch.tensor(wseed), "weights_sha256": np.frombuffer(bytes.fromhex(state_hash(sd)), dtype=np.uint8)}
    if case in STORES_STATE_DICT:
        rec.update({f"sd/{k}": v for k, v in sd.items()})
    if case == "n20_full":  # the reference's own key names, from its own module
        from tests.helpers import REFERENCE_RECORDS

        (REFERENCE_RECORDS / "nargnn_state_dict_keys.json").write_text(json.dumps(list(enc32.state_dict().keys()), indent=0) + "\n")
    return rec


def record(case):
    from tests.helpers import reference_record

    return reference_record(f"nargnn_{case}", lambda: reference_run(case))


def recorded_keys():
    from tests.helpers import REFERENCE_RECORDS

    return json.loads((REFERENCE_RECORDS / "nargnn_state_dict_keys.json").read_text())


def floor32(rec):
    """The fp32 reference's own distance from its fp64 run at the graph's entries: the unit of every tolerance here."""
    b, n, _ = rec["heatmap32"].shape
    nbr = edge_index_to_neighbors(rec["edge_index"], b, n)
    return float((rec["heatmap32"].double().gather(2, nbr) - rec["heatmap64"].gather(2, nbr)).abs().max())


if __name__ == "__main__":  # RL4CO_RECORD_REFERENCE=1 python -m tests.nargnn_ref
    for name in CASES:
        r = record(name)
        print(name, "floor", floor32(r), {k: tuple(v.shape) for k, v in r.items() if not k.startswith("sd/")})
