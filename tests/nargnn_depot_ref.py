"""DeepACO's heatmap encoder for the depot graphs (NARGNNEncoder(env_name="cvrp" | "op" | "pctsp"), inference): a plain-torch
restatement in edge-list form (any dtype: fp32 for the bench baseline, fp64 as the yardstick) that builds
``CVRPEdgeEmbedding``'s graph, pools by source with a segment mean and scatters to [B, N, N]; a seeded generator of
``state_dict``s under the reference's key names; and the recorder of the reference's own classes
(tests/golden/reference/nargnn_depot_<case>.npz).

The recorder runs the reference's ``NARGNNEncoder`` itself through oracle/ref_import.py with tests/nargnn_ref.py's stand-in
``torch_geometric`` and package shells. The weights of every case come from ``make_state_dict`` and are loaded into the
reference module with ``strict=True``; the record keeps the seed and a hash, and for the smallest case the state dict
itself. Every batch norm gets random running statistics and affine terms, as in tests/nargnn_ref.py."""
import json

import numpy as np
import torch

from tests import nargnn_ref as T

D = T.D
SMALL = T.SMALL
BATCH = 3
FEATURES = {"cvrp": 1, "op": 1, "pctsp": 2}  # environment -> F
# case -> (env, N with the depot, k_sparse, GNN layers, heatmap MLP layers, weight seed, data seed)
CASES = {"cvrp_n12": ("cvrp", 12, None, 1, 2, 111, 211), "cvrp_n21_full": ("cvrp", 21, None, 15, 5, 112, 212),
         "op_n51": ("op", 51, None, 3, 3, 113, 213), "pctsp_n40_k17": ("pctsp", 40, 17, 2, 2, 114, 214)}
STORES_STATE_DICT = ("cvrp_n12",)
state_hash, count_layers = T.state_hash, T.count_layers


def num_neighbors(n, k_sparse=None):
    """edge.py:132 (k from N with the depot), ops.py:183 (clamped to the customer block's C - 1)."""
    return min(max(n // 5, 10) if k_sparse is None else k_sparse, n - 2)


# ---- weights --------------------------------------------------------------------------------------------------------------
def make_state_dict(env, seed, layers, mlp_layers, linear_bias=True, d=D):
    """tests/nargnn_ref.py's seeded state dict with the depot graphs' init embedding: ``init_embed`` over (x, y, features),
    ``init_embed_depot`` over (x, y), in the reference's key order."""
    g = torch.Generator().manual_seed(seed + 7)
    body = T.make_state_dict(seed, layers, mlp_layers, linear_bias, d)
    sd = {}
    for name, fan_in in (("init_embedding.init_embed", 2 + FEATURES[env]), ("init_embedding.init_embed_depot", 2)):
        bound = fan_in ** -0.5
        sd[f"{name}.weight"] = (torch.rand(d, fan_in, generator=g) * 2 - 1) * bound
        sd[f"{name}.bias"] = (torch.rand(d, generator=g) * 2 - 1) * bound
    sd.update({k: v for k, v in body.items() if not k.startswith("init_embedding.")})
    return sd


def case_state_dict(case):
    env, _, _, layers, mlp_layers, wseed, _ = CASES[case]
    return make_state_dict(env, wseed, layers, mlp_layers)


def make_instance(env, b, n, seed):
    """(locs [B, N, 2], feats [B, N - 1, F]) in [0, 1): the kernel's inputs, not an environment's distribution."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(b, n, 2, generator=g), torch.rand(b, n - 1, FEATURES[env], generator=g)


def td_of(env, locs, feats):
    """The reference's td keys from the features (the depot's prize / penalty is 0)."""
    zero = torch.zeros(locs.shape[0], 1, dtype=feats.dtype)
    if env == "cvrp":
        return {"locs": locs, "demand": feats[..., 0]}
    if env == "op":
        return {"locs": locs, "prize": torch.cat((zero, feats[..., 0]), 1)}
    return {"locs": locs, "expected_prize": feats[..., 0], "penalty": torch.cat((zero, feats[..., 1]), 1)}


# ---- the graph ------------------------------------------------------------------------------------------------------------
def distances(locs):
    return (locs[..., :, None, :] - locs[..., None, :, :]).norm(p=2, dim=-1)


def select_neighbors(locs, k):
    """edge.py:136-139 for a batch: the customer block, +inf diagonal, topk; (neighbors [B, C, K] int64 in 1 .. N - 1,
    cost [B, C, K], depot_cost [B, C])."""
    cost = distances(locs)
    block = cost[:, 1:, 1:].clone()
    block.diagonal(dim1=1, dim2=2).fill_(torch.inf)
    values, indices = torch.topk(block, k=k, dim=-1, largest=False, sorted=False)
    return indices + 1, values, cost[:, 1:, 0]


def edge_list(nbr):
    """(src [B, E], dst [B, E]) in the reference's order: the kNN edges by source, all (i -> 0), all (0 -> i)."""
    b, c, k = nbr.shape
    cust = torch.arange(1, c + 1, device=nbr.device).expand(b, c)
    zero = torch.zeros(b, c, dtype=torch.int64, device=nbr.device)
    src = torch.cat((cust[:, :, None].expand(b, c, k).reshape(b, c * k), cust, zero), 1)
    dst = torch.cat((nbr.reshape(b, c * k), zero, cust), 1)
    return src, dst


def on_graph(nbr, n):
    src, dst = edge_list(nbr.long())
    on = torch.zeros(nbr.shape[0], n, n, dtype=torch.bool, device=nbr.device)
    on[torch.arange(nbr.shape[0], device=nbr.device)[:, None], src, dst] = True
    return on


def encode(sd, locs, feats, k_sparse=None, dtype=torch.float32, neighbors=None, eps=1e-5):
    """(heatmap_logits [B, N, N], node_embed [B, N, D]) of the encoder in ``dtype``. ``neighbors`` [B, C, K] fixes the
    graph; otherwise it is selected from ``locs`` in ``dtype``. The costs are always ``dtype``'s distances."""
    sd = {k: (v.to(device=locs.device, dtype=dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    locs, feats = locs.to(dtype), feats.to(dtype)
    b, n, _ = locs.shape
    layers, mlp_layers = count_layers(sd)
    silu, sigmoid = torch.nn.functional.silu, torch.sigmoid

    def lin(name, t):
        y = t @ sd[f"{name}.weight"].t()
        return y + sd[f"{name}.bias"] if f"{name}.bias" in sd else y

    def bn(name, t):
        scale = sd[f"{name}.module.weight"] / torch.sqrt(sd[f"{name}.module.running_var"] + eps)
        return (t - sd[f"{name}.module.running_mean"]) * scale + sd[f"{name}.module.bias"]

    if neighbors is None:
        nbr, _, _ = select_neighbors(locs, num_neighbors(n, k_sparse))
    else:
        nbr = neighbors.to(torch.int64)
    src, dst = edge_list(nbr)
    e = src.shape[1]
    batch = torch.arange(b, device=locs.device)[:, None]
    cost = distances(locs)[batch, src, dst]

    def rows(x, idx):  # x [B, N, D], idx [B, E] -> [B, E, D]
        return x.gather(1, idx[:, :, None].expand(-1, -1, x.shape[-1]))

    counts = torch.zeros(b, n, dtype=dtype, device=locs.device).scatter_add_(1, src, torch.ones(b, e, dtype=dtype, device=locs.device))
    node_embed = torch.cat((lin("init_embedding.init_embed_depot", locs[:, :1]),
                            lin("init_embedding.init_embed", torch.cat((locs[:, 1:], feats), -1))), 1)
    x = silu(node_embed)
    w = silu(lin("edge_embedding.edge_embed", cost[..., None]))
    for i in range(layers):
        p = f"graph_network.layers.{i}"
        x1, x2, x3, x4 = (lin(f"{p}.v_lin{j}", x) for j in (1, 2, 3, 4))
        total = torch.zeros_like(x).scatter_add_(1, src[:, :, None].expand(-1, -1, x.shape[-1]), sigmoid(w) * rows(x2, dst))
        x_new = x + silu(bn(f"{p}.v_bn", x1 + total / counts[:, :, None]))
        w = w + silu(bn(f"{p}.e_bn", lin(f"{p}.e_lin", w) + rows(x3, src) + rows(x4, dst)))
        x = x_new
    h = w
    for i in range(mlp_layers - 1):
        h = silu(lin(f"heatmap_generator.linears.{i}", h))
    prob = sigmoid(lin("heatmap_generator.output", h))[..., 0]  # [B, E]
    heat = torch.zeros(b, n, n, dtype=dtype, device=locs.device)
    heat[batch, src, dst] = prob
    return torch.log(heat + SMALL), node_embed


def edge_index_to_neighbors(edge_index, b, n):
    """The reference's batched edge_index [2, B C (K + 2)] -> neighbors [B, C, K] int64, after checking its order: the
    kNN edges by source, then all (i -> 0), then all (0 -> i)."""
    c = n - 1
    e = edge_index.shape[1] // b
    k = e // c - 2
    assert e == c * (k + 2) and edge_index.shape[1] == b * e
    local = edge_index.view(2, b, e) - (torch.arange(b) * n)[None, :, None]
    src, dst = local[0], local[1]
    nbr = dst[:, :c * k].reshape(b, c, k)
    want_src, want_dst = edge_list(nbr)
    assert torch.equal(src, want_src) and torch.equal(dst, want_dst), "the reference's edges are not kNN by source, i -> 0, 0 -> i"
    assert bool((nbr >= 1).all()) and bool((nbr < n).all())
    return nbr


def kernel_parameters(sd, device="cuda"):
    """The state dict as kernels.nargnn_depot_heatmap takes it (batch norms folded in float64, rounded once)."""
    p = T.kernel_parameters(sd, device)  # (init_w is the customers' [D, 2 + F] here)
    p["depot_w"] = sd["init_embedding.init_embed_depot.weight"].to(device=device, dtype=torch.float32).contiguous()
    p["depot_b"] = sd["init_embedding.init_embed_depot.bias"].to(device=device, dtype=torch.float32).contiguous()
    return p


# ---- the recorder -----------------------------------------------------------------------------------------------------------
def reference_run(case):
    env, n, k_sparse, layers, mlp_layers, wseed, dseed = CASES[case]
    cls = T.reference_encoder_class()
    sd = make_state_dict(env, wseed, layers, mlp_layers)
    locs, feats = make_instance(env, BATCH, n, dseed)
    seen = {}

    def build(dtype):
        enc = cls(embed_dim=D, env_name=env, num_layers_heatmap_generator=mlp_layers, num_layers_graph_encoder=layers,
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
        heat32, embed32 = enc32(td_of(env, locs.clone(), feats.clone()))
        # float64: the reference's heatmap generator refuses the dtype at its last step (log(heatmap + small_value)), so the
        # module runs up to the edge probabilities and that one step is taken here
        enc64 = build(torch.float64)
        enc64.heatmap_generator._make_heatmap_logits = lambda graph: graph
        graph, _ = enc64(td_of(env, locs.double(), feats.double()))
        nbr64 = edge_index_to_neighbors(seen[torch.float64], BATCH, n)
        src, dst = edge_list(nbr64)
        heat = torch.zeros(BATCH, n, n, dtype=torch.float64)
        heat[torch.arange(BATCH)[:, None], src, dst] = graph.edge_attr.view(BATCH, -1)
        heat64 = torch.log(heat + SMALL)
    nbr32 = edge_index_to_neighbors(seen[torch.float32], BATCH, n)
    assert torch.equal(nbr32.sort(-1).values, nbr64.sort(-1).values), "fp32 and fp64 select different neighbours: another seed"
    rec = {"locs": locs, "feats": feats, "edge_index": seen[torch.float32], "heatmap32": heat32, "heatmap64": heat64,
           "node_embed32": embed32, "weight_seed": torch.tensor(wseed),
           "weights_sha256": np.frombuffer(bytes.fromhex(state_hash(sd)), dtype=np.uint8)}
    if case in STORES_STATE_DICT:
        rec.update({f"sd/{k}": v for k, v in sd.items()})
    return rec


def reference_keys():
    """{environment: the reference module's own state_dict keys at the default depth}"""
    cls = T.reference_encoder_class()
    return {env: list(cls(embed_dim=D, env_name=env).state_dict().keys()) for env in FEATURES}


def record(case):
    from tests.helpers import reference_record

    return reference_record(f"nargnn_depot_{case}", lambda: reference_run(case))


def recorded_keys():
    from tests.helpers import REFERENCE_RECORDS

    return json.loads((REFERENCE_RECORDS / "nargnn_depot_state_dict_keys.json").read_text())


def floor32(rec):
    """The fp32 reference's own distance from its fp64 run at the graph's entries: the unit of every tolerance here."""
    b, n, _ = rec["heatmap32"].shape
    on = on_graph(edge_index_to_neighbors(rec["edge_index"], b, n), n)
    return float((rec["heatmap32"].double() - rec["heatmap64"])[on].abs().max())


if __name__ == "__main__":  # RL4CO_RECORD_REFERENCE=1 python -m tests.nargnn_depot_ref
    import os

    from tests.helpers import REFERENCE_RECORDS

    if os.environ.get("RL4CO_RECORD_REFERENCE") == "1":
        (REFERENCE_RECORDS / "nargnn_depot_state_dict_keys.json").write_text(json.dumps(reference_keys(), indent=0) + "\n")
    for name in CASES:
        r = record(name)
        print(name, "floor", floor32(r), {k: tuple(v.shape) for k, v in r.items() if not k.startswith("sd/")})
