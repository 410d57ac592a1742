"""DeepACO's heatmap encoder for the depot graphs (CVRP, OP, PCTSP) in TRAIN mode (batch norms on batch statistics): a
plain-torch restatement in edge-list form with autograd in any dtype, and the recorder of the reference's own
``NARGNNEncoder(env_name=...)`` in ``.train()`` on the CPU (tests/golden/reference/nargnn_depot_train_<case>.npz and its
``_part<i>`` files: a record is cut so that no file passes 1 MiB).

The graph helpers, the weights and the instances are tests/nargnn_depot_ref.py's; the fixed upstream gradient, the cutting
into parts and ``bound`` are tests/nargnn_train_ref.py's. A record holds, in fp32 and in float64: the heatmap logits, the
node embedding, every parameter's gradient for ``upstream_grad`` masked to the graph, and the batch norms' buffers after
the one forward. As there, the reference runs up to the edge probabilities and ``log(. + small_value)`` is taken here."""
import numpy as np
import torch

from tests import nargnn_depot_ref as R
from tests import nargnn_train_ref as T
from tests.nargnn_train_ref import bound, is_buffer, record_pairs, upstream_grad  # noqa: F401  (one statement of each)

BATCH = R.BATCH
CASES = R.CASES  # case -> (env, N with the depot, k_sparse, GNN layers, heatmap MLP layers, weight seed, data seed)
case_state_dict = R.case_state_dict


# ---- the restatement --------------------------------------------------------------------------------------------------------
def _forward(p, buffers, locs, feats, nbr, layers, mlp_layers, eps=1e-5, momentum=0.1):
    """The train-mode forward on GIVEN tensors ``p`` by ``state_dict`` key. ``buffers`` (or None) receives BatchNorm1d's
    own train-mode update."""
    b, n, _ = locs.shape
    dev, dtype = locs.device, locs.dtype
    silu, sigmoid = torch.nn.functional.silu, torch.sigmoid

    def lin(name, t):
        return torch.nn.functional.linear(t, p[f"{name}.weight"], p.get(f"{name}.bias"))

    def bn(name, t):  # over the flat rows: batch mean, biased variance; the running variance takes the unbiased one
        rows = t.reshape(-1, t.shape[-1])
        if buffers is None:
            mean, var = rows.mean(0), rows.var(0, unbiased=False)
            return (t - mean) / torch.sqrt(var + eps) * p[f"{name}.module.weight"] + p[f"{name}.module.bias"]
        buffers[f"{name}.module.num_batches_tracked"] += 1
        y = torch.nn.functional.batch_norm(rows, buffers[f"{name}.module.running_mean"], buffers[f"{name}.module.running_var"],
                                           p[f"{name}.module.weight"], p[f"{name}.module.bias"], True, momentum, eps)
        return y.view(t.shape)

    src, dst = R.edge_list(nbr)
    e = src.shape[1]
    batch = torch.arange(b, device=dev)[:, None]
    cost = R.distances(locs)[batch, src, dst]

    def rows_of(x, idx):  # x [B, N, D], idx [B, E] -> [B, E, D]
        return x.gather(1, idx[:, :, None].expand(-1, -1, x.shape[-1]))

    counts = torch.zeros(b, n, dtype=dtype, device=dev).scatter_add_(1, src, torch.ones(b, e, dtype=dtype, device=dev))
    node_embed = torch.cat((lin("init_embedding.init_embed_depot", locs[:, :1]),
                            lin("init_embedding.init_embed", torch.cat((locs[:, 1:], feats), -1))), 1)
    x = silu(node_embed)
    w = silu(lin("edge_embedding.edge_embed", cost[..., None]))
    for i in range(layers):
        q = f"graph_network.layers.{i}"
        x1, x2, x3, x4 = (lin(f"{q}.v_lin{j}", x) for j in (1, 2, 3, 4))
        total = torch.zeros_like(x).scatter_add(1, src[:, :, None].expand(-1, -1, x.shape[-1]), sigmoid(w) * rows_of(x2, dst))
        x_new = x + silu(bn(f"{q}.v_bn", x1 + total / counts[:, :, None]))  # the segment mean by source
        w = w + silu(bn(f"{q}.e_bn", lin(f"{q}.e_lin", w) + rows_of(x3, src) + rows_of(x4, dst)))
        x = x_new
    h = w
    for i in range(mlp_layers - 1):
        h = silu(lin(f"heatmap_generator.linears.{i}", h))
    prob = sigmoid(lin("heatmap_generator.output", h))[..., 0]  # [B, E]
    heat = torch.zeros(b, n, n, dtype=dtype, device=dev).index_put((batch, src, dst), prob)
    return torch.log(heat + R.SMALL), node_embed


def encode_train(sd, locs, feats, k_sparse=None, dtype=torch.float32, neighbors=None):
    """One train-mode forward of the encoder in ``dtype`` on autograd. Returns ``(logits [B, N, N], node_embed, params,
    buffers, neighbors)``: ``params`` the leaf tensors by ``state_dict`` key, ``buffers`` the batch norms' buffers AFTER
    the forward."""
    dev = locs.device
    params = {k: v.detach().to(device=dev, dtype=dtype).clone().requires_grad_() for k, v in sd.items() if not is_buffer(k)}
    buffers = {k: (v.detach().to(device=dev, dtype=dtype) if v.is_floating_point() else v.detach().to(dev)).clone()
               for k, v in sd.items() if is_buffer(k)}
    locs, feats = locs.to(dtype), feats.to(dtype)
    if neighbors is None:
        nbr, _, _ = R.select_neighbors(locs, R.num_neighbors(locs.shape[1], k_sparse))
    else:
        nbr = neighbors.to(device=dev, dtype=torch.int64)
    logits, embed = _forward(params, buffers, locs, feats, nbr, *R.count_layers(sd))
    return logits, embed, params, buffers, nbr


def run(sd, locs, feats, neighbors, dtype, upstream=None):
    """Forward, backward under ``upstream`` (default: ``upstream_grad`` on the graph) -> dict of detached results."""
    logits, embed, params, buffers, nbr = encode_train(sd, locs, feats, dtype=dtype, neighbors=neighbors)
    b, n = locs.shape[:2]
    g = upstream_grad(b, n) if upstream is None else upstream
    logits.backward((g.to(logits.device) * R.on_graph(nbr, n)).to(dtype))
    out = {"heatmap": logits.detach(), "node_embed": embed.detach()}
    out.update({f"grad/{k}": (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in params.items()})
    out.update({f"buf/{k}": v for k, v in buffers.items()})
    return out


class ModuleAsEncoder(torch.nn.Module):
    """The restatement as a differentiable ``encoder=`` for NonAutoregressivePolicy (the bench's torch baseline): its
    parameters are the ``state_dict``'s, its forward is ``_forward`` on them (buffers untouched)."""

    def __init__(self, sd, env, k_sparse=None):
        super().__init__()
        self.keys = [k for k in sd if not is_buffer(k)]
        self.env, self.k_sparse = env, k_sparse
        self.values = torch.nn.ParameterList([torch.nn.Parameter(sd[k].clone().float()) for k in self.keys])
        self.depth = R.count_layers(sd)

    def forward(self, td):
        from rl4co_amd.nargnn import _depot_features

        locs = td["locs"]
        with torch.no_grad():
            nbr, _, _ = R.select_neighbors(locs, R.num_neighbors(locs.shape[1], self.k_sparse))
        return _forward(dict(zip(self.keys, self.values)), None, locs, _depot_features(self.env, td), nbr, *self.depth)


# ---- incoming edges, by brute force -------------------------------------------------------------------------------------------
def incoming_csr_bruteforce(neighbors):
    """The CSR over the targets of the depot graph's rows, one row and one node at a time."""
    b, c, k = neighbors.shape
    n, e = c + 1, c * (k + 2)
    ptr, src = [0], []
    for j in range(b * n):
        for row in range(b * e):
            bb, r = divmod(row, e)
            if r < c * k:
                target = int(neighbors[bb, r // k, r % k])
            elif r < c * k + c:
                target = 0
            else:
                target = r - c * k - c + 1
            if bb * n + target == j:
                src.append(row)
        ptr.append(len(src))
    return torch.tensor(ptr, dtype=torch.int32), torch.tensor(src, dtype=torch.int32)


# ---- the recorder ---------------------------------------------------------------------------------------------------------------
def _reference_once(case, dseed):
    env, n, k_sparse, layers, mlp_layers, wseed, _ = CASES[case]
    cls = R.T.reference_encoder_class()
    sd = R.make_state_dict(env, wseed, layers, mlp_layers)
    locs, feats = R.make_instance(env, BATCH, n, dseed)
    rec = {"locs": locs, "feats": feats, "data_seed": torch.tensor(dseed),
           "weights_sha256": np.frombuffer(bytes.fromhex(R.state_hash(sd)), dtype=np.uint8)}
    sets = {}
    batch = torch.arange(BATCH)[:, None]
    for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
        seen = {}
        enc = cls(embed_dim=R.D, env_name=env, num_layers_heatmap_generator=mlp_layers, num_layers_graph_encoder=layers,
                  k_sparse=k_sparse)
        enc.load_state_dict(sd, strict=True)
        enc = enc.to(dtype).train()
        inner = enc.edge_embedding._cost_matrix_to_graph

        def keep(cost, emb, inner=inner, seen=seen):
            graph = inner(cost, emb)
            seen["edge_index"] = graph.edge_index.clone()
            return graph

        enc.edge_embedding._cost_matrix_to_graph = keep
        enc.heatmap_generator._make_heatmap_logits = lambda graph: graph
        graph, embed = enc(R.td_of(env, locs.to(dtype), feats.to(dtype)))
        nbr = R.edge_index_to_neighbors(seen["edge_index"], BATCH, n)
        sets[tag] = nbr.sort(-1).values
        src, dst = R.edge_list(nbr)
        heat = torch.zeros(BATCH, n, n, dtype=dtype).index_put((batch, src, dst), graph.edge_attr.view(BATCH, -1))
        heat = torch.log(heat + R.SMALL)
        heat.backward((upstream_grad(BATCH, n) * R.on_graph(nbr, n)).to(dtype))
        rec[f"heatmap{tag}"], rec[f"node_embed{tag}"] = heat.detach(), embed.detach()
        if tag == "32":
            rec["edge_index"] = seen["edge_index"]
        named = dict(enc.named_parameters())
        for key, value in enc.state_dict().items():
            if is_buffer(key):
                rec[f"buf/{key}/{tag}"] = value.detach().clone()
            else:
                grad = named[key].grad  # (None: the last layer's node update reaches no output)
                rec[f"grad/{key}/{tag}"] = torch.zeros_like(named[key]) if grad is None else grad.detach().clone()
    return rec if torch.equal(sets["32"], sets["64"]) else None


def reference_run(case):
    """The record of ``case``: fp32 and float64 must have selected the same neighbour sets; where they did not, the data
    seed moves on by 1000 (the seed taken is in the record)."""
    for attempt in range(8):
        rec = _reference_once(case, CASES[case][6] + 1000 * attempt)
        if rec is not None:
            return rec
    raise AssertionError("fp32 and fp64 select different neighbours at every seed tried")


def record(case):
    """The case's record, its part files joined. ``RL4CO_RECORD_REFERENCE=1`` (reference checkout present) rewrites them."""
    import os

    from tests.helpers import REFERENCE_RECORDS, reference_record

    name = f"nargnn_depot_train_{case}"
    if os.environ.get("RL4CO_RECORD_REFERENCE") == "1":
        parts = T._parts(reference_run(case))
        for old in REFERENCE_RECORDS.glob(f"{name}_part*.npz"):
            old.unlink()
        for i, part in enumerate(parts):
            reference_record(name if i == 0 else f"{name}_part{i}", lambda part=part: part)
    rec = {}
    for path in [REFERENCE_RECORDS / f"{name}.npz"] + sorted(REFERENCE_RECORDS.glob(f"{name}_part*.npz")):
        with np.load(path) as z:
            rec.update({k: torch.from_numpy(z[k].copy()) for k in z.files})
    return rec


if __name__ == "__main__":  # RL4CO_RECORD_REFERENCE=1 python -m tests.nargnn_depot_train_ref
    for name in CASES:
        r = record(name)
        print(name, len(r), "arrays; data seed", int(r["data_seed"]), "heatmap floor",
              float((r["heatmap32"].double() - r["heatmap64"]).abs().max()))
