"""DeepACO's heatmap encoder in TRAIN mode (batch norms on batch statistics): a dense plain-torch restatement with autograd
in any dtype, and the recorder of the reference's own ``NARGNNEncoder`` in ``.train()`` on the CPU
(tests/golden/reference/nargnn_train_<case>.npz and its ``_part<i>`` files: a record is cut so that no file passes 1 MiB).

Weights, the stand-in ``torch_geometric`` and the loader of the reference class are tests/nargnn_ref.py's. A record holds, in
fp32 and in float64: the heatmap logits, the node embedding, every parameter's gradient for the fixed upstream
``upstream_grad`` (|g| <= 1 on the graph's entries, 0 elsewhere) and the batch norms' buffers after the one forward. The
reference's heatmap generator refuses float64 at its last step (``log(heatmap + small_value)``), so in both dtypes the module
runs up to the edge probabilities and that one step is taken here.

The tolerance every comparison of a kernel result uses is ``bound(ref32, ref64)``: four times the fp32 reference's own
distance from float64, and never less than four units in the last place of the tensor's largest value."""
import numpy as np
import torch

from tests import nargnn_ref as R

BATCH = 3
# case -> (N, k_sparse, GNN layers, heatmap MLP layers, weight seed, data seed)
CASES = {"n11": (11, None, 1, 2, 301, 401), "n20_full": (20, None, 15, 5, 302, 402), "n60_k17": (60, 17, 2, 2, 303, 403)}
PART_BYTES = 900 * 1024
BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def is_buffer(key):
    return key.rsplit(".", 1)[1] in BUFFERS


def upstream_grad(b, n, seed=77):
    """The fixed gradient of the heatmap logits, [B, N, N] in (-1, 1); the caller masks it to the graph."""
    return torch.rand(b, n, n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1


def graph_mask(nbr, n):
    return torch.zeros(nbr.shape[0], n, n, dtype=torch.bool, device=nbr.device).scatter_(2, nbr.long(), True)


def bound(ref32, ref64):
    ref64 = ref64.double()
    return 4 * max(float((ref32.double() - ref64).abs().max()), 2.0 ** -23 * float(ref64.abs().max()))


# ---- the restatement --------------------------------------------------------------------------------------------------------
def encode_train(sd, locs, k_sparse=None, dtype=torch.float32, neighbors=None, eps=1e-5, momentum=0.1):
    """One train-mode forward of the encoder in ``dtype`` on autograd. Returns ``(logits [B, N, N], node_embed, params,
    buffers, neighbors)``: ``params`` the leaf tensors by ``state_dict`` key (call ``logits.backward(g)`` and read their
    ``.grad``), ``buffers`` the batch norms' buffers AFTER the forward."""
    dev = locs.device
    params = {k: v.detach().to(device=dev, dtype=dtype).clone().requires_grad_() for k, v in sd.items() if not is_buffer(k)}
    buffers = {k: (v.detach().to(device=dev, dtype=dtype) if v.is_floating_point() else v.detach().to(dev)).clone()
               for k, v in sd.items() if is_buffer(k)}
    locs = locs.to(dtype)
    layers, mlp_layers = R.count_layers(sd)
    silu, sigmoid = torch.nn.functional.silu, torch.sigmoid

    def lin(name, t):
        y = t @ params[f"{name}.weight"].t()
        return y + params[f"{name}.bias"] if f"{name}.bias" in params else y

    def bn(name, t):
        # BatchNorm1d's own train-mode step over the flat rows (batch mean, biased variance; the running variance takes the
        # unbiased one), as the reference's layer calls it
        buffers[f"{name}.module.num_batches_tracked"] += 1
        y = torch.nn.functional.batch_norm(t.reshape(-1, t.shape[-1]), buffers[f"{name}.module.running_mean"],
                                           buffers[f"{name}.module.running_var"], params[f"{name}.module.weight"],
                                           params[f"{name}.module.bias"], True, momentum, eps)
        return y.view(t.shape)

    if neighbors is None:
        nbr, cost = R.select_neighbors(locs, R.num_neighbors(locs.shape[1], k_sparse))
    else:
        nbr = neighbors.to(device=dev, dtype=torch.int64)
        cost = (locs[:, :, None, :] - R.gather_nodes(locs, nbr)).norm(p=2, dim=-1)
    node_embed = lin("init_embedding.init_embed", locs)
    x = silu(node_embed)
    w = silu(lin("edge_embedding.edge_embed", cost[..., None]))
    for i in range(layers):
        p = f"graph_network.layers.{i}"
        x1, x2, x3, x4 = (lin(f"{p}.v_lin{j}", x) for j in (1, 2, 3, 4))
        agg = (sigmoid(w) * R.gather_nodes(x2, nbr)).mean(2)
        x_new = x + silu(bn(f"{p}.v_bn", x1 + agg))
        w = w + silu(bn(f"{p}.e_bn", lin(f"{p}.e_lin", w) + x3[:, :, None, :] + R.gather_nodes(x4, nbr)))
        x = x_new
    h = w
    for i in range(mlp_layers - 1):
        h = silu(lin(f"heatmap_generator.linears.{i}", h))
    prob = sigmoid(lin("heatmap_generator.output", h))[..., 0]
    heat = torch.zeros(locs.shape[0], locs.shape[1], locs.shape[1], dtype=dtype, device=dev).scatter(2, nbr, prob)
    return torch.log(heat + R.SMALL), node_embed, params, buffers, nbr


def run(sd, locs, neighbors, dtype, upstream=None):
    """Forward, backward under ``upstream`` (default: ``upstream_grad`` on the graph) -> dict of detached results."""
    logits, embed, params, buffers, nbr = encode_train(sd, locs, dtype=dtype, neighbors=neighbors)
    b, n = locs.shape[:2]
    g = upstream_grad(b, n) if upstream is None else upstream
    logits.backward((g.to(logits.device) * graph_mask(nbr, n)).to(dtype))
    out = {"heatmap": logits.detach(), "node_embed": embed.detach()}
    out.update({f"grad/{k}": (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in params.items()})
    out.update({f"buf/{k}": v for k, v in buffers.items()})
    return out


class ModuleAsEncoder(torch.nn.Module):
    """The restatement as a differentiable ``encoder=`` for DeepACOPolicy (the bench's torch baseline): its parameters are
    the ``state_dict``'s, its forward is ``encode_train`` on them."""

    def __init__(self, sd, k_sparse=None):
        super().__init__()
        self.keys = [k for k in sd if not is_buffer(k)]
        self.k_sparse = k_sparse
        self.values = torch.nn.ParameterList([torch.nn.Parameter(sd[k].clone().float()) for k in self.keys])
        self.depth = R.count_layers(sd)

    def forward(self, td):
        locs = td["locs"]
        return _forward_on(dict(zip(self.keys, self.values)), locs, self.k_sparse, *self.depth)


def _forward_on(p, locs, k_sparse, layers, mlp_layers, eps=1e-5):
    """``encode_train``'s forward on GIVEN tensors (no copies, buffers untouched): what autograd differentiates in the bench."""
    silu, sigmoid = torch.nn.functional.silu, torch.sigmoid

    def lin(name, t):
        return torch.nn.functional.linear(t, p[f"{name}.weight"], p.get(f"{name}.bias"))

    def bn(name, t):
        rows = t.reshape(-1, t.shape[-1])
        mean, var = rows.mean(0), rows.var(0, unbiased=False)
        return (t - mean) / torch.sqrt(var + eps) * p[f"{name}.module.weight"] + p[f"{name}.module.bias"]

    with torch.no_grad():
        nbr, cost = R.select_neighbors(locs, R.num_neighbors(locs.shape[1], k_sparse))
    node_embed = lin("init_embedding.init_embed", locs)
    x = silu(node_embed)
    w = silu(lin("edge_embedding.edge_embed", cost[..., None]))
    for i in range(layers):
        q = f"graph_network.layers.{i}"
        x1, x2, x3, x4 = (lin(f"{q}.v_lin{j}", x) for j in (1, 2, 3, 4))
        agg = (sigmoid(w) * R.gather_nodes(x2, nbr)).mean(2)
        x_new = x + silu(bn(f"{q}.v_bn", x1 + agg))
        w = w + silu(bn(f"{q}.e_bn", lin(f"{q}.e_lin", w) + x3[:, :, None, :] + R.gather_nodes(x4, nbr)))
        x = x_new
    h = w
    for i in range(mlp_layers - 1):
        h = silu(lin(f"heatmap_generator.linears.{i}", h))
    prob = sigmoid(lin("heatmap_generator.output", h))[..., 0]
    heat = torch.zeros(locs.shape[0], locs.shape[1], locs.shape[1], dtype=prob.dtype, device=locs.device).scatter(2, nbr, prob)
    return torch.log(heat + R.SMALL), node_embed


# ---- incoming edges, by brute force -------------------------------------------------------------------------------------------
def incoming_csr_bruteforce(neighbors):
    b, n, k = neighbors.shape
    ptr, src = [0], []
    for j in range(b * n):
        for e in range(b * n * k):
            i, kk = divmod(e, k)
            if (i // n) * n + int(neighbors[i // n, i % n, kk]) == j:
                src.append(e)
        ptr.append(len(src))
    return torch.tensor(ptr, dtype=torch.int32), torch.tensor(src, dtype=torch.int32)


# ---- the recorder ---------------------------------------------------------------------------------------------------------------
def case_state_dict(case):
    _, _, layers, mlp_layers, wseed, _ = CASES[case]
    return R.make_state_dict(wseed, layers, mlp_layers)


def reference_run(case):
    n, k_sparse, layers, mlp_layers, wseed, dseed = CASES[case]
    cls = R.reference_encoder_class()
    sd = R.make_state_dict(wseed, layers, mlp_layers)
    locs = torch.rand(BATCH, n, 2, generator=torch.Generator().manual_seed(dseed))
    rec = {"locs": locs, "weights_sha256": np.frombuffer(bytes.fromhex(R.state_hash(sd)), dtype=np.uint8)}
    sets = {}
    for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
        seen = {}
        enc = cls(embed_dim=R.D, env_name="tsp", num_layers_heatmap_generator=mlp_layers, num_layers_graph_encoder=layers,
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
        graph, embed = enc({"locs": locs.to(dtype)})
        nbr = R.edge_index_to_neighbors(seen["edge_index"], BATCH, n)
        sets[tag] = nbr.sort(-1).values
        heat = torch.log(torch.zeros(BATCH, n, n, dtype=dtype).scatter(2, nbr, graph.edge_attr.view(BATCH, n, -1)) + R.SMALL)
        heat.backward((upstream_grad(BATCH, n) * graph_mask(nbr, n)).to(dtype))
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
    assert torch.equal(sets["32"], sets["64"]), "fp32 and fp64 select different neighbours: another seed"
    return rec


def _parts(rec):
    parts, size = [{}], 0
    for key, value in rec.items():
        nbytes = value.numel() * value.element_size() if torch.is_tensor(value) else np.asarray(value).nbytes
        if size + nbytes > PART_BYTES and parts[-1]:
            parts.append({})
            size = 0
        parts[-1][key] = value
        size += nbytes
    return parts


def record(case):
    """The case's record, its part files joined. ``RL4CO_RECORD_REFERENCE=1`` (reference checkout present) rewrites them."""
    import os

    from tests.helpers import REFERENCE_RECORDS, reference_record

    name = f"nargnn_train_{case}"
    if os.environ.get("RL4CO_RECORD_REFERENCE") == "1":
        parts = _parts(reference_run(case))
        for old in REFERENCE_RECORDS.glob(f"{name}_part*.npz"):
            old.unlink()
        for i, part in enumerate(parts):
            reference_record(name if i == 0 else f"{name}_part{i}", lambda part=part: part)
    rec = {}
    for path in [REFERENCE_RECORDS / f"{name}.npz"] + sorted(REFERENCE_RECORDS.glob(f"{name}_part*.npz")):
        with np.load(path) as z:
            rec.update({k: torch.from_numpy(z[k].copy()) for k in z.files})
    return rec


def record_pairs(rec):
    """name -> (ref32, ref64) for every recorded result (heatmap, node_embed, grad/<key>, buf/<key>)."""
    pairs = {"heatmap": (rec["heatmap32"], rec["heatmap64"]), "node_embed": (rec["node_embed32"], rec["node_embed64"])}
    for key in rec:
        if key.startswith(("grad/", "buf/")) and key.endswith("/64"):
            pairs[key[:-3]] = (rec[key[:-3] + "/32"], rec[key])
    return pairs


if __name__ == "__main__":  # RL4CO_RECORD_REFERENCE=1 python -m tests.nargnn_train_ref
    for name in CASES:
        r = record(name)
        print(name, len(r), "arrays; heatmap floor", float((r["heatmap32"].double() - r["heatmap64"]).abs().max()))
