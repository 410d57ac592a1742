"""GFACS's encoder (models/zoo/gfacs/encoder.py: DeepACO's heatmap encoder plus the log-partition head ``Z_net``) in TRAIN
mode: a plain-torch restatement of the head alone and of the whole encoder with the head, with autograd in any dtype, and the
recorder of the reference's own ``GFACSEncoder`` in ``.train()`` on the CPU (tests/golden/reference/gfacs_<case>.npz and its
``_part<i>`` files: a record is cut so that no file passes 1 MiB).

The weights, the graph helpers, the stand-in ``torch_geometric`` and the loader of the reference's package are
tests/nargnn_ref.py's and tests/nargnn_depot_ref.py's; the fixed upstream gradient of the heatmap, the cutting into parts
and ``bound`` are tests/nargnn_train_ref.py's. The restatement runs both graphs in edge-list form (a TSP node's K rows, then
the next node's: the kernel's own order) so that the stack's output ``w`` [B, E, 64] is there for the head; without the head
it is tests/nargnn_train_ref.py's and tests/nargnn_depot_train_ref.py's restatement, which tests/test_gfacs_cpu.py checks.

A record holds, in fp32 and in float64: ``logZ``, the heatmap logits, the node embedding, every parameter's gradient for the
fixed upstream pair (``upstream_grad`` on the graph for the heatmap, ``upstream_logz`` for ``logZ``) and the batch norms'
buffers after the one forward. B = 3: the reference's pooling (``reshape(-1, B, Z).mean(0)``, a stride over the instances)
and the per-instance mean then give different numbers, which is how the record settles which one the reference computes."""
import importlib
import math
import sys

import numpy as np
import torch

from tests import nargnn_depot_ref as RD
from tests import nargnn_ref as R
from tests import nargnn_train_ref as T
from tests.nargnn_train_ref import bound, is_buffer, upstream_grad  # noqa: F401  (one statement of each)

D = R.D
BATCH = 3
# case -> (env, N, z_out_dim, GNN layers, heatmap MLP layers, weight seed, data seed)
CASES = {"tsp_n11": ("tsp", 11, 2, 2, 2, 501, 601), "cvrp_n12": ("cvrp", 12, 1, 2, 2, 502, 602)}
Z_KEYS = ("Z_net.0.weight", "Z_net.0.bias", "Z_net.2.weight", "Z_net.2.bias")


def upstream_logz(b, z, seed=78):
    """The fixed gradient of ``logZ``, [B, Z] in (-1, 1)."""
    return torch.rand(b, z, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1


# ---- weights --------------------------------------------------------------------------------------------------------------
def z_net_state_dict(seed, z_out_dim, d=D):
    g = torch.Generator().manual_seed(seed + 13)
    bound_ = d ** -0.5
    shapes = {"Z_net.0.weight": (d, d), "Z_net.0.bias": (d,), "Z_net.2.weight": (z_out_dim, d), "Z_net.2.bias": (z_out_dim,)}
    return {key: (torch.rand(*shape, generator=g) * 2 - 1) * bound_ for key, shape in shapes.items()}


def make_state_dict(env, seed, layers, mlp_layers, z_out_dim, linear_bias=True):
    """The seeded state dict of the env's heatmap encoder and, behind it as in the reference, ``Z_net``'s four tensors."""
    body = (R.make_state_dict(seed, layers, mlp_layers, linear_bias) if env == "tsp"
            else RD.make_state_dict(env, seed, layers, mlp_layers, linear_bias))
    return {**body, **z_net_state_dict(seed, z_out_dim)}


def case_state_dict(case):
    env, _, z, layers, mlp_layers, wseed, _ = CASES[case]
    return make_state_dict(env, wseed, layers, mlp_layers, z)


def make_instance(env, b, n, seed):
    """(locs [B, N, 2], feats [B, N - 1, F] or None for tsp)"""
    if env == "tsp":
        return torch.rand(b, n, 2, generator=torch.Generator().manual_seed(seed)), None
    return RD.make_instance(env, b, n, seed)


# ---- the restatement --------------------------------------------------------------------------------------------------------
def head(w, W1, b1, W2, b2, batch, pooling="reference"):
    """``Z_net`` over the flat edge rows and the pooled mean: ``w`` [..., 64] batch-major -> ``logZ`` [B, Z]."""
    z = torch.nn.functional.silu(w.reshape(-1, w.shape[-1]) @ W1.t() + b1) @ W2.t() + b2
    if pooling == "reference":  # gfacs/encoder.py:62 as written
        return z.reshape(-1, batch, z.shape[-1]).mean(0)
    return z.reshape(batch, -1, z.shape[-1]).mean(1)


def edge_list(env, nbr):
    """(src [B, E], dst [B, E]) in the kernels' row order."""
    if env != "tsp":
        return RD.edge_list(nbr)
    b, n, k = nbr.shape
    src = torch.arange(n, device=nbr.device)[None, :, None].expand(b, n, k).reshape(b, n * k)
    return src, nbr.reshape(b, n * k)


def forward(p, buffers, env, locs, feats, nbr, layers, mlp_layers, pooling="reference", eps=1e-5, momentum=0.1):
    """The train-mode forward on GIVEN tensors ``p`` by ``state_dict`` key -> ``(logits [B, N, N], node_embed, logZ, w)``.
    ``buffers`` receives BatchNorm1d's own train-mode update."""
    b, n, _ = locs.shape
    dev, dtype = locs.device, locs.dtype
    silu, sigmoid = torch.nn.functional.silu, torch.sigmoid

    def lin(name, t):
        return torch.nn.functional.linear(t, p[f"{name}.weight"], p.get(f"{name}.bias"))

    def bn(name, t):  # over the flat rows: batch mean, biased variance; the running variance takes the unbiased one
        buffers[f"{name}.module.num_batches_tracked"] += 1
        y = torch.nn.functional.batch_norm(t.reshape(-1, t.shape[-1]), buffers[f"{name}.module.running_mean"],
                                           buffers[f"{name}.module.running_var"], p[f"{name}.module.weight"],
                                           p[f"{name}.module.bias"], True, momentum, eps)
        return y.view(t.shape)

    def rows_of(x, idx):  # x [B, N, D], idx [B, E] -> [B, E, D]
        return x.gather(1, idx[:, :, None].expand(-1, -1, x.shape[-1]))

    src, dst = edge_list(env, nbr)
    e = src.shape[1]
    batch = torch.arange(b, device=dev)[:, None]
    cost = RD.distances(locs)[batch, src, dst]
    counts = torch.zeros(b, n, dtype=dtype, device=dev).scatter_add_(1, src, torch.ones(b, e, dtype=dtype, device=dev))
    if env == "tsp":
        node_embed = lin("init_embedding.init_embed", locs)
    else:
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
    logz = head(w, *(p[key] for key in Z_KEYS), b, pooling)
    h = w
    for i in range(mlp_layers - 1):
        h = silu(lin(f"heatmap_generator.linears.{i}", h))
    prob = sigmoid(lin("heatmap_generator.output", h))[..., 0]  # [B, E]
    heat = torch.zeros(b, n, n, dtype=dtype, device=dev).index_put((batch, src, dst), prob)
    return torch.log(heat + R.SMALL), node_embed, logz, w


def on_graph(env, nbr, n):
    return T.graph_mask(nbr, n) if env == "tsp" else RD.on_graph(nbr, n)


def encode_train(sd, env, locs, feats, nbr, dtype=torch.float32, pooling="reference"):
    """One train-mode forward in ``dtype`` on autograd -> ``(logits, node_embed, logZ, params, buffers)``: ``params`` the
    leaf tensors by ``state_dict`` key, ``buffers`` the batch norms' buffers AFTER the forward."""
    dev = locs.device
    params = {k: v.detach().to(device=dev, dtype=dtype).clone().requires_grad_() for k, v in sd.items() if not is_buffer(k)}
    buffers = {k: (v.detach().to(device=dev, dtype=dtype) if v.is_floating_point() else v.detach().to(dev)).clone()
               for k, v in sd.items() if is_buffer(k)}
    body = {k: v for k, v in sd.items() if not k.startswith("Z_net.")}
    logits, embed, logz, _ = forward(params, buffers, env, locs.to(dtype), None if feats is None else feats.to(dtype),
                                     nbr.to(device=dev, dtype=torch.int64), *R.count_layers(body), pooling=pooling)
    return logits, embed, logz, params, buffers


def run(sd, env, locs, feats, nbr, dtype, pooling="reference"):
    """Forward, backward under the fixed upstream pair -> dict of detached results (the record's names)."""
    logits, embed, logz, params, buffers = encode_train(sd, env, locs, feats, nbr, dtype, pooling)
    b, n = locs.shape[:2]
    g_heat = (upstream_grad(b, n).to(logits.device) * on_graph(env, nbr.to(logits.device), n)).to(dtype)
    torch.autograd.backward([logits, logz], [g_heat, upstream_logz(b, logz.shape[1]).to(device=logits.device, dtype=dtype)])
    out = {"heatmap": logits.detach(), "node_embed": embed.detach(), "logZ": logz.detach()}
    out.update({f"grad/{k}": (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in params.items()})
    out.update({f"buf/{k}": v for k, v in buffers.items()})
    return out


# ---- the loss, restated --------------------------------------------------------------------------------------------------------
def reference_log_pb_cvrp(actions, n_ants):
    """gfacs/model.py:145-153, its numpy / scipy lines as they stand."""
    import scipy.special

    _a1 = actions.detach().cpu().numpy()
    n_nodes = np.count_nonzero(_a1, axis=1)
    _a2 = _a1[:, 1:] - _a1[:, :-1]
    n_routes = np.count_nonzero(_a2, axis=1) - n_nodes
    _a3 = _a1[:, 2:] - _a1[:, :-2]
    n_multinode_routes = np.count_nonzero(_a3, axis=1) - n_nodes
    log_b_p = -scipy.special.gammaln(n_routes + 1) - n_multinode_routes * math.log(2)
    return torch.from_numpy(log_b_p).to(actions.device).view(n_ants, -1).t()  # ops.unbatchify


def tb_loss(out, env, alpha, beta, ls, dtype=torch.float64):
    """gfacs/model.py:107-138 line by line in ``dtype``, the cvrp term from its numpy lines."""
    out = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in out.items()}
    reward = out["reward"]
    n_ants = reward.size(1)

    def log_pb(actions):
        if env == "tsp":
            return math.log(1 / 2 * actions.size(1))
        return reference_log_pb_cvrp(actions, n_ants) if env == "cvrp" else math.log(1 / 2)

    advantage = reward - reward.mean(dim=1, keepdim=True)
    if ls:
        ls_reward = out["ls_reward"]
        ls_advantage = ls_reward - ls_reward.mean(dim=1, keepdim=True)
        weighted_advantage = advantage * (1 - alpha) + ls_advantage * alpha
    else:
        weighted_advantage = advantage
    forward_flow = out["log_likelihood"] + out["logZ"].repeat(1, n_ants)
    backward_flow = log_pb(out["actions"]) + weighted_advantage.detach() * beta
    tb_loss = torch.pow(forward_flow - backward_flow, 2).mean()
    if ls:
        ls_forward_flow = out["ls_log_likelihood"] + out["ls_logZ"].repeat(1, n_ants)
        ls_backward_flow = log_pb(out["ls_actions"]) + ls_advantage.detach() * beta
        tb_loss = tb_loss + torch.pow(ls_forward_flow - ls_backward_flow, 2).mean()
    return tb_loss


# ---- the recorder ---------------------------------------------------------------------------------------------------------------
def reference_encoder_class():
    """The reference's GFACSEncoder, its file executed verbatim on tests/nargnn_ref.py's loader; one more empty package
    shell keeps the gfacs package's ``__init__`` (the lightning model) out."""
    from oracle import ref_import

    R.reference_encoder_class()
    pkg = "rl4co.models.zoo.gfacs"
    if pkg not in sys.modules:
        mod = ref_import._Shell(pkg)
        mod.__path__ = [str(ref_import.REFERENCE_ROOT / pkg.replace(".", "/"))]
        mod.__package__ = pkg
        sys.modules[pkg] = mod
        setattr(sys.modules[pkg.rpartition(".")[0]], pkg.rpartition(".")[2], mod)
    return importlib.import_module("rl4co.models.zoo.gfacs.encoder").GFACSEncoder


def reference_keys():
    """{environment: the reference module's own state_dict keys at the default depth}"""
    cls = reference_encoder_class()
    return {env: list(cls(embed_dim=D, env_name=env, z_out_dim=2).state_dict().keys()) for env in ("tsp", "cvrp", "op", "pctsp")}


def _reference_once(case, dseed):
    env, n, z, layers, mlp_layers, wseed, _ = CASES[case]
    cls = reference_encoder_class()
    from tensordict import TensorDict  # (the loader's stand-in: len(td) is the batch size, which encoder.py:62 reads)

    sd = make_state_dict(env, wseed, layers, mlp_layers, z)
    locs, feats = make_instance(env, BATCH, n, dseed)
    rec = {"locs": locs, "data_seed": torch.tensor(dseed), "weights_sha256": np.frombuffer(bytes.fromhex(R.state_hash(sd)), dtype=np.uint8)}
    if feats is not None:
        rec["feats"] = feats
    sets = {}
    batch = torch.arange(BATCH)[:, None]
    for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
        seen = {}
        enc = cls(embed_dim=D, env_name=env, num_layers_heatmap_generator=mlp_layers, num_layers_graph_encoder=layers, z_out_dim=z)
        enc.load_state_dict(sd, strict=True)
        enc = enc.to(dtype).train()
        inner = enc.edge_embedding._cost_matrix_to_graph

        def keep(cost, emb, inner=inner, seen=seen):
            graph = inner(cost, emb)
            seen["edge_index"] = graph.edge_index.clone()
            return graph

        enc.edge_embedding._cost_matrix_to_graph = keep
        enc.heatmap_generator._make_heatmap_logits = lambda graph: graph  # (float64 is refused at log(. + small_value))
        source = {"locs": locs.to(dtype)} if env == "tsp" else RD.td_of(env, locs.to(dtype), feats.to(dtype))
        graph, embed, logz = enc(TensorDict(source, batch_size=[BATCH]))
        if env == "tsp":
            nbr = R.edge_index_to_neighbors(seen["edge_index"], BATCH, n)
        else:
            nbr = RD.edge_index_to_neighbors(seen["edge_index"], BATCH, n)
        sets[tag] = nbr.sort(-1).values
        src, dst = edge_list(env, nbr)
        heat = torch.zeros(BATCH, n, n, dtype=dtype).index_put((batch, src, dst), graph.edge_attr.view(BATCH, -1))
        heat = torch.log(heat + R.SMALL)
        g_heat = (upstream_grad(BATCH, n) * on_graph(env, nbr, n)).to(dtype)
        torch.autograd.backward([heat, logz], [g_heat, upstream_logz(BATCH, z).to(dtype)])
        rec[f"heatmap{tag}"], rec[f"node_embed{tag}"], rec[f"logZ{tag}"] = heat.detach(), embed.detach(), logz.detach()
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
    import json
    import os

    from tests.helpers import REFERENCE_RECORDS, reference_record

    name = f"gfacs_{case}"
    if os.environ.get("RL4CO_RECORD_REFERENCE") == "1":
        parts = T._parts(reference_run(case))
        for old in REFERENCE_RECORDS.glob(f"{name}_part*.npz"):
            old.unlink()
        for i, part in enumerate(parts):
            reference_record(name if i == 0 else f"{name}_part{i}", lambda part=part: part)
        (REFERENCE_RECORDS / "gfacs_state_dict_keys.json").write_text(json.dumps(reference_keys(), indent=0) + "\n")
    rec = {}
    for path in [REFERENCE_RECORDS / f"{name}.npz"] + sorted(REFERENCE_RECORDS.glob(f"{name}_part*.npz")):
        with np.load(path) as z:
            rec.update({k: torch.from_numpy(z[k].copy()) for k in z.files})
    return rec


def recorded_keys():
    import json

    from tests.helpers import REFERENCE_RECORDS

    return json.loads((REFERENCE_RECORDS / "gfacs_state_dict_keys.json").read_text())


def record_pairs(rec):
    """name -> (ref32, ref64) for every recorded result (logZ, heatmap, node_embed, grad/<key>, buf/<key>)."""
    pairs = T.record_pairs(rec)
    pairs["logZ"] = (rec["logZ32"], rec["logZ64"])
    return pairs


def record_graph(case, rec):
    """(env, locs, feats or None, neighbors int64) of a record."""
    env, n = CASES[case][:2]
    if env == "tsp":
        return env, rec["locs"], None, R.edge_index_to_neighbors(rec["edge_index"], BATCH, n)
    return env, rec["locs"], rec["feats"], RD.edge_index_to_neighbors(rec["edge_index"], BATCH, n)


if __name__ == "__main__":  # RL4CO_RECORD_REFERENCE=1 python -m tests.gfacs_ref
    for name in CASES:
        r = record(name)
        print(name, len(r), "arrays; data seed", int(r["data_seed"]), "logZ floor",
              float((r["logZ32"].double() - r["logZ64"]).abs().max()))
