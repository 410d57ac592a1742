"""DeepACO's front end: the reference's ``NARGNNEncoder`` (models/zoo/nargnn/encoder.py: TSP init and edge embeddings, the
anisotropic edge-gated GNN of models/nn/graph/gnn.py, the ``EdgeHeatmapGenerator`` MLP) in inference as ONE kernel launch
(``rl4co_nargnn_heatmap``, csrc/nargnn.hip), and the val / test path of ``DeepACOPolicy.forward``
(models/zoo/deepaco/policy.py:122-127, 165-184) on top of it and of :class:`rl4co_amd.aco.AntSystem`: instance -> heatmap ->
ants -> tours, all on the device. ``NARGNNDepotEncoder`` is the same encoder for CVRP, OP and PCTSP, whose graph has a
depot (``CVRPEdgeEmbedding``: every customer's nearest customers plus the depot, the depot to every customer), on
``rl4co_nargnn_depot_heatmap`` (csrc/nargnn_depot.hip).

The modules carry the reference's ``state_dict`` keys (``graph_network.layers.{i}.v_bn.module.*`` is how PyG's
``BatchNorm`` wraps ``BatchNorm1d``), so a reference checkpoint loads with ``load_state_dict(strict=True)``. The neighbour
lists are the reference's own selection (distance matrix, ``+inf`` on the diagonal, ``torch.topk(largest=False,
sorted=False)``) taken for the whole batch on the device; the eval-mode batch norms are folded into a per-channel scale and
shift (in float64, rounded once). Training, CPU tensors, other environments, activations, aggregations and widths are
refused with ``NotImplementedError``: there is no torch fall-back. ``TrainableNARGNNEncoder`` is ``NARGNNEncoder`` that also
trains (TSP): in ``.train()`` the GNN stack runs on batch statistics, forward and backward, on csrc/nargnn_train.hip;
``TrainableNARGNNDepotEncoder`` is the same for ``NARGNNDepotEncoder`` (CVRP, OP, PCTSP) on that file's depot-graph kernels.
``GFACSEncoder`` / ``GFACSDepotEncoder`` add GFACS's log-partition head (models/zoo/gfacs/encoder.py) on csrc/nargnn_logz.hip,
``GFACSPolicy`` is the reference's policy over them (models/zoo/gfacs/policy.py). ``NARGNNPolicy`` (models/zoo/nargnn/policy.py)
is the family's base model: the trainable encoder and :func:`rl4co_amd.aco.heatmap_decode`, with greedy and top-k / top-p
decoding for ``phase="val"`` / ``"test"``."""
from __future__ import annotations

from functools import partial

import torch
from torch import Tensor, nn

from . import kernels as K
from .aco import AntSystem, heatmap_decode, heatmap_rollout

SMALL_VALUE = 1e-12  # encoder.py:81-82: the fp32 heatmap's guard against log(0)


class _TSPInitEmbedding(nn.Module):
    """env_embeddings/init.py:55-68"""

    def __init__(self, embed_dim: int, linear_bias: bool = True):
        super().__init__()
        self.init_embed = nn.Linear(2, embed_dim, linear_bias)


class _TSPEdgeEmbedding(nn.Module):
    """env_embeddings/edge.py:53-116 (sparsify=True): the parameters and the rule for k."""

    def __init__(self, embed_dim: int, linear_bias: bool = True, k_sparse: int | None = None):
        super().__init__()
        self.k_sparse = k_sparse
        self.edge_embed = nn.Linear(1, embed_dim, linear_bias)

    def num_neighbors(self, n: int) -> int:
        k = max(n // 5, 10) if self.k_sparse is None else int(self.k_sparse)
        return min(k, n - 1)  # ops.py:183


class _BatchNorm(nn.Module):
    """torch_geometric.nn.BatchNorm: a ``BatchNorm1d`` under the attribute ``module``."""

    def __init__(self, units: int):
        super().__init__()
        self.module = nn.BatchNorm1d(units)


class _GNNLayer(nn.Module):
    """gnn.py:14-43"""

    def __init__(self, units: int):
        super().__init__()
        self.v_lin1 = nn.Linear(units, units)
        self.v_lin2 = nn.Linear(units, units)
        self.v_lin3 = nn.Linear(units, units)
        self.v_lin4 = nn.Linear(units, units)
        self.v_bn = _BatchNorm(units)
        self.e_lin = nn.Linear(units, units)
        self.e_bn = _BatchNorm(units)


class _GNNEncoder(nn.Module):
    """gnn.py:64-82"""

    def __init__(self, num_layers: int, embed_dim: int):
        super().__init__()
        self.layers = nn.ModuleList([_GNNLayer(embed_dim) for _ in range(num_layers)])


class _EdgeHeatmapGenerator(nn.Module):
    """encoder.py:20-48"""

    def __init__(self, embed_dim: int, num_layers: int, linear_bias: bool = True):
        super().__init__()
        self.linears = nn.ModuleList([nn.Linear(embed_dim, embed_dim, bias=linear_bias) for _ in range(num_layers - 1)])
        self.output = nn.Linear(embed_dim, 1, bias=linear_bias)


def _fold_batch_norm(bn: nn.BatchNorm1d) -> Tensor:
    """Eval-mode batch norm as (scale, shift) [2, D]: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean
    * scale, in float64 and rounded once."""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    shift = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
    return torch.stack((scale, shift), 0).float()


class NARGNNEncoder(nn.Module):
    """encoder.py:96-193 for TSP in inference: ``forward(td)`` returns ``(heatmap_logits [B, N, N], node_embed [B, N, D])``."""

    ENVS: tuple = ("tsp",)  # what the class's kernel serves
    KERNEL = "rl4co_nargnn_heatmap"

    def __init__(self, embed_dim: int = 64, env_name: str = "tsp", init_embedding: nn.Module | None = None,
                 edge_embedding: nn.Module | None = None, graph_network: nn.Module | None = None,
                 heatmap_generator: nn.Module | None = None, num_layers_heatmap_generator: int = 5,
                 num_layers_graph_encoder: int = 15, act_fn="silu", agg_fn="mean", linear_bias: bool = True,
                 k_sparse: int | None = None):
        super().__init__()
        self.env_name = env_name
        self.embed_dim = embed_dim
        self.act_fn, self.agg_fn = act_fn, agg_fn
        given = dict(init_embedding=init_embedding, edge_embedding=edge_embedding, graph_network=graph_network,
                     heatmap_generator=heatmap_generator)
        self.custom = [name for name, module in given.items() if module is not None]
        self.init_embedding = self._own_init_embedding(embed_dim) if init_embedding is None else init_embedding
        self.edge_embedding = _TSPEdgeEmbedding(embed_dim, k_sparse=k_sparse) if edge_embedding is None else edge_embedding
        self.graph_network = (_GNNEncoder(num_layers_graph_encoder, embed_dim) if graph_network is None else graph_network)
        self.heatmap_generator = (_EdgeHeatmapGenerator(embed_dim, num_layers_heatmap_generator, linear_bias)
                                  if heatmap_generator is None else heatmap_generator)
        self._packed: tuple | None = None  # (key, tensors): the kernel's view of the parameters, rebuilt when one changes

    def _own_init_embedding(self, embed_dim: int) -> nn.Module:
        return _TSPInitEmbedding(embed_dim)

    def _extra_parameters(self, f32) -> dict:
        """What a subclass's kernel reads beyond ``rl4co_nargnn_args``' parameters."""
        return {}

    # ---- what the kernel serves -------------------------------------------------------------------------------------------
    def _check(self, locs: Tensor) -> None:
        me = type(self).__name__
        if self.training:
            raise NotImplementedError(f"{me} serves inference only: a training-mode batch norm needs the statistics "
                                      "of the whole batch (call .eval())")
        if self.custom:
            raise NotImplementedError(f"{me} serves its own sub-modules only, got a custom {', '.join(self.custom)}")
        if self.env_name not in self.ENVS:
            raise NotImplementedError(f"{me} serves the {' / '.join(self.ENVS)} environment only (NARGNNEncoder: the regular "
                                      f"k-nearest graph; NARGNNDepotEncoder: the depot graphs of cvrp, op and pctsp), got "
                                      f"{self.env_name!r}")
        if self.act_fn != "silu":
            raise NotImplementedError(f"{me} serves act_fn='silu' only, got {self.act_fn!r}")
        if self.agg_fn != "mean":
            raise NotImplementedError(f"{me} serves agg_fn='mean' only, got {self.agg_fn!r}")
        if self.embed_dim != 64:
            raise NotImplementedError(f"{me} serves embed_dim=64 only, got {self.embed_dim}")
        if not locs.is_cuda:
            raise NotImplementedError(f"{me} runs inside the MI355X kernel ({self.KERNEL}) only: td['locs'] "
                                      f"on {locs.device}")

    def packed_parameters(self, device) -> dict:
        """The parameters as the kernel reads them (stacked per layer, batch norms folded), cached until one changes."""
        tensors = list(self.parameters()) + list(self.buffers())
        key = (str(device),) + tuple((t.data_ptr(), t._version) for t in tensors)
        if self._packed is not None and self._packed[0] == key:
            return self._packed[1]

        def f32(t):
            return None if t is None else t.detach().to(device=device, dtype=torch.float32).contiguous()

        layers = list(self.graph_network.layers)
        gen = self.heatmap_generator
        p = dict(init_w=f32(self.init_embedding.init_embed.weight), init_b=f32(self.init_embedding.init_embed.bias),
                 edge_w=f32(self.edge_embedding.edge_embed.weight), edge_b=f32(self.edge_embedding.edge_embed.bias),
                 lin_w=None, lin_b=None, bn=None, mlp_w=None, mlp_b=None, out_w=f32(gen.output.weight), out_b=f32(gen.output.bias))
        if layers:
            lins = [[getattr(layer, n) for n in ("v_lin1", "v_lin2", "v_lin3", "v_lin4", "e_lin")] for layer in layers]
            p["lin_w"] = f32(torch.stack([torch.stack([m.weight for m in row], 0) for row in lins], 0))
            p["lin_b"] = f32(torch.stack([torch.stack([m.bias for m in row], 0) for row in lins], 0))
            p["bn"] = f32(torch.stack([torch.stack((_fold_batch_norm(layer.v_bn.module), _fold_batch_norm(layer.e_bn.module)), 0)
                                       for layer in layers], 0))
        if len(gen.linears):
            p["mlp_w"] = f32(torch.stack([m.weight for m in gen.linears], 0))
            if gen.linears[0].bias is not None:
                p["mlp_b"] = f32(torch.stack([m.bias for m in gen.linears], 0))
        p.update(self._extra_parameters(f32))
        self._packed = (key, p)
        return p

    def neighbors(self, locs: Tensor) -> tuple[Tensor, Tensor]:
        """edge.py:88-104 and ops.py:169-199 for the whole batch: (neighbors [B, N, K] int32, edge_cost [B, N, K])."""
        n = locs.shape[1]
        cost = (locs[..., :, None, :] - locs[..., None, :, :]).norm(p=2, dim=-1)
        cost.diagonal(dim1=1, dim2=2).fill_(torch.inf)
        values, indices = torch.topk(cost, k=self.edge_embedding.num_neighbors(n), dim=-1, largest=False, sorted=False)
        return indices.to(torch.int32).contiguous(), values.contiguous()

    @torch.no_grad()
    def forward(self, td):
        locs = td["locs"]
        self._check(locs)
        locs = locs.detach().to(torch.float32).contiguous()
        neighbors, cost = self.neighbors(locs)
        return K.nargnn_heatmap(locs, neighbors, cost, small_value=SMALL_VALUE, **self.packed_parameters(locs.device))


class _GNNStackTrain(torch.autograd.Function):
    """The whole L-layer GNN stack on batch statistics as ONE autograd node over the forward and backward entry points of
    csrc/nargnn_train.hip for ``graph`` (``"regular"``: ``rl4co_nargnn_train_*``, ``"depot"``:
    ``rl4co_nargnn_depot_train_*``). ``stats`` [L, 6, 64] comes out beside the two states for the running statistics and
    carries no gradient."""

    KERNELS = {"regular": ("nargnn_train_forward", "nargnn_train_backward"),
               "depot": ("nargnn_depot_train_forward", "nargnn_depot_train_backward")}

    @staticmethod
    def forward(ctx, x_in, w_in, lin_w, lin_b, bn_w, bn_b, neighbors, csr_ptr, csr_src, eps, graph="regular"):
        tensors = [t.detach().contiguous() for t in (x_in, w_in, lin_w, lin_b, bn_w, bn_b)]
        keys = dict(lin_w=tensors[2], lin_b=tensors[3], bn_w=tensors[4], bn_b=tensors[5], eps=eps)
        run = getattr(K, _GNNStackTrain.KERNELS[graph][0])
        x_out, w_out, stats, workspace = run(neighbors, csr_ptr, csr_src, tensors[0], tensors[1], **keys)
        ctx.save_for_backward(*tensors, neighbors, csr_ptr, csr_src, stats, workspace)
        ctx.eps, ctx.graph = eps, graph
        ctx.mark_non_differentiable(stats)
        return x_out, w_out, stats

    @staticmethod
    def backward(ctx, grad_x, grad_w, _grad_stats):
        x_in, w_in, lin_w, lin_b, bn_w, bn_b, neighbors, csr_ptr, csr_src, stats, workspace = ctx.saved_tensors
        run = getattr(K, _GNNStackTrain.KERNELS[ctx.graph][1])
        g = run(neighbors, csr_ptr, csr_src, x_in, w_in, lin_w=lin_w, lin_b=lin_b, bn_w=bn_w, bn_b=bn_b, stats=stats,
                workspace=workspace, grad_x_out=grad_x.contiguous(), grad_w_out=grad_w.contiguous(), eps=ctx.eps)
        return g["x_in"], g["w_in"], g["lin_w"], g["lin_b"], g["bn_w"], g["bn_b"], None, None, None, None, None


class _TrainsOnKernels:
    """What the trainable encoders share, mixed in ahead of the inference class: the train-mode refusals, the stacking of
    the per-layer parameters, the one-eps / one-momentum rule, the call of the stack, the running statistics' update and
    the heatmap MLP. A subclass names its graph and its smallest instance and supplies ``forward`` and ``encode_train``."""

    GRAPH = "regular"                          # _GNNStackTrain.KERNELS' key
    TRAIN_KERNEL = "rl4co_nargnn_train_forward"
    MIN_NODES = 2

    def _train_refusals(self, locs: Tensor) -> tuple:
        me = type(self).__name__
        return (
            (bool(self.custom), f"{me} serves its own sub-modules only, got a custom {', '.join(self.custom)}"),
            (self.env_name not in self.ENVS, f"{me} serves the {' / '.join(self.ENVS)} environment only, got {self.env_name!r}"),
            (self.act_fn != "silu", f"{me} serves act_fn='silu' only, got {self.act_fn!r}"),
            (self.agg_fn != "mean", f"{me} serves agg_fn='mean' only, got {self.agg_fn!r}"),
            (self.embed_dim != 64, f"{me} serves embed_dim=64 only, got {self.embed_dim}"),
            (not locs.is_cuda, f"{me} runs inside the MI355X kernels ({self.TRAIN_KERNEL}) only: td['locs'] on "
                               f"{locs.device}"),
        )

    def _check(self, locs: Tensor, *others: Tensor) -> None:
        if not self.training:
            return super()._check(locs)
        me = type(self).__name__
        for refused, why in self._train_refusals(locs):
            if refused:
                raise NotImplementedError(why)
        dtypes = {p.dtype for p in self.parameters()} | {locs.dtype} | {t.dtype for t in others}
        if dtypes != {torch.float32}:
            raise NotImplementedError(f"{me} trains in fp32 only, got {sorted(str(d) for d in dtypes)}")
        least = self.MIN_NODES
        if locs.dim() != 3 or locs.shape[0] * locs.shape[1] < 2 or locs.shape[1] < least:
            raise NotImplementedError(f"{me} needs B N >= 2 rows for a batch statistic and N >= {least} nodes for an edge, got "
                                      f"td['locs'] {tuple(locs.shape)}")

    def _stack_train(self, x: Tensor, w: Tensor, neighbors: Tensor, csr: tuple) -> tuple[Tensor, Tensor]:
        """The GNN layers over the activated embeddings ``x`` [B, N, 64] and ``w`` (the graph's edge rows), on the kernels;
        updates every batch norm's running statistics once. Without layers the stack is the identity."""
        layers = list(self.graph_network.layers)
        if not layers:
            return x, w
        bns = [bn.module for layer in layers for bn in (layer.v_bn, layer.e_bn)]
        eps, momentum = bns[0].eps, bns[0].momentum
        if momentum is None or any(bn.eps != eps or bn.momentum != momentum for bn in bns):
            raise NotImplementedError(f"{type(self).__name__} serves one eps and one momentum for all batch norms")
        lins = [[getattr(layer, n) for n in ("v_lin1", "v_lin2", "v_lin3", "v_lin4", "e_lin")] for layer in layers]
        lin_w = torch.stack([torch.stack([m.weight for m in row], 0) for row in lins], 0)
        lin_b = torch.stack([torch.stack([m.bias for m in row], 0) for row in lins], 0)
        bn_w = torch.stack([bn.weight for bn in bns], 0).view(len(layers), 2, -1)
        bn_b = torch.stack([bn.bias for bn in bns], 0).view(len(layers), 2, -1)
        x, w, stats = _GNNStackTrain.apply(x, w, lin_w, lin_b, bn_w, bn_b, neighbors, *csr, eps, self.GRAPH)
        self._update_running_statistics(bns, stats, x.shape[0] * x.shape[1], 0, momentum, edge_rows=w.numel() // w.shape[-1])
        return x, w

    def _edge_probabilities(self, w: Tensor) -> Tensor:
        """The heatmap MLP over the edge rows: ``w`` [..., 64] -> probabilities [...] in float64."""
        gen = self.heatmap_generator
        h = w
        for linear in gen.linears:
            h = nn.functional.silu(linear(h))
        # the tail behind the last product runs in float64 -- the bias, the sigmoid and, in the caller, the scatter and the
        # log, a few numbers per edge row: the logits are rounded to fp32 once, and on the way back the output bias's
        # gradient, ONE number that sums every edge row of the batch with terms that nearly cancel, is summed in float64
        out = nn.functional.linear(h, gen.output.weight).double()
        if gen.output.bias is not None:
            out = out + gen.output.bias.double()
        return torch.sigmoid(out)[..., 0]

    @staticmethod
    @torch.no_grad()
    def _update_running_statistics(bns: list, stats: Tensor, node_rows: int, k: int, momentum: float,
                                   edge_rows: int | None = None) -> None:
        """``BatchNorm1d``'s own update from the batch's mean and BIASED variance: ``stats`` [L, 6, D] = (mu_v, r_v, var_v, mu_e,
        r_e, var_e) per layer; the running variance takes the unbiased one, var n / (n - 1), n the rows of its side:
        ``node_rows`` and ``edge_rows`` (``node_rows * k`` when not given)."""
        flat = stats.view(-1, 3, stats.shape[-1])  # [2 L]: v_bn, e_bn per layer
        rows = [node_rows, node_rows * k if edge_rows is None else edge_rows]
        unbiased = flat[:, 2] * torch.tensor([rows[i % 2] / (rows[i % 2] - 1) for i in range(len(bns))],
                                             dtype=stats.dtype, device=stats.device)[:, None]
        tracked = [i for i, bn in enumerate(bns) if bn.track_running_stats and bn.running_mean is not None]
        means, variances = [bns[i].running_mean for i in tracked], [bns[i].running_var for i in tracked]
        torch._foreach_mul_(means, 1.0 - momentum)
        torch._foreach_add_(means, [flat[i, 0] for i in tracked], alpha=momentum)
        torch._foreach_mul_(variances, 1.0 - momentum)
        torch._foreach_add_(variances, [unbiased[i] for i in tracked], alpha=momentum)
        torch._foreach_add_([bns[i].num_batches_tracked for i in tracked], 1)


class TrainableNARGNNEncoder(_TrainsOnKernels, NARGNNEncoder):
    """``NARGNNEncoder`` that also trains, for TSP: the same constructor and ``state_dict`` keys. In ``.eval()`` it IS the
    parent (one launch of ``rl4co_nargnn_heatmap``, no gradient). In ``.train()`` ``forward(td)`` returns ``(heatmap_logits
    [B, N, N], node_embed [B, N, 64])`` attached to autograd, the batch norms on BATCH statistics as the reference's train
    mode, and updates ``running_mean``, ``running_var`` and ``num_batches_tracked`` of all 2 L batch norms once. The L-layer
    GNN stack, forward and backward, runs on the kernels of csrc/nargnn_train.hip behind one autograd node; the neighbour
    selection, the incoming-edge CSR, the two embeddings and the heatmap MLP are torch."""

    def forward(self, td):
        if not self.training:
            return super().forward(td)
        locs = td["locs"]
        self._check(locs)
        locs = locs.detach().contiguous()
        with torch.no_grad():
            neighbors, cost = self.neighbors(locs)
        return self.encode_train(locs, neighbors, cost)

    def encode_train(self, locs: Tensor, neighbors: Tensor, cost: Tensor):
        """Train mode on a given graph: ``neighbors`` [B, N, K] int32 and the edges' ``cost`` [B, N, K]."""
        return self._encode_train(locs, neighbors, cost)[:2]

    def _encode_train(self, locs: Tensor, neighbors: Tensor, cost: Tensor):
        """``encode_train`` and, third, the stack's edge state ``w`` [B, N, K, 64] (what a further head reads)."""
        node_embed = self.init_embedding.init_embed(locs)
        x = nn.functional.silu(node_embed)
        w = nn.functional.silu(self.edge_embedding.edge_embed(cost[..., None]))
        if len(self.graph_network.layers):
            x, w = self._stack_train(x, w, neighbors, K.incoming_csr(neighbors))
        prob = self._edge_probabilities(w)  # [B, N, K]
        heat = torch.zeros(locs.shape[0], locs.shape[1], locs.shape[1], dtype=prob.dtype, device=prob.device)
        heat = heat.scatter(2, neighbors.to(torch.int64), prob)
        return torch.log(heat + SMALL_VALUE).float(), node_embed, w


class _DepotInitEmbedding(nn.Module):
    """env_embeddings/init.py: VRPInitEmbedding (115-136), PCTSPInitEmbedding (221-251), OPInitEmbedding (254-280): one
    linear over (x, y, features) for the customers, one over (x, y) for the depot."""

    def __init__(self, embed_dim: int, node_dim: int, linear_bias: bool = True):
        super().__init__()
        self.init_embed = nn.Linear(node_dim, embed_dim, linear_bias)
        self.init_embed_depot = nn.Linear(2, embed_dim, linear_bias)


def _depot_features(env_name: str, td) -> Tensor:
    """The customers' features behind their coordinates, [B, N - 1, F], in the reference's order."""
    if env_name == "cvrp":
        return td["demand"][..., None]
    if env_name == "op":
        return td["prize"][..., 1:, None]
    return torch.stack((td["expected_prize"], td["penalty"][..., 1:]), -1)


DEPOT_ENVS = {"cvrp": 1, "op": 1, "pctsp": 2}  # environment -> F, the customer features behind the coordinates


class NARGNNDepotEncoder(NARGNNEncoder):
    """encoder.py:96-193 for CVRP, OP and PCTSP in inference, on ``rl4co_nargnn_depot_heatmap``: the graph of
    ``CVRPEdgeEmbedding`` (every customer's nearest customers plus the depot, the depot to every customer)."""

    ENVS = tuple(DEPOT_ENVS)
    KERNEL = "rl4co_nargnn_depot_heatmap"

    def __init__(self, embed_dim: int = 64, env_name: str = "cvrp", **kwargs):
        super().__init__(embed_dim=embed_dim, env_name=env_name, **kwargs)

    def _own_init_embedding(self, embed_dim: int) -> nn.Module:
        return _DepotInitEmbedding(embed_dim, 2 + DEPOT_ENVS.get(self.env_name, 1))

    def _extra_parameters(self, f32) -> dict:
        depot = self.init_embedding.init_embed_depot
        return dict(depot_w=f32(depot.weight), depot_b=f32(depot.bias))

    def neighbors(self, locs: Tensor) -> tuple[Tensor, Tensor, Tensor]:
        """edge.py:125-163 for the whole batch: (neighbors [B, C, K] int32 with values in 1 .. N - 1, edge_cost [B, C, K],
        depot_cost [B, C]). The selection runs on the customer block of the distance matrix; k comes from N with the depot."""
        n = locs.shape[1]
        cost = (locs[..., :, None, :] - locs[..., None, :, :]).norm(p=2, dim=-1)
        depot_cost = cost[:, 1:, 0].contiguous()
        block = cost[:, 1:, 1:].clone()
        block.diagonal(dim1=1, dim2=2).fill_(torch.inf)
        k = max(n // 5, 10) if self.edge_embedding.k_sparse is None else int(self.edge_embedding.k_sparse)
        values, indices = torch.topk(block, k=min(k, n - 2), dim=-1, largest=False, sorted=False)
        return (indices + 1).to(torch.int32).contiguous(), values.contiguous(), depot_cost

    @torch.no_grad()
    def forward(self, td):
        locs = td["locs"]
        self._check(locs)
        locs = locs.detach().to(torch.float32).contiguous()
        feats = _depot_features(self.env_name, td).detach().to(torch.float32).contiguous()
        neighbors, cost, depot_cost = self.neighbors(locs)
        return K.nargnn_depot_heatmap(locs, feats, neighbors, cost, depot_cost, small_value=SMALL_VALUE,
                                      **self.packed_parameters(locs.device))


class TrainableNARGNNDepotEncoder(_TrainsOnKernels, NARGNNDepotEncoder):
    """``NARGNNDepotEncoder`` that also trains, for CVRP, OP and PCTSP: the same constructor and ``state_dict`` keys. In
    ``.eval()`` it IS the parent (one launch of ``rl4co_nargnn_depot_heatmap``, no gradient). In ``.train()``
    ``forward(td)`` returns ``(heatmap_logits [B, N, N], node_embed [B, N, 64])`` attached to autograd, the batch norms on
    BATCH statistics, and updates the running statistics of all 2 L batch norms once (the unbiased factor from B N node
    rows and B (N - 1)(K + 2) edge rows). The GNN stack runs on csrc/nargnn_train.hip's depot-graph kernels behind one
    autograd node; the neighbour selection, the CSR, the embeddings, the heatmap MLP and the scatter are torch."""

    GRAPH = "depot"
    TRAIN_KERNEL = "rl4co_nargnn_depot_train_forward"
    MIN_NODES = 3  # the depot and two customers: a customer needs a customer neighbour

    def forward(self, td):
        if not self.training:
            return super().forward(td)
        locs = td["locs"]
        self._check(locs)  # (before the features are read: spctsp has other keys)
        feats = _depot_features(self.env_name, td).detach().contiguous()
        self._check(locs, feats)
        locs = locs.detach().contiguous()
        with torch.no_grad():
            neighbors, cost, depot_cost = self.neighbors(locs)
        return self.encode_train(locs, feats, neighbors, cost, depot_cost)

    def encode_train(self, locs: Tensor, feats: Tensor, neighbors: Tensor, cost: Tensor, depot_cost: Tensor):
        """Train mode on a given graph: ``neighbors`` [B, N - 1, K] int32 (values in 1 .. N - 1), the kNN edges' ``cost``
        [B, N - 1, K] and ``depot_cost`` [B, N - 1]. The edge rows are in the reference's order: the kNN rows by source,
        every ``i -> 0``, every ``0 -> i``."""
        return self._encode_train(locs, feats, neighbors, cost, depot_cost)[:2]

    def _encode_train(self, locs: Tensor, feats: Tensor, neighbors: Tensor, cost: Tensor, depot_cost: Tensor):
        """``encode_train`` and, third, the stack's edge state ``w`` [B, E, 64] (what a further head reads)."""
        b, n, _ = locs.shape
        c, k = n - 1, neighbors.shape[2]
        init = self.init_embedding
        node_embed = torch.cat((init.init_embed_depot(locs[:, :1]), init.init_embed(torch.cat((locs[:, 1:], feats), -1))), 1)
        x = nn.functional.silu(node_embed)
        row_cost = torch.cat((cost.reshape(b, c * k), depot_cost, depot_cost), 1)  # [B, E]
        w = nn.functional.silu(self.edge_embedding.edge_embed(row_cost[..., None]))
        if len(self.graph_network.layers):
            x, w = self._stack_train(x, w, neighbors, K.depot_incoming_csr(neighbors))
        prob = self._edge_probabilities(w)  # [B, E]
        cust = torch.arange(1, n, device=locs.device).expand(b, c)
        zero = torch.zeros_like(cust)
        src = torch.cat((cust[:, :, None].expand(b, c, k).reshape(b, c * k), cust, zero), 1)
        dst = torch.cat((neighbors.to(torch.int64).reshape(b, c * k), zero, cust), 1)
        heat = torch.zeros(b, n, n, dtype=prob.dtype, device=prob.device)
        heat = heat.index_put((torch.arange(b, device=locs.device)[:, None], src, dst), prob)
        return torch.log(heat + SMALL_VALUE).float(), node_embed, w


class _LogZHead(torch.autograd.Function):
    """GFACS's log-partition head (gfacs/encoder.py:45-47, 62) as ONE autograd node over csrc/nargnn_logz.hip: ``w`` [..., 64]
    the stack's edge state (``batch`` instances, batch-major), the two linears of ``Z_net`` -> ``logZ`` [B, Z]. The hidden is
    never stored: the backward recomputes it. There is no double backward."""

    @staticmethod
    def forward(ctx, w, W1, b1, W2, b2, batch, pooling):
        tensors = [t.detach().contiguous() for t in (w, W1, b1, W2, b2)]
        ctx.save_for_backward(*tensors)
        ctx.batch, ctx.pooling = batch, pooling
        return K.nargnn_logz_forward(*tensors, batch=batch, pooling=pooling)

    @staticmethod
    def backward(ctx, grad_logz):
        if torch.is_grad_enabled():
            raise RuntimeError("the logZ head has no double backward: rl4co_nargnn_logz_backward is not differentiable "
                               "(create_graph=True is not served)")
        g = K.nargnn_logz_backward(*ctx.saved_tensors, grad_logz.to(torch.float32).contiguous(), batch=ctx.batch,
                                   pooling=ctx.pooling)
        return g["w"], g["W1"], g["b1"], g["W2"], g["b2"], None, None


class _EstimatesLogZ:
    """What the two GFACS encoders add to their trainable parents, mixed in ahead of them: ``Z_net`` under the reference's
    keys (``Z_net.0.*``, ``Z_net.2.*``), ``z_out_dim``, the pooling rule, and the third output."""

    def _add_z_net(self, embed_dim: int, z_out_dim: int, pooling: str) -> None:
        if z_out_dim not in (1, 2):
            raise NotImplementedError(f"{type(self).__name__} serves z_out_dim 1 or 2 (logZ, and ls_logZ when training with "
                                      f"local search), got {z_out_dim}")
        if pooling not in K.LOGZ_POOLING:
            raise ValueError(f"pooling must be one of {sorted(K.LOGZ_POOLING)}, got {pooling!r}")
        self.Z_net = nn.Sequential(nn.Linear(embed_dim, embed_dim), nn.SiLU(), nn.Linear(embed_dim, z_out_dim))
        self.z_out_dim, self.pooling = z_out_dim, pooling

    def forward(self, td):
        """``.train()``: ``(heatmap_logits [B, N, N], node_embed [B, N, 64], logZ [B, z_out_dim])``, all attached to autograd.
        ``.eval()``: ``(heatmap_logits, node_embed, None)`` -- the fused inference kernel keeps the edge state on chip and
        the reference's val / test path never reads ``logZ``."""
        if not self.training:
            return (*super().forward(td), None)
        return super().forward(td)  # (the parent's graph selection, then encode_train below)

    def encode_train(self, *graph):
        """The parent's ``encode_train`` and ``logZ`` [B, z_out_dim] from the kernel head on the stack's output ``w`` (without
        GNN layers: on the activated edge embedding). The heatmap MLP and the head both read ``w``; autograd adds the two
        gradients."""
        heat, node_embed, w = self._encode_train(*graph)
        first, last = self.Z_net[0], self.Z_net[2]
        logz = _LogZHead.apply(w, first.weight, first.bias, last.weight, last.bias, heat.shape[0], self.pooling)
        return heat, node_embed, logz


class GFACSEncoder(_EstimatesLogZ, TrainableNARGNNEncoder):
    """gfacs/encoder.py:8-68 for TSP: ``TrainableNARGNNEncoder`` plus the log-partition head ``Z_net`` (``Linear(64, 64)``,
    ``SiLU``, ``Linear(64, z_out_dim)``) for the trajectory-balance loss; a reference GFACS ``state_dict`` loads with
    ``strict=True``. ``pooling="reference"`` (the default, what the reference's checkpoints were trained with) is
    encoder.py:62 as written: ``logZ[b]`` is the mean over the flat edge rows r with ``r % B == b``; ``pooling="instance"``
    is the mean over instance b's own rows. See ``forward``."""

    def __init__(self, embed_dim: int = 64, env_name: str = "tsp", z_out_dim: int = 1, pooling: str = "reference", **kwargs):
        super().__init__(embed_dim=embed_dim, env_name=env_name, **kwargs)
        self._add_z_net(embed_dim, z_out_dim, pooling)


class GFACSDepotEncoder(_EstimatesLogZ, TrainableNARGNNDepotEncoder):
    """:class:`GFACSEncoder` for CVRP, OP and PCTSP: ``TrainableNARGNNDepotEncoder`` plus ``Z_net`` over the depot graph's
    B (N - 1)(K + 2) edge rows."""

    def __init__(self, embed_dim: int = 64, env_name: str = "cvrp", z_out_dim: int = 1, pooling: str = "reference", **kwargs):
        super().__init__(embed_dim=embed_dim, env_name=env_name, **kwargs)
        self._add_z_net(embed_dim, z_out_dim, pooling)


def _merge_with_defaults(value, **defaults) -> dict:
    """utils/utils.py merge_with_defaults: an int for every phase, a dict over the defaults, None for the defaults."""
    if value is None:
        return dict(defaults)
    if isinstance(value, dict):
        return {**defaults, **value}
    return {key: value for key in defaults}


class DeepACOPolicy(nn.Module):
    """policy.py:22-184. The val / test path: encoder, ``heatmap / temperature``, ``AntSystem.run``. ``phase="train"`` (the
    constructive training path, TSP) is served when the caller supplied ``encoder=``, a differentiable module returning
    ``(heatmap [B, N, N], anything)``: the ants' rollout and its backward are one launch each
    (:func:`rl4co_amd.aco.heatmap_rollout`); with the policy's own inference-only kernel encoder it is refused. The
    constructor takes the reference's arguments; ``top_k`` / ``top_p`` above 0 and an explicit ``k_sparse`` on the policy
    (the reference then hands ``top_k`` to the sampler) are refused."""

    def __init__(self, encoder: nn.Module | None = None, env_name: str = "tsp", temperature: float = 1.0, top_p: float = 0.0,
                 top_k: int = 0, aco_class: type | None = None, aco_kwargs: dict = {}, train_with_local_search: bool = False,
                 n_ants: int | dict | None = None, n_iterations: int | dict | None = None, start_node: int | None = None,
                 multistart: bool = False, k_sparse: int | None = None, **encoder_kwargs):
        super().__init__()
        if k_sparse is not None:
            raise NotImplementedError("DeepACOPolicy(k_sparse=...) makes the reference pass top_k to the sampler, which the "
                                      "Ant System kernel does not serve; set k_sparse on the encoder alone")
        if top_k > 0 or top_p > 0:
            raise NotImplementedError(f"top_k / top_p filtering of the heatmap is not served (top_k={top_k}, top_p={top_p})")
        if encoder is None:
            encoder = (NARGNNDepotEncoder if env_name in DEPOT_ENVS else NARGNNEncoder)(env_name=env_name, **encoder_kwargs)
            self._own_encoder = True  # the kernel encoder: inference only, no gradient
        else:
            self._own_encoder = False
        self.encoder = encoder
        self.env_name = env_name
        self.temperature = temperature
        self.top_p, self.top_k = top_p, top_k
        self.decode_type = "multistart_sampling" if env_name == "tsp" or multistart else "sampling"
        self.default_decoding_kwargs: dict = {"select_best": False}
        if "multistart" in self.decode_type:
            self.default_decoding_kwargs.update(
                {"multistart": True, "select_start_nodes_fn": partial(self.select_start_node_fn, start_node=start_node)})
        else:
            self.default_decoding_kwargs.update({"multisample": True})
        self.aco_class = AntSystem if aco_class is None else aco_class
        self.aco_kwargs = aco_kwargs
        self.train_with_local_search = train_with_local_search
        if train_with_local_search:
            assert self.aco_kwargs.get("use_local_search", False)
        self.n_ants = _merge_with_defaults(n_ants, train=30, val=48, test=48)
        self.n_iterations = _merge_with_defaults(n_iterations, train=1, val=5, test=10)
        self.last_aco = None  # the search object of the last forward (its log_heuristic, pheromone, last_iterations)

    @staticmethod
    def select_start_node_fn(td, env, num_starts: int, start_node: int | None = None):
        """policy.py:97-106"""
        mask = td["action_mask"]
        if env.name == "tsp" and start_node is not None:
            return start_node * torch.ones(mask.shape[0] * num_starts, dtype=torch.long, device=mask.device)
        return torch.multinomial(mask.float(), num_starts, replacement=True).view(-1)

    def forward(self, td_initial, env=None, phase: str = "train", return_actions: bool = True, **decoding_kwargs):
        if phase == "train" and not self._own_encoder:
            return self._forward_train(td_initial, env, return_actions, decoding_kwargs)
        if phase not in ("val", "test"):
            why = (": its gradient reaches a caller-supplied differentiable encoder= only, the policy's own kernel encoder "
                   "is inference-only") if phase == "train" else ""
            raise NotImplementedError(f"DeepACOPolicy serves phase='val' and phase='test' (the Ant System search); "
                                      f"phase={phase!r} is the constructive training path{why}")
        n_ants = self.n_ants[phase]
        decoding_kwargs.update(self.default_decoding_kwargs)
        decoding_kwargs.update({"num_starts": n_ants} if "multistart" in self.decode_type else {"num_samples": n_ants})
        if env is None or isinstance(env, str):
            from .envs import get_env

            env = get_env(self.env_name if env is None else env)
        heatmap = self.encoder(td_initial)[0]  # (heatmap, node_embed) or, from a GFACS encoder, (heatmap, node_embed, logZ)
        heatmap /= self.temperature
        aco = self.aco_class(heatmap, n_ants=n_ants, **self.aco_kwargs)
        self.last_aco = aco
        n_iterations = self.n_iterations[phase]
        actions, iter_rewards = aco.run(td_initial, env, n_iterations, decoding_kwargs)
        out = {"reward": iter_rewards[n_iterations - 1]}
        out.update({f"reward_{i:03d}": iter_rewards[i] for i in range(n_iterations)})
        if return_actions:
            out["actions"] = actions
        return out

    def _forward_train(self, td_initial, env, return_actions: bool, decoding_kwargs: dict) -> dict:
        """policy.py:138-163 through ``ConstructivePolicy.forward`` for TSP: ``n_ants['train']`` constructive rollouts per
        instance from the caller's encoder's heatmap in one launch (:func:`rl4co_amd.aco.heatmap_rollout`), the gradient
        back to the heatmap in one more. The heatmap is not divided by the temperature: the temperature goes to the step."""
        if self.env_name != "tsp":
            raise NotImplementedError(f"DeepACOPolicy phase='train' serves env_name='tsp' only (the backward kernel rests on "
                                      f"a TSP tour being a permutation), got env_name={self.env_name!r}")
        if decoding_kwargs.pop("actions", None) is not None:
            raise NotImplementedError("DeepACOPolicy phase='train' does not serve actions= (the reference's 'evaluate' "
                                      "strategy under multistart)")
        if decoding_kwargs.pop("return_entropy", False):
            raise NotImplementedError("DeepACOPolicy phase='train' does not serve return_entropy=True")
        if not decoding_kwargs.pop("return_sum_log_likelihood", True):
            raise NotImplementedError("DeepACOPolicy phase='train' does not serve return_sum_log_likelihood=False")
        return_hidden = decoding_kwargs.pop("return_hidden", True)
        n_ants = self.n_ants["train"]
        decoding_kwargs.setdefault("temperature", self.temperature)
        decoding_kwargs.update(self.default_decoding_kwargs)
        decoding_kwargs.update({"num_starts": n_ants})
        if env is None or isinstance(env, str):
            from .envs import get_env

            env = get_env(self.env_name if env is None else env)
        # the refusals come before the encoder runs: the search's own check on an empty heatmap on the instances' device
        # (every decoding keyword it refuses, then CPU tensors)
        locs = td_initial["locs"]
        self.aco_class(locs.new_empty((locs.shape[0], 0, 0)), n_ants=n_ants, **self.aco_kwargs)._check(td_initial, env, decoding_kwargs)
        heatmap, _ = self.encoder(td_initial)
        aco = self.aco_class(heatmap.detach(), n_ants=n_ants, **self.aco_kwargs)
        temperature = aco._check(td_initial, env, decoding_kwargs)  # (the encoder's output device)
        starts = aco._start_nodes(td_initial, env, decoding_kwargs)  # select_start_nodes_fn, called once
        rolled = heatmap_rollout(heatmap, td_initial["locs"], n_ants=n_ants, start_nodes=starts, temperature=temperature)

        def unbatchify(x):  # [rows] ant-major -> [B, n_ants]
            return x.view(n_ants, -1).t()

        out = {"reward": unbatchify(rolled["reward"]), "log_likelihood": unbatchify(rolled["log_likelihood"])}
        if return_actions:
            out["actions"] = rolled["actions"]
        if return_hidden:
            out["hidden"] = heatmap
        if self.train_with_local_search:
            self.last_aco = aco
            _, ls_reward = aco.local_search(td_initial, env, rolled["actions"], decoding_kwargs)
            out["ls_reward"] = unbatchify(ls_reward)
        return out


class GFACSPolicy(DeepACOPolicy):
    """gfacs/policy.py:22-180 with the reference's constructor. With ``encoder=None`` the policy builds the trainable GFACS
    encoder of ``env_name`` (``z_out_dim = 2 if train_with_local_search else 1``), and unlike ``DeepACOPolicy`` its own
    encoder trains. ``train_with_local_search`` (default True, as in the reference) needs
    ``aco_kwargs["use_local_search"]`` and is refused for cvrp, op and pctsp, where no local search is served.

    ``phase="train"`` (policy.py:107-160): one :func:`rl4co_amd.aco.heatmap_rollout` and ``reward``, ``log_likelihood``
    [B, n_ants] and ``logZ`` [B, 1]; with local search ``aco.local_search`` on the sampled tours (2-opt, or NLS with
    ``use_nls``), a second ``heatmap_rollout(actions=ls_actions)`` and ``ls_logZ`` [B, 1], ``ls_reward``,
    ``ls_log_likelihood`` [B, n_ants] and ``ls_actions``. ``actions`` and ``ls_actions`` stay ant-major rows
    [n_ants * B, W]. tsp runs multistart, cvrp / op / pctsp multisample (cvrp multistart too, with ``multistart=True``).
    The decoding keywords ``DeepACOPolicy``'s train path refuses are refused here too, before the encoder runs.
    ``phase="val"`` / ``"test"``: ``DeepACOPolicy.forward`` itself, which reads the first output of the encoder."""

    def __init__(self, encoder: nn.Module | None = None, env_name: str = "tsp", temperature: float = 1.0, top_p: float = 0.0,
                 top_k: int = 0, aco_class: type | None = None, aco_kwargs: dict = {}, train_with_local_search: bool = True,
                 n_ants: int | dict | None = None, n_iterations: int | dict | None = None, multistart: bool = False,
                 k_sparse: int | None = None, **encoder_kwargs):
        from .aco import _SERVES

        why = _SERVES[env_name].no_local_search if env_name in _SERVES else None
        if train_with_local_search and why:
            raise NotImplementedError(f"GFACSPolicy(train_with_local_search=True) is not served for {env_name}: {why} "
                                      f"(pass train_with_local_search=False)")
        if encoder is None:
            cls = GFACSDepotEncoder if env_name in DEPOT_ENVS else GFACSEncoder
            encoder = cls(env_name=env_name, z_out_dim=2 if train_with_local_search else 1, **encoder_kwargs)
        elif train_with_local_search and getattr(encoder, "z_out_dim", 2) < 2:
            raise ValueError("GFACSPolicy(train_with_local_search=True) reads logZ[:, 1]: the encoder needs z_out_dim=2")
        super().__init__(encoder=encoder, env_name=env_name, temperature=temperature, top_p=top_p, top_k=top_k,
                         aco_class=aco_class, aco_kwargs=aco_kwargs, train_with_local_search=train_with_local_search,
                         n_ants=n_ants, n_iterations=n_iterations, multistart=multistart, k_sparse=k_sparse)

    def forward(self, td_initial, env=None, phase: str = "train", return_actions: bool = True, return_hidden: bool = False,
                actions=None, **decoding_kwargs):
        if phase != "train":  # the parent's Ant System search on the encoder's heatmap; it refuses any other phase
            return super().forward(td_initial, env, phase, return_actions, **decoding_kwargs)
        if env is None or isinstance(env, str):
            from .envs import get_env

            env = get_env(self.env_name if env is None else env)
        return self._train(td_initial, env, self.n_ants["train"], return_actions, return_hidden, actions, decoding_kwargs)

    def _train(self, td_initial, env, n_ants: int, return_actions: bool, return_hidden: bool, actions, decoding_kwargs: dict):
        if actions is not None or decoding_kwargs.pop("actions", None) is not None:
            raise NotImplementedError("GFACSPolicy phase='train' does not serve actions= (the reference's 'evaluate' strategy); "
                                      "rl4co_amd.aco.heatmap_rollout(actions=...) evaluates given rows")
        if decoding_kwargs.pop("return_entropy", False):
            raise NotImplementedError("GFACSPolicy phase='train' does not serve return_entropy=True")
        if not decoding_kwargs.pop("return_sum_log_likelihood", True):
            raise NotImplementedError("GFACSPolicy phase='train' does not serve return_sum_log_likelihood=False")
        multistart = "multistart" in self.decode_type
        decoding_kwargs.setdefault("temperature", self.temperature)
        decoding_kwargs.update(self.default_decoding_kwargs)
        decoding_kwargs.update({"num_starts": n_ants} if multistart else {"num_samples": n_ants})
        # the refusals come before the encoder runs: the search's own check on an empty heatmap on the instances' device
        locs = td_initial["locs"]
        self.aco_class(locs.new_empty((locs.shape[0], 0, 0)), n_ants=n_ants, **self.aco_kwargs)._check(td_initial, env, decoding_kwargs)
        heatmap, _, logz = self.encoder(td_initial)
        aco = self.aco_class(heatmap.detach(), n_ants=n_ants, **self.aco_kwargs)
        temperature = aco._check(td_initial, env, decoding_kwargs)  # (the encoder's output device)
        starts = aco._start_nodes(td_initial, env, decoding_kwargs) if multistart else None  # called once
        graph = {} if self.env_name == "tsp" else {"env_name": self.env_name, "td": td_initial}
        rolled = heatmap_rollout(heatmap, locs, n_ants=n_ants, start_nodes=starts, temperature=temperature, **graph)

        def unbatchify(x):  # [rows] ant-major -> [B, n_ants]
            return x.view(n_ants, -1).t()

        out = {"logZ": logz[:, [0]], "reward": unbatchify(rolled["reward"]),
               "log_likelihood": unbatchify(rolled["log_likelihood"])}
        if return_actions:
            out["actions"] = rolled["actions"]
        if self.train_with_local_search:
            self.last_aco = aco
            ls_actions, ls_reward = aco.local_search(td_initial, env, rolled["actions"], decoding_kwargs)
            searched = heatmap_rollout(heatmap, locs, n_ants=n_ants, actions=ls_actions, temperature=temperature, **graph)
            out.update({"ls_logZ": logz[:, [1]], "ls_reward": unbatchify(ls_reward),
                        "ls_log_likelihood": unbatchify(searched["log_likelihood"])})
            if return_actions:
                out["ls_actions"] = searched["actions"]
        if return_hidden:
            out["hidden"] = heatmap
        return out


_TRAIN_ENVS = ("tsp", "cvrp", "op", "pctsp", "spctsp")


class NonAutoregressivePolicy(nn.Module):
    """models/common/constructive/nonautoregressive/policy.py: the constructive policy over a heatmap, the training
    surface DeepACO's ``phase="train"`` delegates to. ``encoder`` is the caller's differentiable module returning
    ``(heatmap [B, N, N], init_embeds)``; the decode is :func:`rl4co_amd.aco.heatmap_rollout` — one launch forward, one
    backward — instead of the reference's step loop under autograd.

    Served: ``phase="train"`` with sampling; ``tsp`` with multistart (``train_decode_type="multistart_sampling"`` or
    ``multistart=True``, ``num_starts``), ``cvrp`` / ``op`` / ``pctsp`` / ``spctsp`` with multisample (``multisample=True``,
    ``num_samples``), ``cvrp`` with multistart too. Returns ``ConstructivePolicy.forward``'s dict: flat ant-major [rows]
    ``reward`` and ``log_likelihood``, ``actions`` [rows, W] (zero-filled after each row's length) and on request ``hidden``
    (the heatmap) and ``init_embeds``. Everything else is refused with ``NotImplementedError`` BEFORE the encoder runs:
    ``actions=``, ``return_entropy``, ``return_sum_log_likelihood=False``, ``top_k`` / ``top_p`` / ``tanh_clipping``,
    ``mask_logits=False``, ``select_best``, unknown decoding keywords, CPU tensors, and ``phase="val"`` / ``"test"`` (greedy
    decoding of a heatmap: DeepACO's inference is :class:`DeepACOPolicy`'s Ant System search)."""

    def __init__(self, encoder: nn.Module, decoder=None, env_name: str = "tsp", temperature: float = 1.0,
                 tanh_clipping: float = 0, mask_logits: bool = True, train_decode_type: str = "sampling",
                 val_decode_type: str = "greedy", test_decode_type: str = "greedy"):
        super().__init__()
        if encoder is None:
            raise ValueError("NonAutoregressivePolicy takes the caller's differentiable encoder")
        if decoder is not None:
            raise NotImplementedError("NonAutoregressivePolicy(decoder=...) is not served: the decode is the Ant System "
                                      "kernels' (NonAutoregressiveDecoder's heatmap rows)")
        if env_name not in _TRAIN_ENVS:
            raise NotImplementedError(f"NonAutoregressivePolicy serves env_name in {_TRAIN_ENVS}, got {env_name!r}")
        self.encoder = encoder
        self.env_name = env_name
        self.temperature = temperature
        self.tanh_clipping = tanh_clipping
        self.mask_logits = mask_logits
        self.train_decode_type = train_decode_type
        self.val_decode_type = val_decode_type
        self.test_decode_type = test_decode_type

    def forward(self, td, env=None, phase: str = "train", calc_reward: bool = True, return_actions: bool = True,
                return_entropy: bool = False, return_hidden: bool = False, return_init_embeds: bool = False,
                return_sum_log_likelihood: bool = True, actions=None, max_steps=1_000_000, **decoding_kwargs) -> dict:
        name = "NonAutoregressivePolicy"
        if phase != "train":
            raise NotImplementedError(f"{name} serves phase='train' (the constructive training decode); phase={phase!r} is "
                                      f"a greedy decode of the heatmap, which no kernel serves: DeepACO's inference is "
                                      f"DeepACOPolicy's Ant System search (phase='val' / 'test' there)")
        if actions is not None:
            raise NotImplementedError(f"{name} does not serve actions= (the reference's 'evaluate' strategy); "
                                      f"rl4co_amd.aco.heatmap_rollout(actions=...) evaluates given rows")
        if return_entropy:
            raise NotImplementedError(f"{name} does not serve return_entropy=True")
        if not return_sum_log_likelihood:
            raise NotImplementedError(f"{name} does not serve return_sum_log_likelihood=False; "
                                      f"rl4co_amd.aco.heatmap_rollout returns the per-step log-probs")
        kw = dict(decoding_kwargs)
        decode_type = kw.pop("decode_type", None) or self.train_decode_type
        if decode_type not in ("sampling", "multistart_sampling"):
            raise NotImplementedError(f"{name} serves the decode types 'sampling' and 'multistart_sampling', got {decode_type!r}")
        temperature = float(kw.pop("temperature", self.temperature))
        if kw.pop("tanh_clipping", self.tanh_clipping):
            raise NotImplementedError(f"{name} does not serve tanh_clipping")
        if not kw.pop("mask_logits", self.mask_logits):
            raise NotImplementedError(f"{name} does not serve mask_logits=False")
        if kw.pop("top_k", 0) or kw.pop("top_p", 0.0):
            raise NotImplementedError(f"{name} does not serve top_k / top_p filtering of the heatmap")
        if kw.pop("select_best", False):
            raise NotImplementedError(f"{name} does not serve select_best=True: training takes every ant's row")
        kw.pop("store_all_logp", None)
        multistart = bool(kw.pop("multistart", False)) or decode_type == "multistart_sampling"
        multisample = bool(kw.pop("multisample", False))
        num_starts, num_samples = kw.pop("num_starts", None), kw.pop("num_samples", None)
        start_fn = kw.pop("select_start_nodes_fn", None)
        if kw:
            raise NotImplementedError(f"{name} does not serve the decoding keywords {sorted(kw)}")
        if multistart == multisample:
            raise NotImplementedError(f"{name} takes exactly one of multistart (decode type 'multistart_sampling' or "
                                      f"multistart=True) and multisample=True")
        if multistart and self.env_name not in ("tsp", "cvrp"):
            raise NotImplementedError(f"{name} serves multistart for tsp and cvrp; {self.env_name!r} ants start at the depot "
                                      f"(multisample=True, num_samples=...)")
        if multisample and self.env_name == "tsp":
            raise NotImplementedError(f"{name} serves tsp with multistart (num_starts=...): the ants' kernel starts every "
                                      f"tour from a given node")
        n_ants = num_starts if multistart else num_samples
        if n_ants is None or int(n_ants) < 1:
            raise NotImplementedError(f"{name} takes {'num_starts' if multistart else 'num_samples'} >= 1 (the ants per instance)")
        n_ants = int(n_ants)
        for key in ("locs",):
            if not td[key].is_cuda:
                raise NotImplementedError(f"{name} runs inside the MI355X kernels only: td[{key!r}] on {td[key].device}")
        if env is None or isinstance(env, str):
            from .envs import get_env

            env = get_env(self.env_name if env is None else env)

        hidden, init_embeds = self.encoder(td)
        starts = None
        if multistart:  # Sampling.pre_decoder_hook: called once
            starts = start_fn(td, env, n_ants) if start_fn is not None else env.select_start_nodes(td, num_starts=n_ants)
            starts = starts.to(device=hidden.device, dtype=torch.int64).reshape(-1)
        rolled = heatmap_rollout(hidden, td["locs"], n_ants=n_ants, start_nodes=starts, temperature=temperature,
                                 env_name=self.env_name, td=td)
        out = {"reward": rolled["reward"], "log_likelihood": rolled["log_likelihood"]}
        if return_actions:
            out["actions"] = rolled["actions"]
        if return_hidden:
            out["hidden"] = hidden
        if return_init_embeds:
            out["init_embeds"] = init_embeds
        return out


_DECODE_TYPES = ("greedy", "sampling", "multistart_greedy", "multistart_sampling")


class NARGNNPolicy(nn.Module):
    """models/zoo/nargnn/policy.py:15-105 with the reference's constructor: the plain heatmap model. With ``encoder=None``
    it builds :class:`TrainableNARGNNEncoder` (``tsp``) or :class:`TrainableNARGNNDepotEncoder` (``cvrp``, ``op``,
    ``pctsp``), so a reference ``NARGNNPolicy.state_dict()`` loads with ``strict=True``. ``temperature``,
    ``tanh_clipping`` and ``mask_logits`` are ``ConstructivePolicy``'s keywords.

    ``forward`` is ``ConstructivePolicy.forward`` (constructive/base.py:154-263) with the decode loop as ONE launch of
    :func:`rl4co_amd.aco.heatmap_decode` (and one more for the gradient). Served: ``phase`` "train", "val" and "test" with
    the reference's defaults (``multistart_sampling``, then ``multistart_greedy`` twice); ``decode_type`` "greedy",
    "sampling", "multistart_greedy" and "multistart_sampling"; ``multistart`` / ``num_starts`` (tsp and cvrp; None: the
    environment's ``get_num_starts``) with ``select_start_nodes_fn``; ``multisample`` / ``num_samples`` (cvrp, op, pctsp);
    neither on a depot graph: one row per instance from the depot; ``select_best`` (the best row of every instance, picked on
    the device); ``temperature``, ``top_k``, ``top_p``; ``actions=`` (evaluate: ant-major rows [n * B, W], with multistart
    column 0 is the start); ``calc_reward``, ``return_actions``, ``return_hidden``, ``return_init_embeds`` and
    ``return_sum_log_likelihood``. Rows are ant-major (the reference's batchify) and W wide, zero-filled after each row's
    length. Refused by name before the encoder runs (``NotImplementedError``): a multistart decode type on ``op`` / ``pctsp``
    (every ant starts at the depot), ``tsp`` without multistart (the ants' kernel starts a tour from a given node),
    ``tanh_clipping``, ``mask_logits=False``, ``return_entropy``, beam search and other decode types, unknown decoding
    keywords, a ``decoder=`` and CPU tensors."""

    def __init__(self, encoder: nn.Module | None = None, decoder=None, embed_dim: int = 64, env_name: str = "tsp",
                 init_embedding: nn.Module | None = None, edge_embedding: nn.Module | None = None,
                 graph_network: nn.Module | None = None, heatmap_generator: nn.Module | None = None,
                 num_layers_heatmap_generator: int = 5, num_layers_graph_encoder: int = 15, act_fn="silu", agg_fn="mean",
                 linear_bias: bool = True, train_decode_type: str = "multistart_sampling",
                 val_decode_type: str = "multistart_greedy", test_decode_type: str = "multistart_greedy",
                 **constructive_policy_kw):
        super().__init__()
        if decoder is not None:
            raise NotImplementedError("NARGNNPolicy(decoder=...) is not served: the decode is the Ant System kernels' "
                                      "(NonAutoregressiveDecoder's heatmap rows)")
        if env_name not in _TRAIN_ENVS:
            raise NotImplementedError(f"NARGNNPolicy serves env_name in {_TRAIN_ENVS}, got {env_name!r}")
        self.temperature = constructive_policy_kw.pop("temperature", 1.0)
        self.tanh_clipping = constructive_policy_kw.pop("tanh_clipping", 0)
        self.mask_logits = constructive_policy_kw.pop("mask_logits", True)
        if constructive_policy_kw:  # (the reference logs "Unused kwargs" and hands them on)
            raise NotImplementedError(f"NARGNNPolicy does not serve the keywords {sorted(constructive_policy_kw)}")
        if encoder is None:
            if env_name == "spctsp":
                raise NotImplementedError("NARGNNPolicy builds no encoder for spctsp: pass encoder=")
            cls = TrainableNARGNNDepotEncoder if env_name in DEPOT_ENVS else TrainableNARGNNEncoder
            encoder = cls(embed_dim=embed_dim, env_name=env_name, init_embedding=init_embedding, edge_embedding=edge_embedding,
                          graph_network=graph_network, heatmap_generator=heatmap_generator,
                          num_layers_heatmap_generator=num_layers_heatmap_generator,
                          num_layers_graph_encoder=num_layers_graph_encoder, act_fn=act_fn, agg_fn=agg_fn,
                          linear_bias=linear_bias)
        self.encoder = encoder
        self.env_name = env_name
        self.train_decode_type = train_decode_type
        self.val_decode_type = val_decode_type
        self.test_decode_type = test_decode_type

    def forward(self, td, env=None, phase: str = "train", calc_reward: bool = True, return_actions: bool = True,
                return_entropy: bool = False, return_hidden: bool = False, return_init_embeds: bool = False,
                return_sum_log_likelihood: bool = True, actions=None, max_steps=1_000_000, **decoding_kwargs) -> dict:
        name, env_name = "NARGNNPolicy", self.env_name
        if phase not in ("train", "val", "test"):
            raise NotImplementedError(f"{name} serves phase 'train', 'val' and 'test', got {phase!r}")
        if return_entropy:
            raise NotImplementedError(f"{name} does not serve return_entropy=True")
        kw = dict(decoding_kwargs)
        decode_type = kw.pop("decode_type", None) or getattr(self, f"{phase}_decode_type")
        if decode_type not in _DECODE_TYPES:
            raise NotImplementedError(f"{name} serves the decode types {_DECODE_TYPES}, got {decode_type!r}")
        temperature = float(kw.pop("temperature", self.temperature))
        if kw.pop("tanh_clipping", self.tanh_clipping):
            raise NotImplementedError(f"{name} does not serve tanh_clipping")
        if not kw.pop("mask_logits", self.mask_logits):
            raise NotImplementedError(f"{name} does not serve mask_logits=False")
        top_k, top_p = kw.pop("top_k", 0), kw.pop("top_p", 0.0)
        K.decoding_filter(top_k, top_p, 2)  # decoding.py:184: "top-p should be in (0, 1]."
        select_best = bool(kw.pop("select_best", False))
        kw.pop("store_all_logp", None)
        multistart = bool(kw.pop("multistart", False)) or "multistart" in decode_type
        multisample = bool(kw.pop("multisample", False))
        num_starts, num_samples = kw.pop("num_starts", None), kw.pop("num_samples", None)
        start_fn = kw.pop("select_start_nodes_fn", None)
        if kw:
            raise NotImplementedError(f"{name} does not serve the decoding keywords {sorted(kw)}")
        # DecodingStrategy.__init__ (decoding.py:237-253)
        assert not (multistart and multisample), "Using both multistart and multisample is not supported"
        if num_samples and num_starts:
            assert not (num_samples > 1 and num_starts > 1), f"num_samples={num_samples} and num_starts={num_starts} are both > 1"
        if num_samples is not None:
            multisample = num_samples > 1
        if num_starts is not None:
            multistart = num_starts > 1
        if multistart and env_name not in ("tsp", "cvrp"):
            raise NotImplementedError(f"decoding_kwargs['multistart'] is not served for {env_name}: every ant starts at the "
                                      f"depot (multisample); decode type {decode_type!r}")
        if not multistart and env_name == "tsp":
            raise NotImplementedError(f"{name} serves tsp with multistart (a multistart decode type or multistart=True, "
                                      f"num_starts > 1): the ants' kernel starts every tour from a given node")
        if not td["locs"].is_cuda:
            raise NotImplementedError(f"{name} runs inside the MI355X kernels only: td['locs'] on {td['locs'].device}")
        if env is None or isinstance(env, str):
            from .envs import get_env

            env = get_env(env_name if env is None else env)
        batch = td["locs"].shape[0]
        n_rows = num_starts if multistart else num_samples if multisample else 1
        if actions is not None:  # the 'evaluate' strategy: the rows say how many there are per instance
            if actions.dim() != 2 or actions.shape[0] == 0 or actions.shape[0] % batch:
                raise ValueError(f"actions must be [n * B, W] ant-major with B = {batch}, got {tuple(actions.shape)}")
            n_rows = actions.shape[0] // batch
        elif n_rows is None:  # pre_decoder_hook (decoding.py:289-290)
            n_rows = int(env.get_num_starts(td))
        n_rows = int(n_rows)

        hidden, init_embeds = self.encoder(td)
        starts = None
        if multistart and actions is None:  # pre_decoder_hook: called once
            starts = start_fn(td, env, n_rows) if start_fn is not None else env.select_start_nodes(td, num_starts=n_rows)
            starts = starts.to(device=hidden.device, dtype=torch.int64).reshape(-1)
        elif multistart and env_name == "cvrp":
            starts = actions[:, 0]  # (says that column 0 is a given customer)
        rolled = heatmap_decode(hidden, td["locs"], n_ants=n_rows, decode_type="greedy" if "greedy" in decode_type else "sampling",
                                top_k=top_k, top_p=top_p, start_nodes=starts, actions=actions, temperature=temperature,
                                env_name=env_name, td=td)
        reward, acts = rolled["reward"], rolled["actions"]
        ll = rolled["log_likelihood"] if return_sum_log_likelihood else rolled["logps"]
        if select_best and n_rows > 1 and actions is None:  # DecodingStrategy._select_best: rows are ant-major
            best = reward.view(n_rows, batch).t().max(dim=-1)[1]
            rows = best * batch + torch.arange(batch, device=best.device)
            reward, acts, ll = reward[rows], acts[rows], ll[rows]
        out = {"reward": reward, "log_likelihood": ll} if calc_reward else {"log_likelihood": ll}
        if return_actions:
            out["actions"] = acts
        if return_hidden:
            out["hidden"] = hidden
        if return_init_embeds:
            out["init_embeds"] = init_embeds
        return out
