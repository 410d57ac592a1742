"""Ant System search on a heatmap: the reference's ``AntSystem`` (models/zoo/deepaco/antsystem.py), DeepACO's test-time
loop, behind its own class surface with the loop inside ONE kernel launch (``rl4co_aco_tsp``, csrc/aco_tsp.hip; for CVRP
``rl4co_aco_cvrp``, csrc/aco_cvrp.hip).

``run`` without local search is one launch for all iterations and one read-back of the error word. With
``use_local_search`` every iteration is a SAMPLE launch, ``env.local_search`` (the 2-opt kernel, from ``td["locs"]``, on the
device), ``env.get_reward`` and an UPDATE launch. With ``use_nls`` as well (DeepACO's neural-guided local search) the local
search of an iteration is ONE launch instead (``rl4co_tsp_nls``, csrc/tsp_nls.hip): the 2-opt, then ``n_perturbations``
rounds of a 2-opt over ``heuristic_dist`` (the heatmap's distances) and a 2-opt over the real distances, the better tour
kept per ant, rewards included. The update (best tour, reward map, pheromone) is the reference's bit for bit; the sampled
tours follow the kernel's own noise (Philox), so they are the reference's in distribution, not draw for draw. Served: TSP,
``use_local_search``, ``use_nls``, ``multistart`` decoding with ``num_starts == n_ants``, ``select_start_nodes_fn``,
``temperature``. Refused (``NotImplementedError``): other environments, ``top_k`` / ``top_p`` / ``multisample`` and any
other decoding keyword, CPU tensors (with ``use_nls`` by the constructor already: ``heuristic_dist`` is built on the
heatmap's device).

CVRP (``env.name == "cvrp"``, the heatmap's node 0 is the depot): ``multisample`` with ``num_samples == n_ants`` (DeepACO's
default: every ant starts at the depot) or ``multistart`` with ``num_starts == n_ants``; no local search (the reference's
is the external HGS library, so ``use_local_search`` and with it ``use_nls`` stay refused). The kernel's rows are
``W = max(C + 1, 2 C - 1)`` wide and zero-filled after each row's length, and every reward is the one of that W-wide row (csrc/aco_cvrp.hip states why). ``final_actions`` is the reference's
ragged list: entry ``b`` has the width the reference's batch had in the iteration that last replaced it, the longest row of
that iteration, which takes one small read-back (with the error word) after the launch.

OP and PCTSP (``env.name`` "op", "pctsp" or "spctsp"; ``rl4co_aco_prize``, csrc/aco_prize.hip): ``multisample`` with
``num_samples == n_ants`` only, no local search (the reference's destroy-and-repair search is not served) and no
``multistart``. ``td`` is the environment's reset state: ``prize`` and ``max_length`` (OP), ``real_prize`` and ``penalty``
(PCTSP; ``real_prize`` is the stochastic prize under ``SPCTSPEnv``). Rows are ``W = n`` wide and zero-filled after each
row's length, the reward is ``env.get_reward`` on that W-wide row, ``final_actions`` is the ragged list as for CVRP.

Training: :func:`heatmap_rollout` is DeepACO's constructive training decode — for TSP the SAMPLE launch of
``rl4co_aco_tsp`` forward, ``rl4co_aco_tsp_logp_grad`` (csrc/aco_tsp_grad.hip) backward; with ``env_name`` "cvrp", "op",
"pctsp" or "spctsp" the SAMPLE launch of ``rl4co_aco_cvrp`` / ``rl4co_aco_prize`` forward and
``rl4co_aco_depot_logp_grad`` (csrc/aco_depot_grad.hip) backward; every pair joined by the one ``torch.autograd.Function`` below — and
:func:`deepaco_loss` the model's REINFORCE loss with the shared baseline (deepaco/model.py:79-91).
``rl4co_amd.NonAutoregressivePolicy`` (rl4co_amd/nargnn.py) is the reference's training surface over it.
:func:`gfacs_loss`, :func:`log_pb_uniform`, :func:`gfacs_alpha` and :func:`gfacs_beta` are GFACS's trajectory-balance loss and
its two schedules (gfacs/model.py); ``rl4co_amd.GFACSPolicy`` returns what the loss reads."""
from __future__ import annotations

import math
from functools import cached_property
from typing import NamedTuple

import torch
from torch import Tensor

from . import _lib
from . import kernels as K


class _Serves(NamedTuple):
    """What ``AntSystem`` serves per environment: the decoding keywords, why ``use_local_search`` is refused (None: it is
    served) and which of multistart / multisample a run may ask for (two: exactly one of them)."""
    kwargs: tuple[str, ...]
    no_local_search: str | None
    modes: tuple[str, ...]


_SERVED_KWARGS = ("multistart", "num_starts", "select_best", "select_start_nodes_fn", "temperature")
_PRIZE = _Serves(("multisample", "num_samples", "select_best", "temperature"),
                 "the reference's destroy-and-repair local search is not part of the Ant System kernel", ("multisample",))
_SERVES = {"tsp": _Serves(_SERVED_KWARGS, None, ("multistart",)),
           "cvrp": _Serves(_SERVED_KWARGS + ("multisample", "num_samples"),
                           "the reference's CVRP local search is the external HGS library", ("multistart", "multisample")),
           "op": _PRIZE, "pctsp": _PRIZE, "spctsp": _PRIZE}  # spctsp is pctsp with the stochastic prize in td["real_prize"]
_NUM_KEY = {"multistart": "num_starts", "multisample": "num_samples"}


def _instance(env_name: str, td, dev) -> dict:
    """The instance tensors of ``td`` under the bindings' keywords (``kernels.ACO_TD_KEYS``), fp32 on ``dev``."""
    return {kw: td[key].detach().to(device=dev, dtype=torch.float32).contiguous() for kw, key in K.ACO_TD_KEYS[env_name]}


class _AntLogLikelihood(torch.autograd.Function):
    """The ants' per-step log-probs and their sum as functions of the heatmap: the forward is the SAMPLE launch of the
    environment's search kernel (``kernels.aco_search``; pheromone of ones, alpha = beta = 1: ``rl4co_logf(1) == 0`` exactly,
    so its logits ARE the heatmap), the backward is its log-likelihood gradient kernel (``kernels.aco_logp_grad``). ``data``:
    ``locs`` and the instance tensors the bindings take by name; ``lengths`` is None for tsp. ``decode``: the options
    ``greedy`` / ``top_k`` / ``top_p`` of both launches (empty: the symbols without them). Nothing is saved unless the
    heatmap requires a gradient; there is no double backward."""

    @staticmethod
    def forward(ctx, heatmap, env_name, data, start_nodes, forced, n_ants, temperature, seed, err, decode):
        kw = dict(data, **decode)
        if K.aco_family(env_name).start_nodes:
            kw["start_nodes"] = None if start_nodes is None else start_nodes[None].contiguous()
        out = K.aco_search(env_name, torch.ones_like(heatmap), n_ants=n_ants, phases=_lib.ACO_SAMPLE, log_heuristic=heatmap,
                           forced_actions=forced, temperature=temperature, philox_seed=seed, philox_offset=0, err=err, **kw)
        actions, lengths, logps, reward = out["actions"], out.get("lengths"), out["logps"], out["reward"]
        ctx.set_materialize_grads(False)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(heatmap, actions)
            ctx.temperature, ctx.err, ctx.env_name, ctx.multistart = temperature, err, env_name, start_nodes is not None
            ctx.decode = decode
            ctx.data = {key: data[key] for key, _ in K.aco_grad_family(env_name).needs[env_name]}
        ctx.mark_non_differentiable(*(t for t in (actions, lengths, reward) if t is not None))
        return logps, logps.sum(1), actions, lengths, reward

    @staticmethod
    def backward(ctx, grad_logps, grad_ll, _grad_actions, _grad_lengths, _grad_reward):
        fam = K.aco_grad_family(ctx.env_name)
        if torch.is_grad_enabled():
            raise RuntimeError(f"heatmap_rollout has no double backward: {fam.symbol} is not differentiable "
                               "(create_graph=True is not served)")
        heatmap, actions = ctx.saved_tensors
        if grad_ll is None:
            grad_ll = torch.zeros(actions.shape[0], dtype=torch.float32, device=heatmap.device)
        grad_ll = grad_ll.to(torch.float32).contiguous()
        if grad_logps is not None:
            grad_logps = grad_logps.to(torch.float32).contiguous()
        own = ctx.err is None
        err = K.new_error_word(heatmap.device) if own else ctx.err
        grad = K.aco_logp_grad(ctx.env_name, heatmap, actions, grad_ll, grad_steps=grad_logps, temperature=ctx.temperature,
                               err=err, **ctx.data, **ctx.decode, **({"multistart": ctx.multistart} if fam.depot else {}))
        if own:
            _lib.raise_for_error_bits(int(err.item()))
        return grad, None, None, None, None, None, None, None, None, None


def heatmap_rollout(heatmap: Tensor, locs: Tensor, *, n_ants: int, start_nodes: Tensor | None = None,
                    actions: Tensor | None = None, temperature: float = 1.0, seed: int | None = None,
                    err: Tensor | None = None, env_name: str = "tsp", td=None) -> dict:
    """:func:`heatmap_decode` with ``decode_type="sampling"`` and no filter.

    DeepACO's constructive training rollout for TSP (``ConstructivePolicy.forward`` under ``NonAutoregressiveDecoder``:
    ``n_ants`` tours per instance sampled step by step from ``softmax(heatmap[b, current, unvisited] / temperature)``) as
    ONE launch, with the gradient back to ``heatmap`` [B, N, N] as one more.

    Rows are ant-major: row ``j * B + b`` is ant ``j`` of instance ``b``. ``start_nodes`` int64 [rows] (None: ant ``j``
    starts at node ``j % N``, TSPEnv's own multistart choice); ``actions`` [rows, N]: these tours are followed and only
    evaluated (the reference's ``forced_actions``). Returns ``actions`` [rows, N], ``logps`` [rows, N] (column 0 is 0),
    ``log_likelihood`` [rows] and ``reward`` [rows] (bit-equal to ``TSPEnv.get_reward``); ``logps`` and
    ``log_likelihood`` carry the gradient when ``heatmap.requires_grad``. ``seed``: the Philox key (None: drawn from
    torch's CPU generator). ``err``: the caller's sticky error word, both launches OR into it and nothing is synchronised;
    None: the forward launch reads its own word back and a set bit raises, and so does the backward launch.

    ``env_name`` "cvrp", "op", "pctsp" or "spctsp" (node 0 of the heatmap is the depot): ``td`` is the environment's reset
    state (``demand`` and ``vehicle_capacity``; ``prize`` and ``max_length``; ``real_prize`` and ``penalty``). Every ant
    starts at the depot and samples its first action from row 0; ``start_nodes`` (cvrp only) are given customers. Rows are
    ``W`` wide (``kernels.aco_depot_width``) and zero-filled after ``lengths`` [rows], which is returned too; ``logps``
    [rows, W] are 0 there, ``reward`` is the environment's ``get_reward`` on the W-wide row. ``actions`` [rows, W] are
    followed and evaluated (with ``start_nodes`` given too, column 0 is the multistart start)."""
    return heatmap_decode(heatmap, locs, n_ants=n_ants, start_nodes=start_nodes, actions=actions, temperature=temperature,
                          seed=seed, err=err, env_name=env_name, td=td)


def heatmap_decode(heatmap: Tensor, locs: Tensor, *, n_ants: int, decode_type: str = "sampling", top_k: int = 0,
                   top_p: float = 0.0, start_nodes: Tensor | None = None, actions: Tensor | None = None,
                   temperature: float = 1.0, seed: int | None = None, err: Tensor | None = None, env_name: str = "tsp",
                   td=None) -> dict:
    """One constructive decode of a heatmap, ``n_ants`` rows per instance, as ONE launch (the gradient back to ``heatmap``
    as one more): NonAutoregressiveDecoder's rows under the reference's ``Sampling`` or ``Greedy`` strategy with
    ``process_logits`` (utils/decoding.py:138-188) at every step. Every keyword, shape and returned key is
    :func:`heatmap_rollout`'s; on top of it:

    ``decode_type`` "sampling" (the Philox noise of ``seed``) or "greedy" (the argmax of the step's log-probs, the lowest
    node on equal values; no noise, ``seed`` is not drawn). ``top_k`` / ``top_p``: the step's feasible logits are cut to
    the ``top_k`` largest (ties at the k-th value stay) and then to the nucleus of mass ``top_p`` before the log-softmax,
    so log-probs, ``log_likelihood`` and the gradient are those of the filtered distribution (a removed node gets gradient
    0). Given ``actions`` are evaluated under the same filter: an action outside a step's kept set has log-prob -inf and
    raises the reference's "Logprobs should not be -inf". With "sampling" and no filter this is :func:`heatmap_rollout`,
    launch for launch."""
    if decode_type not in ("sampling", "greedy"):
        raise NotImplementedError(f"heatmap_decode serves decode_type 'sampling' and 'greedy', got {decode_type!r}")
    greedy = decode_type == "greedy"
    for name, t in (("heatmap", heatmap), ("locs", locs)):
        if not t.is_cuda:
            raise NotImplementedError(f"heatmap_rollout runs inside the MI355X kernel (rl4co_aco_tsp) only: {name} on {t.device}")
    if env_name not in K.ACO_TD_KEYS:
        raise NotImplementedError(f"heatmap_rollout serves tsp, cvrp, op, pctsp and spctsp, got env_name={env_name!r}")
    fam = K.aco_family(env_name)
    depot = fam.ragged  # node 0 is the depot
    if depot and td is None:
        raise ValueError(f"heatmap_rollout(env_name={env_name!r}) takes td=: the instance's reset state (demand and "
                         f"vehicle_capacity; prize and max_length; real_prize and penalty)")
    for _, key in K.ACO_TD_KEYS[env_name]:
        if not td[key].is_cuda:
            raise NotImplementedError(f"heatmap_rollout runs inside the MI355X kernels only: td[{key!r}] on {td[key].device}")
    if heatmap.dim() != 3 or heatmap.shape[1] != heatmap.shape[2]:
        raise ValueError(f"heatmap must be {'[B, n, n]' if depot else '[B, N, N]'}, got {tuple(heatmap.shape)}")
    if start_nodes is not None and not fam.start_nodes:
        raise NotImplementedError(f"start_nodes (multistart) is served for tsp and cvrp, not for {env_name!r}: every ant "
                                  f"starts at the depot")
    b, n, _ = heatmap.shape
    n_ants = int(n_ants)
    rows, w = n_ants * b, fam.width(n)
    dev = heatmap.device
    heatmap = heatmap.to(torch.float32).contiguous()
    data = {"locs": locs.detach().to(device=dev, dtype=torch.float32).contiguous(), **_instance(env_name, td, dev)}
    if actions is not None:
        actions = actions.detach().to(device=dev, dtype=torch.int64).contiguous()
        if tuple(actions.shape) != (rows, w):
            raise ValueError(f"actions must be {(rows, w)}, got {tuple(actions.shape)}")
        if start_nodes is not None or not depot:
            start_nodes = actions[:, 0]
    elif start_nodes is None and not depot:  # TSPEnv's own multistart choice; on a depot graph every ant starts at the depot
        start_nodes = (torch.arange(n_ants, device=dev) % n).repeat_interleave(b)
    if start_nodes is not None:
        start_nodes = start_nodes.detach().to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        if start_nodes.shape[0] != rows:
            raise ValueError(f"start_nodes must be [n_ants * B] = [{rows}], got {tuple(start_nodes.shape)}")
    if seed is None:
        seed = 0 if greedy else int(torch.randint(0, 2**62, (1,)).item())
    top_k, top_p = K.decoding_filter(top_k, top_p, n)
    decode = {key: value for key, value in (("greedy", greedy), ("top_k", top_k), ("top_p", top_p)) if value}
    # err goes through as it is: with None the forward launch and the backward launch each read their own word
    logps, ll, acts, lengths, reward = _AntLogLikelihood.apply(heatmap, env_name, data, start_nodes, actions, n_ants,
                                                               float(temperature), int(seed), err, decode)
    out = {"actions": acts, "lengths": lengths, "logps": logps, "log_likelihood": ll, "reward": reward}
    if not depot:
        del out["lengths"]
    return out


def deepaco_loss(out: dict, train_with_local_search: bool = False, ls_reward_aug_W: float = 0.95) -> Tensor:
    """deepaco/model.py:79-91: REINFORCE with the mean over an instance's ants as the shared baseline; with local search
    the advantage is ``(1 - W)`` of the sampled tours' and ``W`` of the improved tours'. ``out``: ``reward``,
    ``log_likelihood`` and (local search) ``ls_reward``, each [B, n_ants]."""
    reward = out["reward"]
    advantage = reward - reward.mean(dim=1, keepdim=True)
    if train_with_local_search:
        ls_reward = out["ls_reward"]
        ls_advantage = ls_reward - ls_reward.mean(dim=1, keepdim=True)
        advantage = advantage * (1 - ls_reward_aug_W) + ls_advantage * ls_reward_aug_W
    return -(advantage * out["log_likelihood"]).mean()


def log_pb_uniform(actions: Tensor, env_name: str, n_ants: int):
    """gfacs/model.py:140-157, ``GFACS.calculate_log_pb_uniform``: the log of the uniform backward policy of a trajectory.
    tsp: ``log(1 / 2 * N)`` as the reference writes it; op and pctsp: ``log(1 / 2)``; cvrp: per row
    ``-lgamma(routes + 1) - multinode_routes log 2`` from counts of non-zeros of ``actions`` [n_ants * B, W] and of its
    shifted differences, float64 [B, n_ants] -- the reference's formula with ``torch.lgamma`` on the actions' device in
    place of numpy and scipy on the host: no read-back."""
    if env_name == "tsp":
        return math.log(1 / 2 * actions.size(1))
    if env_name == "cvrp":
        a = actions.detach()
        n_nodes = torch.count_nonzero(a, dim=1)
        n_routes = torch.count_nonzero(a[:, 1:] - a[:, :-1], dim=1) - n_nodes
        n_multinode_routes = torch.count_nonzero(a[:, 2:] - a[:, :-2], dim=1) - n_nodes
        log_b_p = -torch.lgamma((n_routes + 1).to(torch.float64)) - n_multinode_routes.to(torch.float64) * math.log(2)
        return log_b_p.view(n_ants, -1).t()  # unbatchify: ant-major rows -> [B, n_ants]
    if env_name in ("op", "pctsp"):
        return math.log(1 / 2)
    raise ValueError(f"Unknown environment: {env_name}")


def gfacs_loss(out: dict, env_name: str, alpha: float = 1.0, beta: float = 1.0, train_with_local_search: bool = False) -> Tensor:
    """gfacs/model.py:107-138, ``GFACS.calculate_loss``: the trajectory-balance loss ``mean((log_likelihood + logZ -
    log_pb_uniform - beta * advantage)^2)`` with the mean over an instance's ants as the baseline; with local search the
    advantage is ``(1 - alpha)`` of the sampled tours' and ``alpha`` of the improved tours', and the same loss on the
    improved tours (``ls_log_likelihood``, ``ls_logZ``, ``ls_actions``, their own advantage) is added. ``out`` is
    ``GFACSPolicy``'s train-phase dict: ``reward``, ``log_likelihood`` [B, n_ants], ``logZ`` [B, 1], ``actions`` ant-major."""
    reward = out["reward"]
    n_ants = reward.size(1)
    advantage = reward - reward.mean(dim=1, keepdim=True)
    if train_with_local_search:
        ls_reward = out["ls_reward"]
        ls_advantage = ls_reward - ls_reward.mean(dim=1, keepdim=True)
        weighted_advantage = advantage * (1 - alpha) + ls_advantage * alpha
    else:
        weighted_advantage = advantage
    forward_flow = out["log_likelihood"] + out["logZ"].repeat(1, n_ants)
    backward_flow = log_pb_uniform(out["actions"], env_name, n_ants) + weighted_advantage.detach() * beta
    tb_loss = torch.pow(forward_flow - backward_flow, 2).mean()
    if train_with_local_search:
        ls_forward_flow = out["ls_log_likelihood"] + out["ls_logZ"].repeat(1, n_ants)
        ls_backward_flow = log_pb_uniform(out["ls_actions"], env_name, n_ants) + ls_advantage.detach() * beta
        tb_loss = tb_loss + torch.pow(ls_forward_flow - ls_backward_flow, 2).mean()
    return tb_loss


def gfacs_alpha(epoch: int, max_epochs: int, alpha_min: float = 0.5, alpha_max: float = 1.0, alpha_flat_epochs: int = 5) -> float:
    """gfacs/model.py:75-80: the weight of the improved tours' advantage, linear in the epoch up to ``alpha_max``."""
    return alpha_min + (alpha_max - alpha_min) * min(epoch / (max_epochs - alpha_flat_epochs), 1.0)


def gfacs_beta(epoch: int, max_epochs: int, beta_min: float = 1.0, beta_max: float = 1.0, beta_flat_epochs: int = 5) -> float:
    """gfacs/model.py:82-88: the inverse temperature of the reward, logarithmic in the epoch up to ``beta_max``."""
    return beta_min + (beta_max - beta_min) * min(math.log(epoch + 1) / math.log(max_epochs - beta_flat_epochs), 1.0)


class AntSystem:
    """antsystem.py:15-76, attribute for attribute. ``Q`` defaults to ``1 / n_ants / decay``."""

    def __init__(self, log_heuristic: Tensor, n_ants: int = 20, alpha: float = 1.0, beta: float = 1.0, decay: float = 0.95,
                 Q: float | None = None, pheromone: Tensor | int | None = None, use_local_search: bool = False,
                 use_nls: bool = False, n_perturbations: int = 1, local_search_params: dict = {},
                 perturbation_params: dict = {}):
        self.batch_size = log_heuristic.shape[0]
        self.n_ants = n_ants
        self.alpha = alpha
        self.beta = beta
        self.decay = decay
        self.Q = 1 / self.n_ants / self.decay if Q is None else Q
        self.log_heuristic = log_heuristic
        if pheromone is None or isinstance(pheromone, int):
            self.pheromone = torch.ones_like(log_heuristic)
            self.pheromone.fill_(pheromone if isinstance(pheromone, int) else 1)
        else:
            assert pheromone.shape == log_heuristic.shape
            self.pheromone = pheromone
        self.final_actions = self.final_reward = None
        self.final_reward_cache: dict = {}
        self.use_local_search = use_local_search
        assert not (use_nls and not use_local_search), "use_nls requires use_local_search"
        if use_nls and not log_heuristic.is_cuda:  # heuristic_dist and the search live on the heatmap's device
            raise NotImplementedError(f"use_nls (neural-guided local search) runs inside the MI355X kernel (rl4co_tsp_nls) "
                                      f"only: log_heuristic on {log_heuristic.device}")
        self.use_nls = use_nls
        self.n_perturbations = n_perturbations
        self.local_search_params = local_search_params.copy()
        self.perturbation_params = perturbation_params.copy()
        self.last_iterations: dict | None = None  # tests only: per-iteration actions / rewards of the last run
        self._err: Tensor | None = None  # the error word of the iteration in flight (None: local_search reads back its own)

    @cached_property
    def heuristic_dist(self) -> Tensor:
        """antsystem.py:78-85 on the device of ``log_heuristic``: the heatmap as a distance matrix [B, N, N] fp32, 0 on the
        diagonal (the local search adds its 1e9 there)."""
        heuristic = self.log_heuristic.detach().to(torch.float32).exp() + 1e-10
        heuristic_dist = 1 / (heuristic / heuristic.max(-1, keepdim=True)[0] + 1e-5)
        n = heuristic_dist.shape[1]
        heuristic_dist[:, torch.arange(n), torch.arange(n)] = 0
        return heuristic_dist.contiguous()

    # ---- what the kernel takes ---------------------------------------------------------------------------------------
    def _check(self, td, env, decoding_kwargs: dict) -> float:
        name = getattr(env, "name", None)
        if name not in _SERVES:
            raise NotImplementedError(f"AntSystem serves the tsp, cvrp, op, pctsp and spctsp environments only (rl4co_aco_tsp, "
                                      f"rl4co_aco_cvrp, rl4co_aco_prize), got {getattr(env, 'name', env)!r}")
        serves = _SERVES[name]
        if self.use_local_search and serves.no_local_search:
            raise NotImplementedError(f"use_local_search is not served for {name}: {serves.no_local_search}")
        if "multistart" not in serves.modes and decoding_kwargs.get("multistart", False):
            raise NotImplementedError(f"decoding_kwargs['multistart'] is not served for {name}: every ant starts at the depot "
                                      f"(multisample)")
        for key in decoding_kwargs:
            if key not in serves.kwargs and key != "multistart":
                raise NotImplementedError(f"decoding_kwargs[{key!r}] is not served by the Ant System kernel for {name}")
        on = [mode for mode in serves.modes if decoding_kwargs.get(mode, False)]
        if len(on) != 1:
            asked = " and ".join(f"decoding_kwargs[{mode!r}]" for mode in serves.modes)
            raise NotImplementedError(f"{'exactly one of ' if len(serves.modes) > 1 else ''}{asked} must be True for {name}")
        if decoding_kwargs.get(_NUM_KEY[on[0]], self.n_ants) != self.n_ants:
            raise NotImplementedError(f"decoding_kwargs[{_NUM_KEY[on[0]]!r}] must equal n_ants = {self.n_ants}")
        if decoding_kwargs.get("select_best", False):
            raise NotImplementedError("decoding_kwargs['select_best'] must be False: the update needs every ant's tour")
        for what, t in (("log_heuristic", self.log_heuristic), ("pheromone", self.pheromone), ("td['locs']", td["locs"])):
            if not t.is_cuda:  # (before any other key of td is touched)
                raise NotImplementedError(f"AntSystem runs inside the MI355X kernel ({K.aco_family(name).symbol}) only: "
                                          f"{what} on {t.device} (env {name!r})")
        return float(decoding_kwargs.get("temperature", 1.0))

    def _tensors(self, td):
        dev = self.log_heuristic.device
        heu = self.log_heuristic.detach().to(torch.float32).contiguous()
        if self.pheromone.dtype != torch.float32 or not self.pheromone.is_contiguous():
            self.pheromone = self.pheromone.detach().to(torch.float32).contiguous()
        return heu, td["locs"].detach().to(device=dev, dtype=torch.float32).contiguous()

    def _start_nodes(self, td, env, decoding_kwargs: dict) -> Tensor:
        """Sampling.pre_decoder_hook (decoding.py:304-311): called once per iteration."""
        fn = decoding_kwargs.get("select_start_nodes_fn", None)
        nodes = fn(td, env, self.n_ants) if fn is not None else env.select_start_nodes(td, num_starts=self.n_ants)
        return nodes.to(device=self.log_heuristic.device, dtype=torch.int64).reshape(-1)

    def _next_seed(self) -> tuple[int, int]:
        """The Philox key of one launch: drawn from torch's (CPU) generator, so ``torch.manual_seed`` reproduces a run."""
        return int(torch.randint(0, 2**62, (1,)).item()), 0

    def _common(self, temperature: float) -> dict:
        return dict(n_ants=self.n_ants, alpha=float(self.alpha), beta=float(self.beta), decay=float(self.decay),
                    Q=float(self.Q), temperature=temperature)

    def _record(self):
        has = self.final_reward is not None
        return dict(has_best=has, final_reward=self.final_reward if has else None,
                    final_actions=torch.stack(self.final_actions, 0).contiguous() if has else None)

    def _take_record(self, out: dict) -> None:
        self.final_reward = out["final_reward"]
        self.final_actions = list(out["final_actions"].unbind(0))

    # ---- AntSystem.run (antsystem.py:87-118) -----------------------------------------------------------------------------
    def run(self, td_initial, env, n_iterations: int, decoding_kwargs: dict, disable_tqdm: bool = True):
        temperature = self._check(td_initial, env, decoding_kwargs)
        if K.aco_family(env.name).ragged:
            out = self._sampling(td_initial, env, decoding_kwargs, temperature, n_iterations)
            for i in range(n_iterations):
                self.final_reward_cache[i] = out["final_reward_cache"][i].clone()
            self.last_iterations = {"actions": out["iter_actions"], "reward": out["iter_reward"], "lengths": out["iter_lengths"]}
            return self._convert_final_action_to_matrix(), self.final_reward_cache
        if self.use_local_search:
            acts, rews, sampled = [], [], []
            for i in range(n_iterations):
                a, r = self._one_step(td_initial, env, decoding_kwargs)
                acts.append(a)
                rews.append(r)
                sampled.append(self._sampled_reward)
                self.final_reward_cache[i] = self.final_reward.clone()
            self.last_iterations = {"actions": torch.stack(acts, 0), "reward": torch.stack(rews, 0),
                                    "sampled_reward": torch.stack(sampled, 0)}
            return self._convert_final_action_to_matrix(), self.final_reward_cache
        heu, locs = self._tensors(td_initial)
        starts = torch.stack([self._start_nodes(td_initial, env, decoding_kwargs) for _ in range(n_iterations)], 0)
        seed, offset = self._next_seed()
        err = K.new_error_word(heu.device)
        out = K.aco_tsp(self.pheromone, iterations=n_iterations, log_heuristic=heu, locs=locs, start_nodes=starts.contiguous(),
                        philox_seed=seed, philox_offset=offset, record_iterations=True, err=err, **self._record(),
                        **self._common(temperature))
        _lib.raise_for_error_bits(int(err.item()))  # the one read-back of the run
        self._take_record(out)
        for i in range(n_iterations):
            self.final_reward_cache[i] = out["final_reward_cache"][i].clone()
        self.last_iterations = {"actions": out["iter_actions"], "reward": out["iter_reward"]}
        return self._convert_final_action_to_matrix(), self.final_reward_cache

    # ---- AntSystem._one_step (antsystem.py:120-147) ----------------------------------------------------------------------
    def _one_step(self, td, env, decoding_kwargs: dict):
        """One iteration: sample, optional local search, update. Returns (actions [rows, N], reward [rows]), ant-major."""
        temperature = self._check(td, env, decoding_kwargs)
        if K.aco_family(env.name).ragged:  # actions [rows, W], zero-filled after each row's length
            out = self._sampling(td, env, decoding_kwargs, temperature, 1)
            return out["actions"], out["reward"]
        heu, locs = self._tensors(td)
        starts = self._start_nodes(td, env, decoding_kwargs)[None].contiguous()
        seed, offset = self._next_seed()
        err = K.new_error_word(heu.device)
        common = self._common(temperature)
        if not self.use_local_search:
            out = K.aco_tsp(self.pheromone, log_heuristic=heu, locs=locs, start_nodes=starts, philox_seed=seed,
                            philox_offset=offset, err=err, **self._record(), **common)
            actions, reward = out["actions"], out["reward"]
        else:
            sampled = K.aco_tsp(self.pheromone, phases=_lib.ACO_SAMPLE, log_heuristic=heu, locs=locs, start_nodes=starts,
                                philox_seed=seed, philox_offset=offset, err=err, **common)
            self._sampled_reward = sampled["reward"]  # (tests: the local search never makes a tour longer)
            self._err = err  # the NLS launch ORs into this iteration's word: read back once, below
            try:
                actions, reward = self.local_search(td, env, sampled["actions"], decoding_kwargs)
            finally:
                self._err = None
            out = K.aco_tsp(self.pheromone, phases=_lib.ACO_UPDATE, actions=actions.contiguous(),
                            reward=reward.to(torch.float32).contiguous(), err=err, **self._record(), **common)
        _lib.raise_for_error_bits(int(err.item()))
        self._take_record(out)
        return actions, reward

    # ---- depot graphs: sampling and update of ``n_iterations`` iterations in one launch (rl4co_aco_cvrp, rl4co_aco_prize) ------
    def _sampling(self, td, env, decoding_kwargs: dict, temperature: float, n_iterations: int) -> dict:
        heu, locs = self._tensors(td)
        dev = heu.device
        data = _instance(env.name, td, dev)
        if decoding_kwargs.get("multistart", False):  # Sampling.pre_decoder_hook: called once per iteration
            data["start_nodes"] = torch.stack([self._start_nodes(td, env, decoding_kwargs) for _ in range(n_iterations)],
                                              0).contiguous()
        seed, offset = self._next_seed()
        err = K.new_error_word(dev)
        record = self._padded_record(K.aco_family(env.name).width(heu.shape[1]))
        out = K.aco_search(env.name, self.pheromone, iterations=n_iterations, log_heuristic=heu, locs=locs, philox_seed=seed,
                           philox_offset=offset, record_iterations=True, err=err, **data, **record, **self._common(temperature))
        self._take_ragged_record(out, err, record["has_best"])
        return out

    def _padded_record(self, width: int) -> dict:
        has = self.final_reward is not None
        record = dict(has_best=has, final_reward=self.final_reward if has else None, final_actions=None)
        if has:  # the ragged list, zero-padded to the kernel's width
            record["final_actions"] = torch.stack(
                [torch.nn.functional.pad(t, (0, width - t.shape[0])) for t in self.final_actions], 0).contiguous()
        return record

    def _take_ragged_record(self, out: dict, err: Tensor, has: bool) -> None:
        """The one read-back of the run: the error word, which iteration last replaced each record, every iteration's width."""
        b = self.batch_size
        widths = out["iter_lengths"].amax(1).to(torch.int32)
        host = torch.cat((err, out["final_iteration"], widths)).tolist()
        _lib.raise_for_error_bits(host[0])
        replaced, widths = host[1 : 1 + b], host[1 + b :]
        self.final_reward = out["final_reward"]
        if not has:
            self.final_actions = [None] * b
        for i, it in enumerate(replaced):  # antsystem.py:238-245: the entry has the width of its iteration's batch
            if it >= 0:
                self.final_actions[i] = out["final_actions"][i, : widths[it]].clone()

    # ---- AntSystem.local_search (antsystem.py:173-230), without the host round trip --------------------------------------
    def local_search(self, td, env, actions: Tensor, decoding_kwargs: dict):
        if getattr(env, "name", None) != "tsp":
            raise NotImplementedError(f"Local search not implemented for {getattr(env, 'name', env)}")
        if self.use_nls:
            return self._nls(td, actions)
        locs = td["locs"]
        rows = actions.shape[0]
        # one instance row per ant row (ant-major, the reference's batchify): the 2-opt kernel pairs tour r with instance r
        tiled = {"locs": locs.repeat(rows // locs.shape[0], 1, 1)} if locs.shape[0] != rows else {"locs": locs}
        best_actions = env.local_search(td=tiled, actions=actions, **self.local_search_params)
        best_rewards = env.get_reward(tiled, best_actions)
        return best_actions, best_rewards

    @staticmethod
    def _max_iterations(params: dict, name: str) -> int:
        """``env.local_search(td, actions, max_iterations=1000, num_threads=0)``: any other key is a TypeError there."""
        for key in params:
            if key not in ("max_iterations", "num_threads"):  # num_threads: accepted and ignored (one workgroup per tour)
                raise TypeError(f"local_search() got an unexpected keyword argument {key!r} (from {name})")
        return int(params.get("max_iterations", 1000))

    def _nls(self, td, actions: Tensor):
        """The whole of antsystem.py:204-225 in one launch; the caller's error word, no read-back of its own."""
        ls_cap = self._max_iterations(self.local_search_params, "local_search_params")
        perturb_cap = self._max_iterations(self.perturbation_params, "perturbation_params")
        dev = self.log_heuristic.device
        if not actions.is_cuda or not dev.type == "cuda":
            raise NotImplementedError(f"neural-guided local search runs inside the MI355X kernel (rl4co_tsp_nls) only: "
                                      f"actions on {actions.device}, log_heuristic on {dev}")
        locs = td["locs"].detach().to(device=dev, dtype=torch.float32).contiguous()
        return K.tsp_nls(actions.contiguous(), locs=locs, perturb_distances=self.heuristic_dist,
                         n_perturbations=int(self.n_perturbations), ls_max_iterations=ls_cap,
                         perturb_max_iterations=perturb_cap, err=self._err)

    def _convert_final_action_to_matrix(self) -> Tensor:
        assert self.final_actions is not None
        count = max(len(t) for t in self.final_actions)  # antsystem.py:284-294: zero-padded to the longest entry
        if all(len(t) == count for t in self.final_actions):
            return torch.stack(self.final_actions, 0)
        return torch.stack([torch.nn.functional.pad(t, (0, count - len(t))) for t in self.final_actions], 0)
