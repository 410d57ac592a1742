"""Thin torch-tensor front end over the C-ABI (``include/rl4co_amd.h``).

torch is plumbing here: it owns device memory and the HIP stream; every function below hands
raw device pointers + sizes to ``librl4co_amd.so`` on ``torch.cuda.current_stream()``.
There is no CPU path: a non-CUDA tensor is an error.
"""
from __future__ import annotations

import ctypes as C
import inspect
from typing import Callable, NamedTuple

import torch
from torch import Tensor

from . import _lib
from .cache import FoldedCache
from .envspec import SPECS, EnvSpec, spec

MODE_IDS = {"greedy": _lib.DECODE_GREEDY, "sampling": _lib.DECODE_SAMPLE, "evaluate": _lib.DECODE_EVALUATE}
ENV_IDS = {name: sp.env_id for name, sp in SPECS.items()}
VARIANT_IDS = {"auto": _lib.VARIANT_AUTO, "stream": _lib.VARIANT_STREAM, "lds": _lib.VARIANT_LDS, "wide": _lib.VARIANT_WIDE, "ms": _lib.VARIANT_MS,
               "stream_reg": _lib.VARIANT_STREAM_REG}


def decode_row_groups(num_nodes: int, cache_dtype: torch.dtype, max_steps: int, variant: str = "auto",
                      num_trajectories: int = 1 << 20, num_instances: int | None = None) -> int:
    """Row groups of the specified-order contract of the variant that would run (0 = the multistart
    MFMA variant, which has none)."""
    dt = _lib.dtype_id(cache_dtype)
    return _lib.decode_row_groups(num_nodes, dt, max_steps, VARIANT_IDS[variant], num_trajectories, num_instances)


def decode_variant(num_nodes: int, cache_dtype: torch.dtype, max_steps: int, num_trajectories: int,
                   num_instances: int | None = None, env_name: str = "tsp") -> int:
    """The RL4CO_VARIANT_* rl4co_am_decode would run for this shape (host query)."""
    a = _lib.AmDecodeArgs()
    a.env = spec(env_name).env_id
    a.N, a.max_steps, a.B = int(num_nodes), int(max_steps), int(num_trajectories)
    a.B_inst = int(num_trajectories if num_instances is None else num_instances)
    a.cache_dtype = _lib.dtype_id(cache_dtype)
    return _lib.lib().rl4co_am_decode_variant(C.byref(a))


def _ptr(t: Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(t: Tensor, dtype: torch.dtype | None = None, name: str = "tensor") -> Tensor:
    if not t.is_cuda:
        raise _lib.Rl4coLibraryError(
            f"{name} lives on {t.device}; the rl4co_amd kernels only run on the MI355X (no CPU fallback)"
        )
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def _ctx_table(a, t: Tensor, plane_dtype: torch.dtype, name: str) -> Tensor:
    """A folded context table for ``rl4co_am_decode_args``: dense fp32 [B,N,128] (every variant), or — multistart variant —
    rows in the planes' 16-bit type with any (instance, node) strides, e.g. a column block of the fused fold GEMM's output
    matrix (``teacher.build_cache_autograd(fused_planes=True)``): sets ctx_dtype / ctx_row_stride / ctx_batch_stride."""
    if not t.is_cuda:
        raise _lib.Rl4coLibraryError(f"{name} lives on {t.device}; the rl4co_amd kernels only run on the MI355X (no CPU fallback)")
    if t.dtype == torch.float32:
        return _dev(t, torch.float32, name)
    if t.dtype != plane_dtype or t.dim() != 3 or t.stride(2) != 1:
        raise TypeError(f"{name} must be fp32, or [B,N,128] in the planes' dtype {plane_dtype} with unit channel stride")
    dt, rs, bs = _lib.dtype_id(t.dtype), t.stride(1), t.stride(0)
    if a.ctx_dtype not in (0, dt) or (a.ctx_row_stride not in (0, rs)) or (a.ctx_batch_stride not in (0, bs)):
        raise ValueError("ctx_first and ctx_cur must share dtype and strides")
    a.ctx_dtype, a.ctx_row_stride, a.ctx_batch_stride = dt, rs, bs
    return t


def _u8(t: Tensor, name: str) -> Tensor:
    """bool tensors share the uint8 storage the kernels read/write."""
    _dev(t, None, name)
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    if t.dtype != torch.uint8:
        raise TypeError(f"{name} must be bool or uint8, got {t.dtype}")
    return t


def _check_rows(b: int, **tensors) -> None:
    """Every per-trajectory tensor of a step call must hold exactly ``b`` rows (the mask's): a shorter ``action``
    (e.g. an instance-level action against batchified multistart state) would be read out of bounds on the device."""
    for name, t in tensors.items():
        if t is not None and t.shape[0] != b:
            raise ValueError(f"{name} has {t.shape[0]} rows, action_mask has {b}")


_SLOT_DTYPES = {"i64": torch.int64, "f32": torch.float32}


def bind_env_state(a, sp: EnvSpec, state: dict, b: int, n: int) -> int:
    """Fill the state slots of an ``AmDecodeArgs`` / ``EnvReplayArgs`` from the environment's table (envspec.py): every
    tensor on the device, of its dtype and contiguous; per-trajectory tensors with ``b`` rows, instance data with one row
    count (returned: B_inst; ``b`` for an environment without instance data) and its shape behind it."""
    replay = isinstance(a, _lib.EnvReplayArgs)
    b_inst = None
    for f in sp.fields:
        t = _u8(state[f.key], f.key) if f.dtype == "u8" else _dev(state[f.key], _SLOT_DTYPES[f.dtype], f.key)
        if f.kind == "traj":
            _check_rows(b, **{f.key: t})
        else:
            b_inst = t.shape[0] if b_inst is None else b_inst
            if t.shape[0] != b_inst:
                raise ValueError(f"{f.key} has {t.shape[0]} rows, expected {b_inst}")
            dims = {"N-1": (n - 1,), "N": (n,), "N2": (n, 2), "": ()}[f.shape]
            if tuple(t.shape[1:]) != dims:
                raise ValueError(f"{f.key} must be [B_inst, {', '.join(map(str, dims))}], got {tuple(t.shape)}")
        if f.kind == "traj" and f.shape == "BN" and tuple(t.shape) != (b, n):  # (a short row would be read and written past its end)
            raise ValueError(f"{f.key} must be [{b}, {n}], got {tuple(t.shape)}")
        # (the replay kernel keeps the running context scalar, whichever it is, in one slot)
        running = replay and sp.scalar is not None and f.key == sp.scalar.running
        setattr(a, "scalar" if running else f.slot, t.data_ptr())
    b_inst = b if b_inst is None else b_inst
    if b % b_inst:
        raise ValueError(f"{b} trajectories over {b_inst} instances")
    return b_inst


def env_step(env_name: str, state, action: Tensor | None, err: Tensor | None = None) -> None:
    """The environment's in-place step entry (``tsp_step``, ``cvrp_step``, ...) on its state tensors, looked up in this
    module when called."""
    entry, keys = spec(env_name).step
    globals()[entry](action, *(state[k] for k in keys), err)


def new_error_word(device) -> Tensor:
    return torch.zeros(1, dtype=torch.int32, device=device)


def raise_if_error(err: Tensor) -> None:
    """ONE host sync per rollout instead of the reference's 4-5 per decode step."""
    _lib.raise_for_error_bits(int(err.item()))


# ------------------------------------------------------------------------------------------------


def gather_by_index(src: Tensor, idx: Tensor, err: Tensor | None = None) -> Tensor:
    """ops.py:54-66 for src [B,N,D] fp32, idx [B,K] int64 -> [B,K,D]."""
    _dev(src, torch.float32, "src"), _dev(idx, torch.int64, "idx")
    b, n, d = src.shape
    k = idx.shape[1]
    out = torch.empty((b, k, d), dtype=torch.float32, device=src.device)
    st = _lib.lib().rl4co_gather_by_index_f32(_ptr(src), _ptr(idx), b, n, d, k, _ptr(out), _ptr(err), _stream())
    _lib.check(st, "rl4co_gather_by_index_f32")
    return out


def tour_length(locs: Tensor, actions: Tensor, prepend_depot: bool = False, negate: bool = False,
                horizon: tuple[Tensor, int] | None = None) -> Tensor:
    """ops.py:82-90 over gather(locs, actions) (+ depot for CVRP, cvrp/env.py:138-147).

    locs [B_locs,N,2] fp32 with B % B_locs == 0 (s-major multistart), actions [B,T] int64.
    ``horizon = (steps_dev, t_add)``: the tour is the first ``t_add + steps_dev[0]`` columns of the (padded) buffer,
    the count read on the device (rl4co_tour_length_dyn_f32) — no host value needed."""
    _dev(locs, torch.float32, "locs"), _dev(actions, torch.int64, "actions")
    b, t = actions.shape
    b_locs, n, two = locs.shape
    assert two == 2
    out = torch.empty((b,), dtype=torch.float32, device=locs.device)
    if horizon is not None:
        steps_dev, t_add = horizon
        st = _lib.lib().rl4co_tour_length_dyn_f32(_ptr(locs), _ptr(actions), b, b_locs, n, t, _ptr(_dev(steps_dev, torch.int32, "steps")),
                                                  int(t_add), int(prepend_depot), int(negate), _ptr(out), _stream())
        _lib.check(st, "rl4co_tour_length_dyn_f32")
        return out
    st = _lib.lib().rl4co_tour_length_f32(
        _ptr(locs), _ptr(actions), b, b_locs, n, t, int(prepend_depot), int(negate), _ptr(out), _stream()
    )
    _lib.check(st, "rl4co_tour_length_f32")
    return out


def tsp_check_solution(actions: Tensor, num_nodes: int, err: Tensor) -> None:
    _dev(actions, torch.int64, "actions")
    b, t = actions.shape
    st = _lib.lib().rl4co_tsp_check_solution(_ptr(actions), b, num_nodes, t, _ptr(err), _stream())
    _lib.check(st, "rl4co_tsp_check_solution")


def cvrp_check_solution(actions: Tensor, demand: Tensor, vehicle_capacity: Tensor, err: Tensor) -> None:
    _dev(actions, torch.int64, "actions"), _dev(demand, torch.float32, "demand")
    _dev(vehicle_capacity, torch.float32, "vehicle_capacity")
    b, t = actions.shape
    b_inst, n1 = demand.shape
    st = _lib.lib().rl4co_cvrp_check_solution(
        _ptr(actions), _ptr(demand), _ptr(vehicle_capacity), b, b_inst, n1 + 1, t, _ptr(err), _stream()
    )
    _lib.check(st, "rl4co_cvrp_check_solution")


def tsp_step(action: Tensor, action_mask: Tensor, first_node: Tensor, current_node: Tensor,
             step_i: Tensor, done: Tensor, err: Tensor | None = None) -> None:
    """In-place TSPEnv._step (tsp/env.py:60-86)."""
    _dev(action, torch.int64, "action")
    mask = _u8(action_mask, "action_mask")
    b, n = mask.shape
    _check_rows(b, action=action, first_node=first_node, current_node=current_node, i=step_i, done=done)
    st = _lib.lib().rl4co_tsp_step(
        _ptr(action), _ptr(mask), _ptr(_dev(first_node, torch.int64, "first_node")),
        _ptr(_dev(current_node, torch.int64, "current_node")), _ptr(_dev(step_i, torch.int64, "i")),
        _ptr(_u8(done, "done")), b, n, _ptr(err), _stream(),
    )
    _lib.check(st, "rl4co_tsp_step")


def cvrp_step(action: Tensor | None, demand: Tensor, used_capacity: Tensor, vehicle_capacity: Tensor,
              visited: Tensor, current_node: Tensor, action_mask: Tensor, done: Tensor | None,
              err: Tensor | None = None) -> None:
    """In-place CVRPEnv._step + get_action_mask (cvrp/env.py:66-96,126-136); action=None -> mask only."""
    mask = _u8(action_mask, "action_mask")
    b, n = mask.shape
    b_inst = demand.shape[0]
    _check_rows(b, action=action, used_capacity=used_capacity, vehicle_capacity=vehicle_capacity, visited=visited,
                current_node=current_node, done=done)
    st = _lib.lib().rl4co_cvrp_step(
        _ptr(None if action is None else _dev(action, torch.int64, "action")),
        _ptr(_dev(demand, torch.float32, "demand")), _ptr(_dev(used_capacity, torch.float32, "used_capacity")),
        _ptr(_dev(vehicle_capacity, torch.float32, "vehicle_capacity")), _ptr(_u8(visited, "visited")),
        _ptr(_dev(current_node, torch.int64, "current_node")), _ptr(mask),
        _ptr(None if done is None else _u8(done, "done")), b, b_inst, n, _ptr(err), _stream(),
    )
    _lib.check(st, "rl4co_cvrp_step")


def sdvrp_step(action: Tensor | None, demand_with_depot: Tensor, used_capacity: Tensor, vehicle_capacity: Tensor,
               current_node: Tensor, action_mask: Tensor, done: Tensor | None, err: Tensor | None = None) -> None:
    """In-place SDVRPEnv._step + get_action_mask (sdvrp/env.py:56-123); action=None -> mask only.
    ``demand_with_depot`` [B, N] is per trajectory and updated."""
    mask = _u8(action_mask, "action_mask")
    b, n = mask.shape
    _check_rows(b, action=action, demand_with_depot=demand_with_depot, used_capacity=used_capacity,
                vehicle_capacity=vehicle_capacity, current_node=current_node, done=done)
    if tuple(demand_with_depot.shape) != (b, n):
        raise ValueError(f"demand_with_depot must be [{b}, {n}], got {tuple(demand_with_depot.shape)}")
    st = _lib.lib().rl4co_sdvrp_step(
        _ptr(None if action is None else _dev(action, torch.int64, "action")),
        _ptr(_dev(demand_with_depot, torch.float32, "demand_with_depot")), _ptr(_dev(used_capacity, torch.float32, "used_capacity")),
        _ptr(_dev(vehicle_capacity, torch.float32, "vehicle_capacity")), _ptr(_dev(current_node, torch.int64, "current_node")),
        _ptr(mask), _ptr(None if done is None else _u8(done, "done")), b, n, _ptr(err), _stream())
    _lib.check(st, "rl4co_sdvrp_step")


def mtsp_step(action: Tensor, locs: Tensor, num_agents: Tensor, agent_idx: Tensor, current_length: Tensor,
              max_subtour_length: Tensor, current_node: Tensor, action_mask: Tensor, done: Tensor,
              err: Tensor | None = None) -> None:
    """In-place MTSPEnv._step (mtsp/env.py:63-131): the mask is the state, the reward is ``-max_subtour_length``.
    ``locs`` [B_inst, N, 2] / ``num_agents`` [B_inst] are instance data (trajectory b reads row b % B_inst)."""
    mask = _u8(action_mask, "action_mask")
    b, n = mask.shape
    _check_rows(b, action=action, agent_idx=agent_idx, current_length=current_length, max_subtour_length=max_subtour_length,
                current_node=current_node, done=done)
    b_inst = locs.shape[0]
    if tuple(locs.shape) != (b_inst, n, 2) or tuple(num_agents.shape) != (b_inst,) or b % b_inst:
        raise ValueError(f"locs must be [B_inst, {n}, 2] and num_agents [B_inst] with {b} % B_inst == 0, got "
                         f"{tuple(locs.shape)} and {tuple(num_agents.shape)}")
    st = _lib.lib().rl4co_mtsp_step(
        _ptr(_dev(action, torch.int64, "action")), _ptr(_dev(locs, torch.float32, "locs")),
        _ptr(_dev(num_agents, torch.int64, "num_agents")), _ptr(_dev(agent_idx, torch.int64, "agent_idx")),
        _ptr(_dev(current_length, torch.float32, "current_length")),
        _ptr(_dev(max_subtour_length, torch.float32, "max_subtour_length")),
        _ptr(_dev(current_node, torch.int64, "current_node")), _ptr(mask), _ptr(_u8(done, "done")), b, b_inst, n, _ptr(err),
        _stream())
    _lib.check(st, "rl4co_mtsp_step")


def select_start_nodes(batch: int, num_starts: int, num_loc: int, has_depot: bool, device) -> Tensor:
    """ops.py:128-161: s-major ``arange(S).repeat_interleave(B) % num_loc (+1)``."""
    out = torch.empty((batch * num_starts,), dtype=torch.int64, device=device)
    if not out.is_cuda:
        raise _lib.Rl4coLibraryError("select_start_nodes needs a CUDA device")
    st = _lib.lib().rl4co_select_start_nodes(_ptr(out), batch, num_starts, num_loc, int(has_depot), _stream())
    _lib.check(st, "rl4co_select_start_nodes")
    return out


def _bind_cache_and_state(a, sp: EnvSpec, cache: FoldedCache, state: dict, b: int, n: int, ctx_table) -> list:
    """What ``rl4co_am_decode_args`` and ``rl4co_am_decode_beam_args`` have in common (same field names): the three plane
    pointers with their strides, the folded context (not in the unfolded parity mode) and the environment's state.
    ``ctx_table(tensor, name)`` gives the tensor a context-table slot is bound to — the one difference between the two
    kernels. Returns those tensors: the caller holds them until its launch."""
    kvl = cache.kvl  # [3, B, N, 128]: plane pointers + (instance, node) strides — any view with unit channel stride
    if not kvl.is_cuda:
        raise _lib.Rl4coLibraryError(f"cache.kvl lives on {kvl.device}; the rl4co_amd kernels only run on the MI355X (no CPU fallback)")
    if not (kvl.dim() == 4 and kvl.stride(3) == 1):
        raise ValueError("cache.kvl must be [3, B, N, 128] with unit stride along the channels")
    a.cache_dtype = _lib.dtype_id(kvl.dtype)
    a.glimpse_key, a.glimpse_val, a.logit_key = (cache.plane(i).data_ptr() for i in range(3))
    a.kvl_row_stride, a.kvl_batch_stride = cache.row_stride, cache.batch_stride
    tables = []
    if not cache.unfold:
        tables.append(ctx_table(cache.ctx_cur, "ctx_cur"))
        a.ctx_cur = _ptr(tables[-1])
    a.q_bias = _ptr(None if cache.q_bias is None else _dev(cache.q_bias, torch.float32, "q_bias"))
    if not cache.unfold:  # what the folded context needs besides its tables, by the context's layout
        if sp.ctx_first:
            tables.append(ctx_table(cache.ctx_first, "ctx_first"))
            a.ctx_first = _ptr(tables[-1])
            a.q_step0 = _ptr(_dev(cache.q_step0, torch.float32, "q_step0"))
        if sp.scalar is not None:
            a.w_cap = _ptr(_dev(cache.w_cap, torch.float32, "w_cap"))
    b_inst = bind_env_state(a, sp, state, b, n)
    assert b_inst == cache.num_instances or not sp.keys("inst"), "instance data rows must match cache instances"
    return tables


def am_decode(
    cache: FoldedCache,
    state: dict,
    *,
    mode: str,
    max_steps: int,
    actions: Tensor,
    logps: Tensor,
    err: Tensor,
    t0: int = 0,
    tanh_clipping: float = 10.0,
    temperature: float = 1.0,
    mask_inner: bool = True,
    mask_logits: bool = True,
    exp_noise: Tensor | None = None,
    philox_seed: int = 0,
    philox_offset: int = 0,
    philox_seed_dev: Tensor | None = None,
    forced_actions: Tensor | None = None,
    all_logps: Tensor | None = None,
    entropy: Tensor | None = None,
    n_steps: Tensor | None = None,
    steps_summary: Tensor | None = None,
    variant: str = "auto",
    top_k: int = 0,
    top_p: float = 0.0,
    kept_bits: Tensor | None = None,
) -> None:
    """Run ``max_steps`` fused decode steps (1 = a single step, >= horizon = whole rollout).

    ``state`` holds the environment tensors (updated in place): the fields of the environment's record in ``envspec.py``
    (``policy._initial_state`` builds them).
    ``top_k`` / ``top_p``: the reference's top-k / nucleus filter (utils/decoding.py:109-188; see ``decoding_filter``).
    ``kept_bits`` [B, out_stride, W] int32 (W = 4 * ceil(N / 128), the layout of ``env_replay``'s mask bits): per step taken,
    bit j of the row = node j kept (feasible and not filtered); the columns of steps not taken are left as they are.
    """
    sp = spec(cache.env_name)
    a = _lib.AmDecodeArgs()
    b, n = state["action_mask"].shape
    assert n == cache.num_nodes, (n, cache.num_nodes)
    a.env = sp.env_id
    a.B, a.B_inst, a.N = b, cache.num_instances, n
    a.mode = MODE_IDS[mode]
    a.max_steps = int(max_steps)
    a.variant = VARIANT_IDS[variant]
    a.mask_inner, a.mask_logits = int(mask_inner), int(mask_logits)
    a.tanh_clipping, a.temperature = float(tanh_clipping), float(temperature)
    if cache.unfold and not sp.unfold:
        raise ValueError("the unfolded parity mode serves tsp / cvrp")
    # 16-bit context tables go through as they are, with their strides (_ctx_table)
    _bind_cache_and_state(a, sp, cache, state, b, n, lambda t, name: _ctx_table(a, t, cache.kvl.dtype, name))
    if cache.unfold:  # reference-association parity mode: per-step GEMVs against the raw weights (cache.py)
        a.unfold, a.ctx_width = 1, cache.w_ctx_t.shape[0]
        a.node_embed = _ptr(_dev(cache.node_embed, torch.float32, "node_embed"))
        a.w_ctx_t = _ptr(_dev(cache.w_ctx_t, torch.float32, "w_ctx_t"))
        a.w_out_t = _ptr(_dev(cache.w_out_t, torch.float32, "w_out_t"))
        a.w_placeholder = _ptr(None if cache.w_placeholder is None else _dev(cache.w_placeholder, torch.float32, "w_placeholder"))
    elif sp.scalar is not None and sp.scalar.clock:
        a.w_time = _ptr(_dev(cache.w_time, torch.float32, "w_time"))
    if sp.dynamic is not None:  # the dynamic embedding, folded to three vectors (cache.fold_dynamic)
        dyn = _dev(cache.dyn, torch.float32, "dyn")
        if tuple(dyn.shape) != (3, 128):
            raise ValueError(f"cache.dyn must be [3, 128], got {tuple(dyn.shape)}")
        setattr(a, sp.dynamic.slot, dyn.data_ptr())
    if sp.feats is not None:  # several running scalars: their folded context vectors, one row each (cache.fold_features)
        feat = _dev(cache.feat, torch.float32, "feat")
        if tuple(feat.shape) != (len(sp.feats.names), 128):
            raise ValueError(f"cache.feat must be [{len(sp.feats.names)}, 128], got {tuple(feat.shape)}")
        if b != cache.num_instances:
            raise ValueError(f"{sp.name} runs one trajectory per instance (no multistart rows): {b} trajectories over "
                             f"{cache.num_instances} instances")
        a.mtsp_ctx = feat.data_ptr()
    if exp_noise is not None:
        _dev(exp_noise, torch.float32, "exp_noise")
        assert exp_noise.numel() >= max_steps * b * n, "exp_noise must hold [max_steps,B,N] draws"
        a.exp_noise = _ptr(exp_noise)
    a.philox_seed, a.philox_offset = int(philox_seed), int(philox_offset)
    if philox_seed_dev is not None:
        a.philox_seed_dev = _ptr(_dev(philox_seed_dev, torch.int64, "philox_seed_dev"))
    if forced_actions is not None:
        _dev(forced_actions, torch.int64, "forced_actions")
        assert forced_actions.shape == actions.shape
        a.forced_actions = _ptr(forced_actions)
    _dev(actions, torch.int64, "actions"), _dev(logps, torch.float32, "logps")
    assert actions.shape == logps.shape and actions.shape[0] == b
    a.t0, a.out_stride = int(t0), actions.shape[1]
    a.actions, a.logps = _ptr(actions), _ptr(logps)
    a.all_logps = _ptr(None if all_logps is None else _dev(all_logps, torch.float32, "all_logps"))
    a.entropy = _ptr(None if entropy is None else _dev(entropy, torch.float32, "entropy"))
    a.n_steps = _ptr(None if n_steps is None else _dev(n_steps, torch.int32, "n_steps"))
    if steps_summary is not None:  # [max steps, sum steps, rows low, rows high]: the row counter is ONE 64-bit word
        _dev(steps_summary, torch.int32, "steps_summary")
        if steps_summary.numel() < 4 or steps_summary.data_ptr() % 8:
            raise ValueError("steps_summary must be 4 int32 words on an 8-byte boundary (rl4co_am_decode_args.steps_summary)")
    a.steps_summary = _ptr(steps_summary)
    a.err = _ptr(_dev(err, torch.int32, "err"))
    a.top_k, a.top_p = decoding_filter(top_k, top_p, n)
    if kept_bits is not None:
        _dev(kept_bits, torch.int32, "kept_bits")
        words = 4 * ((n + 127) // 128)
        if tuple(kept_bits.shape) != (b, actions.shape[1], words) or not kept_bits.is_contiguous():
            raise ValueError(f"kept_bits must be a contiguous [{b}, {actions.shape[1]}, {words}] int32 tensor")
        a.kept_bits, a.kept_words = _ptr(kept_bits), words
    st = _lib.lib().rl4co_am_decode(C.byref(a), _stream())
    _lib.check(st, "rl4co_am_decode")


def beam_max_width(n: int) -> int:
    """Largest ``beam_width`` the beam-search kernel serves for ``n`` nodes (its LDS budget; a host query)."""
    return int(_lib.lib().rl4co_am_decode_beam_max_width(int(n)))


def beam_served(sp: EnvSpec) -> bool:
    """The environments rl4co_am_decode_beam accepts, by the ids its argument check admits."""
    return sp.env_id in (_lib.ENV_TSP, _lib.ENV_CVRP)


def am_decode_beam(
    cache: FoldedCache,
    state: dict,
    beam_width: int,
    max_steps: int,
    *,
    actions: Tensor,
    logps: Tensor,
    step_nodes: Tensor,
    step_logps: Tensor,
    parents: Tensor,
    cum_logp: Tensor,
    err: Tensor,
    tanh_clipping: float = 10.0,
    temperature: float = 1.0,
    mask_inner: bool = True,
    mask_logits: bool = True,
    steps_summary: Tensor | None = None,
) -> None:
    """Beam search (utils/decoding.py:464-600) over ``beam_width`` beams per instance in one launch (rl4co_am_decode_beam).

    ``state``: the environment's tensors (envspec.py) of the ``beam_width * B`` beam rows, beam-major, AFTER the imposed
    start step; updated in place. Outputs are ``[beam_width * B, T]`` with ``T >= max_steps + 1``: column 0 is the start
    node, the steps fill columns 1 .. ; ``actions`` / ``logps`` (int64 / fp32) are the aligned final beams, best first,
    ``step_nodes`` / ``parents`` (int32), ``step_logps`` / ``cum_logp`` (fp32) the per-step selections before alignment."""
    sp = spec(cache.env_name)
    if not beam_served(sp):
        raise NotImplementedError(f"beam search is not served for {sp.name} (tsp and cvrp are)")
    if cache.unfold:
        raise NotImplementedError("beam search needs the folded cache (fold=True)")
    a = _lib.AmDecodeBeamArgs()
    b, n = state["action_mask"].shape
    w = int(beam_width)
    assert w > 1, "beam width must be larger than 1"  # decoding.py:494
    assert n == cache.num_nodes, (n, cache.num_nodes)
    if b != w * cache.num_instances:
        raise ValueError(f"{b} state rows for {w} beams over {cache.num_instances} instances")
    if w > beam_max_width(n):
        raise NotImplementedError(f"beam search with {w} beams over {n} nodes is beyond the kernel's limit of "
                                  f"{beam_max_width(n)} beams at that size")
    a.env, a.B_inst, a.N, a.beam_width, a.max_steps = sp.env_id, cache.num_instances, n, w, int(max_steps)
    a.mask_inner, a.mask_logits = int(mask_inner), int(mask_logits)
    a.tanh_clipping, a.temperature = float(tanh_clipping), float(temperature)

    def table(t: Tensor, name: str) -> Tensor:  # dense fp32 (a 16-bit table is widened: exact)
        return _dev(t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous(), torch.float32, name)

    keep = _bind_cache_and_state(a, sp, cache, state, b, n, table)  # noqa: F841  (alive until the launch)
    t_len = actions.shape[1]
    if t_len < int(max_steps) + 1:
        raise ValueError(f"outputs hold {t_len} columns, {int(max_steps)} steps need {int(max_steps) + 1}")
    for name, t, dt in (("actions", actions, torch.int64), ("logps", logps, torch.float32), ("step_nodes", step_nodes, torch.int32),
                        ("step_logps", step_logps, torch.float32), ("parents", parents, torch.int32), ("cum_logp", cum_logp, torch.float32)):
        _dev(t, dt, name)
        if tuple(t.shape) != (b, t_len):
            raise ValueError(f"{name} must be [{b}, {t_len}], got {tuple(t.shape)}")
        setattr(a, name, t.data_ptr())
    a.out_stride = t_len
    if steps_summary is not None:
        _dev(steps_summary, torch.int32, "steps_summary")
        if steps_summary.numel() < 2:
            raise ValueError("steps_summary must hold 2 int32 words")
    a.steps_summary = _ptr(steps_summary)
    a.err = _ptr(_dev(err, torch.int32, "err"))
    st = _lib.lib().rl4co_am_decode_beam(C.byref(a), _stream())
    _lib.check(st, "rl4co_am_decode_beam")


def two_opt_lds_nodes() -> int:
    """Largest node count whose distance matrix the 2-opt kernel keeps in LDS (its LDS budget; a host query)."""
    return int(_lib.lib().rl4co_tsp_two_opt_lds_nodes())


def tsp_two_opt(actions: Tensor, *, locs: Tensor | None = None, distances: Tensor | None = None,
                max_iterations: int = 1000, err: Tensor | None = None, return_iterations: bool = False,
                out: Tensor | None = None):
    """Best-improvement 2-opt on every tour of ``actions`` [B, T] (tsp/local_search.py:16-81) in one launch
    (rl4co_tsp_two_opt), bit for bit the reference's result; equal improvements go to the lowest ``(i, j)``.

    Exactly one of ``locs`` [B, N, 2] and ``distances`` [B, N, N] (fp32; the matrix may be asymmetric), N and T up to
    1024. Returns the new int64 tours, and the int32 scan counts [B] with ``return_iterations``. ``out``: where the tours
    go (``out is actions``: in place). With ``err`` the sticky bits are OR-ed into the caller's word and nothing is
    synchronised; without it the word is read back and an out-of-range index raises."""
    if (locs is None) == (distances is None):
        raise ValueError("tsp_two_opt takes exactly one of locs and distances")
    if actions.dim() != 2:
        raise ValueError(f"actions must be [B, T], got {tuple(actions.shape)}")
    if actions.dtype != torch.int64:
        raise TypeError(f"actions must be torch.int64, got {actions.dtype}")
    b, t = actions.shape
    src = locs if distances is None else distances
    if src.dtype != torch.float32:
        raise TypeError(f"{'locs' if distances is None else 'distances'} must be torch.float32, got {src.dtype}")
    n = src.shape[1] if src.dim() == 3 else -1
    if src.dim() != 3 or src.shape[0] != b or (src.shape[2] != 2 if distances is None else src.shape[2] != n):
        raise ValueError(f"{'locs must be [B, N, 2]' if distances is None else 'distances must be [B, N, N]'} with B = {b}, "
                         f"got {tuple(src.shape)}")
    if not 2 <= n <= 1024 or not 1 <= t <= 1024:
        raise NotImplementedError(f"tsp_two_opt serves 2..1024 nodes and tours of 1..1024 positions, got N = {n}, T = {t}")
    if int(max_iterations) < 0:
        raise ValueError("max_iterations must be >= 0")
    actions = _dev(actions.contiguous(), torch.int64, "actions")
    src = _dev(src.contiguous(), torch.float32, "locs" if distances is None else "distances")
    if out is None:
        out = torch.empty_like(actions)
    elif _dev(out, torch.int64, "out").shape != actions.shape:
        raise ValueError(f"out must be {tuple(actions.shape)}, got {tuple(out.shape)}")
    own = err is None
    err = new_error_word(actions.device) if own else _dev(err, torch.int32, "err")
    iters = torch.empty(b, dtype=torch.int32, device=actions.device) if return_iterations else None
    a = _lib.TspTwoOptArgs()
    a.B, a.N, a.T, a.max_iterations = b, n, t, int(max_iterations)
    a.locs, a.distances = (_ptr(src), None) if distances is None else (None, _ptr(src))
    a.actions, a.out_actions, a.iterations, a.err = _ptr(actions), _ptr(out), _ptr(iters), _ptr(err)
    st = _lib.lib().rl4co_tsp_two_opt(C.byref(a), _stream())
    _lib.check(st, "rl4co_tsp_two_opt")
    if own:
        raise_if_error(err)
    return (out, iters) if return_iterations else out


def nls_lds_nodes() -> int:
    """Largest node count whose distance matrix the NLS kernel keeps in LDS (its LDS budget; a host query)."""
    return int(_lib.lib().rl4co_tsp_nls_lds_nodes())


def tsp_nls(actions: Tensor, *, locs: Tensor, perturb_distances: Tensor, n_perturbations: int,
            ls_max_iterations: int = 1000, perturb_max_iterations: int = 1000, err: Tensor | None = None,
            return_counts: bool = False):
    """Neural-guided local search (DeepACO's NLS, antsystem.py:173-230) on every tour row of ``actions`` [R, T] in one
    launch (rl4co_tsp_nls): a 2-opt over the real distances, then ``n_perturbations`` rounds of a 2-opt over
    ``perturb_distances`` followed by a 2-opt over the real distances, the best tour by reward kept per row.

    ``locs`` [I, N, 2] and ``perturb_distances`` [I, N, N] (fp32, without the 1e9 diagonal, may be asymmetric) with
    ``R % I == 0``: row ``r`` uses instance ``r % I`` (ant-major rows), nothing is tiled per ant. Returns
    ``(actions, reward)``: the best int64 tours [R, T] and their fp32 rewards [R] (``TSPEnv.get_reward`` bit for bit);
    with ``return_counts`` also ``scans`` int32 [R, 1 + 2 * n_perturbations] (scans per 2-opt) and ``accepted`` int32 [R]
    (rounds that replaced the best tour). With ``err`` the sticky bits are OR-ed into the caller's word and nothing is
    synchronised; without it the word is read back and an out-of-range index raises."""
    if actions.dim() != 2:
        raise ValueError(f"actions must be [R, T], got {tuple(actions.shape)}")
    if actions.dtype != torch.int64:
        raise TypeError(f"actions must be torch.int64, got {actions.dtype}")
    rows, t = actions.shape
    for name, src in (("locs", locs), ("perturb_distances", perturb_distances)):
        if src.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32, got {src.dtype}")
    if locs.dim() != 3 or locs.shape[2] != 2:
        raise ValueError(f"locs must be [I, N, 2], got {tuple(locs.shape)}")
    inst, n, _ = locs.shape
    if tuple(perturb_distances.shape) != (inst, n, n):
        raise ValueError(f"perturb_distances must be [I, N, N] = {(inst, n, n)}, got {tuple(perturb_distances.shape)}")
    if inst < 1 or rows % inst != 0:
        raise ValueError(f"the {rows} tour rows must be a multiple of the {inst} instances (R % I == 0)")
    if not 2 <= n <= 1024 or not 1 <= t <= 1024:
        raise NotImplementedError(f"tsp_nls serves 2..1024 nodes and tours of 1..1024 positions, got N = {n}, T = {t}")
    counts = dict(n_perturbations=n_perturbations, ls_max_iterations=ls_max_iterations,
                  perturb_max_iterations=perturb_max_iterations)
    for name, value in counts.items():
        if not 0 <= int(value) < 2**30:
            raise ValueError(f"{name} must be in [0, 2^30), got {value}")
    actions = _dev(actions.contiguous(), torch.int64, "actions")
    locs = _dev(locs.contiguous(), torch.float32, "locs")
    perturb_distances = _dev(perturb_distances.contiguous(), torch.float32, "perturb_distances")
    dev = actions.device
    out = torch.empty_like(actions)
    reward = torch.empty(rows, dtype=torch.float32, device=dev)
    own = err is None
    err = new_error_word(dev) if own else _dev(err, torch.int32, "err")
    scans = torch.empty((rows, 1 + 2 * int(n_perturbations)), dtype=torch.int32, device=dev) if return_counts else None
    accepted = torch.empty(rows, dtype=torch.int32, device=dev) if return_counts else None
    a = _lib.TspNlsArgs()
    a.R, a.n_instances, a.N, a.T = rows, inst, n, t
    a.ls_max_iterations, a.perturb_max_iterations = int(ls_max_iterations), int(perturb_max_iterations)
    a.n_perturbations, a.reserved0 = int(n_perturbations), 0
    a.locs, a.perturb_distances, a.actions = _ptr(locs), _ptr(perturb_distances), _ptr(actions)
    a.out_actions, a.out_reward, a.scans, a.accepted, a.err = _ptr(out), _ptr(reward), _ptr(scans), _ptr(accepted), _ptr(err)
    st = _lib.lib().rl4co_tsp_nls(C.byref(a), _stream())
    _lib.check(st, "rl4co_tsp_nls")
    if own:
        raise_if_error(err)
    return (out, reward, scans, accepted) if return_counts else (out, reward)


def nargnn_lds_nodes(k: int) -> int:
    """Largest node count at which the heatmap encoder keeps the edge state of ``k`` out-edges per node in LDS."""
    return int(_lib.lib().rl4co_nargnn_lds_nodes(int(k)))


_NARGNN_SCRATCH_CAP = 1 << 30  # bytes of scratch a launch may take before the grid is made smaller than the card
_NARGNN_PARAMS = ("init_w", "init_b", "edge_w", "edge_b", "lin_w", "lin_b", "bn", "mlp_w", "mlp_b", "out_w", "out_b")


def _nargnn_launch(symbol: str, a, sizes: tuple, inputs: dict, params: dict, extra: dict, scalars: dict, *, small_value,
                   fill_value, n_workgroups, err):
    """The one body behind :func:`nargnn_heatmap` and :func:`nargnn_depot_heatmap`, from the parameter shapes to the
    launch of ``<symbol>_heatmap``. ``sizes``: (B, N, K, D) as the caller checked them; ``inputs``: the instance tensors as
    name -> (tensor, dtype) in the struct's order; ``params``: the eleven parameter keywords both bindings take;
    ``extra``: the graph's own parameters as name -> (tensor, shape), which stand behind ``init_b``; ``scalars``: the
    struct's own scalar fields."""
    b, n, k, d = sizes
    init_w, init_b, edge_w, edge_b, lin_w, lin_b, bn, mlp_w, mlp_b, out_w, out_b = (params[key] for key in _NARGNN_PARAMS)
    layers = 0 if lin_w is None else lin_w.shape[0]
    if layers and (lin_b is None or bn is None):
        raise ValueError("lin_w needs lin_b and bn")
    hidden = 0 if mlp_w is None else mlp_w.shape[0]
    want = {"init_b": (init_b, (d,)), **extra, "edge_b": (edge_b, (d,)), "lin_w": (lin_w, (layers, 5, d, d)),
            "lin_b": (lin_b if layers else None, (layers, 5, d)), "bn": (bn if layers else None, (layers, 2, 2, d)),
            "mlp_w": (mlp_w, (hidden, d, d)), "mlp_b": (mlp_b, (hidden, d)), "out_b": (out_b, (1,))}
    for name, (t, shape) in want.items():
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
    if mlp_b is not None and hidden == 0:
        mlp_b = None
    edge_w, out_w = edge_w.reshape(-1), out_w.reshape(-1)
    if edge_w.numel() != d or out_w.numel() != d:
        raise ValueError(f"edge_w and out_w must hold {d} values, got {edge_w.numel()} and {out_w.numel()}")
    values = {name: _dev(t, dtype, name) for name, (t, dtype) in inputs.items()}
    named = dict(init_w=init_w, init_b=init_b, **{name: t for name, (t, _) in extra.items()}, edge_w=edge_w, edge_b=edge_b,
                 lin_w=lin_w if layers else None, lin_b=lin_b if layers else None, bn=bn if layers else None,
                 mlp_w=mlp_w if hidden else None, mlp_b=mlp_b, out_w=out_w, out_b=out_b)
    values.update({key: (None if t is None else _dev(t, torch.float32, key)) for key, t in named.items()})
    dev = values["locs"].device
    if fill_value is None:
        fill_value = float(torch.log(torch.tensor(small_value, dtype=torch.float32)))
    per_wg = int(getattr(_lib.lib(), symbol + "_scratch_bytes")(n, k))
    if n_workgroups is None:  # one workgroup per CU (eight waves above 128 VGPRs: a second one does not fit), within the cap
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        n_workgroups = min(b, cus, max(1, _NARGNN_SCRATCH_CAP // per_wg))
    if not 1 <= n_workgroups <= b:
        raise ValueError(f"n_workgroups must be in [1, B = {b}], got {n_workgroups}")
    scratch = torch.empty(n_workgroups * per_wg // 4, dtype=torch.float32, device=dev)
    heatmap = torch.empty((b, n, n), dtype=torch.float32, device=dev)
    node_embed = torch.empty((b, n, d), dtype=torch.float32, device=dev)
    values.update(B=b, N=n, K=k, D=d, L=layers, H=hidden + 1, n_workgroups=int(n_workgroups), **scalars,
                  small_value=float(small_value), fill_value=float(fill_value), scratch=scratch,
                  scratch_bytes=scratch.numel() * 4, heatmap=heatmap, node_embed=node_embed)
    _aco_launch(symbol + "_heatmap", a, values, err, dev)
    return heatmap, node_embed


def nargnn_heatmap(locs: Tensor, neighbors: Tensor, edge_cost: Tensor, *, init_w: Tensor, init_b: Tensor, edge_w: Tensor,
                   edge_b: Tensor, lin_w: Tensor | None, lin_b: Tensor | None, bn: Tensor | None, mlp_w: Tensor | None,
                   mlp_b: Tensor | None, out_w: Tensor, out_b: Tensor | None, small_value: float = 1e-12,
                   fill_value: float | None = None, n_workgroups: int | None = None, err: Tensor | None = None):
    """DeepACO's heatmap encoder for TSP (NARGNNEncoder in inference) in one launch (rl4co_nargnn_heatmap), fp32.

    ``locs`` [B, N, 2], ``neighbors`` [B, N, K] int32 (node u's out-edges go to ``neighbors[b, u]``), ``edge_cost``
    [B, N, K]; ``init_w`` [64, 2], ``init_b`` [64], ``edge_w`` [64] or [64, 1], ``edge_b`` [64]; ``lin_w`` [L, 5, 64, 64]
    (v_lin1 .. v_lin4, e_lin), ``lin_b`` [L, 5, 64], ``bn`` [L, 2, 2, 64] (v_bn, e_bn) x (scale, shift) of the eval-mode
    batch norms, all three ``None`` when L == 0; ``mlp_w`` [H - 1, 64, 64] (``None`` when H == 1), ``mlp_b`` [H - 1, 64]
    or ``None``; ``out_w`` [64] or [1, 64], ``out_b`` [1] or ``None``. ``fill_value`` defaults to the fp32 value of
    ``torch.log`` of ``small_value``. Returns ``(heatmap_logits [B, N, N], node_embed [B, N, 64])``. With ``err`` the
    sticky bits are OR-ed into the caller's word and nothing is synchronised; without it the word is read back and an
    out-of-range neighbour index raises."""
    if locs.dim() != 3 or locs.shape[2] != 2:
        raise ValueError(f"locs must be [B, N, 2], got {tuple(locs.shape)}")
    b, n, _ = locs.shape
    if neighbors.dim() != 3 or tuple(neighbors.shape[:2]) != (b, n):
        raise ValueError(f"neighbors must be [B, N, K] = [{b}, {n}, K], got {tuple(neighbors.shape)}")
    k = neighbors.shape[2]
    if tuple(edge_cost.shape) != (b, n, k):
        raise ValueError(f"edge_cost must be [B, N, K] = {(b, n, k)}, got {tuple(edge_cost.shape)}")
    if init_w.dim() != 2 or init_w.shape[1] != 2:
        raise ValueError(f"init_w must be [D, 2], got {tuple(init_w.shape)}")
    d = init_w.shape[0]
    if d != 64:
        raise NotImplementedError(f"nargnn_heatmap serves embed_dim = 64 only, got {d}")
    if b < 1 or not 2 <= n <= 1024 or not 1 <= k <= min(n - 1, 256):
        raise NotImplementedError(f"nargnn_heatmap serves B >= 1, 2 <= N <= 1024 and 1 <= K <= min(N - 1, 256), got "
                                  f"B = {b}, N = {n}, K = {k}")
    params = dict(init_w=init_w, init_b=init_b, edge_w=edge_w, edge_b=edge_b, lin_w=lin_w, lin_b=lin_b, bn=bn, mlp_w=mlp_w,
                  mlp_b=mlp_b, out_w=out_w, out_b=out_b)
    return _nargnn_launch("rl4co_nargnn", _lib.NargnnArgs(), (b, n, k, d),
                          dict(locs=(locs, torch.float32), neighbors=(neighbors, torch.int32),
                               edge_cost=(edge_cost, torch.float32)), params, {},
                          dict(reserved0=0), small_value=small_value, fill_value=fill_value, n_workgroups=n_workgroups,
                          err=err)


def nargnn_depot_lds_nodes(k: int) -> int:
    """Largest node count (depot included) at which the depot-graph heatmap encoder keeps its (N - 1)(k + 2) edge rows in
    LDS."""
    return int(_lib.lib().rl4co_nargnn_depot_lds_nodes(int(k)))


def nargnn_depot_heatmap(locs: Tensor, feats: Tensor, neighbors: Tensor, edge_cost: Tensor, depot_cost: Tensor, *,
                         init_w: Tensor, init_b: Tensor, depot_w: Tensor, depot_b: Tensor, edge_w: Tensor, edge_b: Tensor,
                         lin_w: Tensor | None, lin_b: Tensor | None, bn: Tensor | None, mlp_w: Tensor | None,
                         mlp_b: Tensor | None, out_w: Tensor, out_b: Tensor | None, small_value: float = 1e-12,
                         fill_value: float | None = None, n_workgroups: int | None = None, err: Tensor | None = None):
    """DeepACO's heatmap encoder for the depot graphs of CVRP, OP and PCTSP in one launch (rl4co_nargnn_depot_heatmap),
    fp32.

    ``locs`` [B, N, 2] (node 0 the depot), ``feats`` [B, N - 1, F] with F in {1, 2}, ``neighbors`` [B, N - 1, K] int32
    (customer u's customer neighbours, values in 1 .. N - 1), ``edge_cost`` [B, N - 1, K], ``depot_cost`` [B, N - 1] (the
    distance between customer u and the depot, for both directions); ``init_w`` [64, 2 + F], ``init_b`` [64], ``depot_w``
    [64, 2], ``depot_b`` [64]; every other parameter as :func:`nargnn_heatmap` takes it. Returns ``(heatmap_logits
    [B, N, N], node_embed [B, N, 64])``. With ``err`` the sticky bits are OR-ed into the caller's word and nothing is
    synchronised; without it the word is read back and a neighbour index outside [1, N) raises."""
    if locs.dim() != 3 or locs.shape[2] != 2:
        raise ValueError(f"locs must be [B, N, 2], got {tuple(locs.shape)}")
    b, n, _ = locs.shape
    c = n - 1
    if feats.dim() != 3 or tuple(feats.shape[:2]) != (b, c):
        raise ValueError(f"feats must be [B, N - 1, F] = [{b}, {c}, F], got {tuple(feats.shape)}")
    f = feats.shape[2]
    if neighbors.dim() != 3 or tuple(neighbors.shape[:2]) != (b, c):
        raise ValueError(f"neighbors must be [B, N - 1, K] = [{b}, {c}, K], got {tuple(neighbors.shape)}")
    k = neighbors.shape[2]
    if tuple(edge_cost.shape) != (b, c, k):
        raise ValueError(f"edge_cost must be [B, N - 1, K] = {(b, c, k)}, got {tuple(edge_cost.shape)}")
    if tuple(depot_cost.shape) != (b, c):
        raise ValueError(f"depot_cost must be [B, N - 1] = {(b, c)}, got {tuple(depot_cost.shape)}")
    if init_w.dim() != 2 or init_w.shape[1] != 2 + f:
        raise ValueError(f"init_w must be [D, 2 + F] = [D, {2 + f}], got {tuple(init_w.shape)}")
    d = init_w.shape[0]
    if d != 64:
        raise NotImplementedError(f"nargnn_depot_heatmap serves embed_dim = 64 only, got {d}")
    if f not in (1, 2):
        raise NotImplementedError(f"nargnn_depot_heatmap serves F = 1 or 2 customer features, got {f}")
    if b < 1 or not 3 <= n <= 1024 or not 1 <= k <= min(n - 2, 256):
        raise NotImplementedError(f"nargnn_depot_heatmap serves B >= 1, 3 <= N <= 1024 and 1 <= K <= min(N - 2, 256), got "
                                  f"B = {b}, N = {n}, K = {k}")
    params = dict(init_w=init_w, init_b=init_b, edge_w=edge_w, edge_b=edge_b, lin_w=lin_w, lin_b=lin_b, bn=bn, mlp_w=mlp_w,
                  mlp_b=mlp_b, out_w=out_w, out_b=out_b)
    return _nargnn_launch("rl4co_nargnn_depot", _lib.NargnnDepotArgs(), (b, n, k, d),
                          dict(locs=(locs, torch.float32), feats=(feats, torch.float32), neighbors=(neighbors, torch.int32),
                               edge_cost=(edge_cost, torch.float32), depot_cost=(depot_cost, torch.float32)),
                          params, dict(depot_w=(depot_w, (d, 2)), depot_b=(depot_b, (d,))),
                          dict(F=f), small_value=small_value, fill_value=fill_value, n_workgroups=n_workgroups, err=err)


# ---- the heatmap encoder's GNN stack in train mode (csrc/nargnn_train.hip) ------------------------------------------------------
def nargnn_train_workspace_bytes(b: int, n: int, k: int, layers: int) -> int:
    """Bytes of workspace the train-mode GNN stack needs at this shape (the formula is in include/rl4co_amd.h); 0 outside the
    served range."""
    return int(_lib.lib().rl4co_nargnn_train_workspace_bytes(int(b), int(n), int(k), int(layers)))


def incoming_csr(neighbors: Tensor) -> tuple[Tensor, Tensor]:
    """The reverse adjacency of ``neighbors`` [B, N, K] over the flat rows: ``(csr_ptr [B N + 1] int32, csr_src [B N K]
    int32)``; positions ``csr_ptr[j] .. csr_ptr[j + 1]`` of ``csr_src`` hold, ascending, the edge rows e = (b N + i) K + k
    that point at the global node j = b N + neighbors[b, i, k]. A stable sort of the targets keeps the rows ascending."""
    b, n, k = neighbors.shape
    target = (neighbors.to(torch.int64) + torch.arange(b, device=neighbors.device).view(b, 1, 1) * n).reshape(-1)
    src = torch.sort(target, stable=True).indices.to(torch.int32)
    # (out-of-range targets are clamped for the count alone: the kernel's check refuses such lists)
    counts = torch.bincount(target.clamp(0, b * n - 1), minlength=b * n)
    ptr = torch.zeros(b * n + 1, dtype=torch.int64, device=neighbors.device)
    ptr[1:] = counts.cumsum(0)
    return ptr.to(torch.int32), src.contiguous()


def depot_incoming_csr(neighbors: Tensor) -> tuple[Tensor, Tensor]:
    """:func:`incoming_csr` over the depot graph's rows: ``neighbors`` [B, C, K] (values in 1 .. N - 1, N = C + 1) gives
    E = C (K + 2) edge rows per instance in the reference's order -- the kNN rows by source, every ``i -> 0``, every
    ``0 -> i`` -- and ``(csr_ptr [B N + 1] int32, csr_src [B E] int32)`` lists, ascending, the rows whose target is each
    global node. A stable sort of the closed-form targets keeps the rows ascending inside a node's run."""
    b, c, k = neighbors.shape
    n = c + 1
    dev = neighbors.device
    zero = torch.zeros(b, c, dtype=torch.int64, device=dev)
    cust = torch.arange(1, n, dtype=torch.int64, device=dev).expand(b, c)
    local = torch.cat((neighbors.to(torch.int64).reshape(b, c * k), zero, cust), 1)
    target = (local + torch.arange(b, device=dev).view(b, 1) * n).reshape(-1)
    src = torch.sort(target, stable=True).indices.to(torch.int32)
    counts = torch.bincount(target.clamp(0, b * n - 1), minlength=b * n)  # (clamped for the count alone, as above)
    ptr = torch.zeros(b * n + 1, dtype=torch.int64, device=dev)
    ptr[1:] = counts.cumsum(0)
    return ptr.to(torch.int32), src.contiguous()


# graph -> (symbol stem, args struct, N from neighbors.shape[1], smallest N, edge rows per instance, the served range in words)
_NARGNN_TRAIN_GRAPHS = {
    "regular": ("rl4co_nargnn_train", _lib.NargnnTrainArgs, lambda m: m, 2, lambda n, k: n * k,
                "B >= 1, 2 <= N <= 1024 and 1 <= K <= min(N - 1, 64)", "B N K <= 2^24"),
    "depot": ("rl4co_nargnn_depot_train", _lib.NargnnDepotTrainArgs, lambda m: m + 1, 3, lambda n, k: (n - 1) * (k + 2),
              "B >= 1, 3 <= N <= 1024 and 1 <= K <= min(N - 2, 64)", "B (N - 1)(K + 2) <= 2^24"),
}


def _nargnn_train_args(neighbors, csr_ptr, csr_src, x_in, w_in, lin_w, lin_b, bn_w, bn_b, eps, graph="regular"):
    stem, struct, nodes_of, min_n, rows_of, served, _ = _NARGNN_TRAIN_GRAPHS[graph]
    b, m, k = neighbors.shape
    n = nodes_of(m)
    e = rows_of(n, k)  # edge rows per instance
    d = x_in.shape[-1]
    if d != 64:
        raise NotImplementedError(f"{stem[6:]} serves embed_dim = 64 only, got {d}")
    if b < 1 or not min_n <= n <= 1024 or not 1 <= k <= min(n - min_n + 1, 64):
        raise NotImplementedError(f"{stem[6:]} serves {served}, got B = {b}, N = {n}, K = {k}")
    layers = 0 if lin_w is None else lin_w.shape[0]
    if layers < 1:
        raise ValueError(f"{stem[6:]} takes at least one layer (without layers the stack is the identity)")
    w_shape = (b, n, k, d) if graph == "regular" else (b, e, d)
    want = dict(x_in=(x_in, (b, n, d)), w_in=(w_in, w_shape), lin_w=(lin_w, (layers, 5, d, d)), lin_b=(lin_b, (layers, 5, d)),
                bn_w=(bn_w, (layers, 2, d)), bn_b=(bn_b, (layers, 2, d)))
    for name, (t, shape) in want.items():
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
    if tuple(csr_ptr.shape) != (b * n + 1,) or tuple(csr_src.shape) != (b * e,):
        raise ValueError(f"csr_ptr must be [{b * n + 1}] and csr_src [{b * e}], got {tuple(csr_ptr.shape)} and "
                         f"{tuple(csr_src.shape)}")
    for name, (t, _) in want.items():
        _dev(t, torch.float32, name)
    for name, t in (("neighbors", neighbors), ("csr_ptr", csr_ptr), ("csr_src", csr_src)):
        _dev(t, torch.int32, name)
    a = struct()
    a.B, a.N, a.K, a.D, a.L, a.reserved0, a.eps, a.reserved1 = b, n, k, d, layers, 0, float(eps), 0
    values = dict(neighbors=neighbors, csr_ptr=csr_ptr, csr_src=csr_src, x_in=x_in, w_in=w_in, lin_w=lin_w, lin_b=lin_b, bn_w=bn_w,
                  bn_b=bn_b)
    return a, values, (b, n, k, d, layers)


def _nargnn_train_launch(symbol: str, a, values: dict, err: Tensor | None, dev) -> None:
    for name, ctype in a._fields_:
        if ctype is C.c_void_p and name != "err":
            setattr(a, name, _ptr(values.get(name)))
    own = err is None
    word = new_error_word(dev) if own else _dev(err, torch.int32, "err")
    a.err = _ptr(word)
    _lib.check(getattr(_lib.lib(), symbol)(C.byref(a), _stream()), symbol)
    if own:
        raise_if_error(word)


def _nargnn_train_forward(graph, neighbors, csr_ptr, csr_src, x_in, w_in, lin_w, lin_b, bn_w, bn_b, eps, err):
    stem, *_, rows = _NARGNN_TRAIN_GRAPHS[graph]
    a, values, (b, n, k, d, layers) = _nargnn_train_args(neighbors, csr_ptr, csr_src, x_in, w_in, lin_w, lin_b, bn_w, bn_b, eps, graph)
    dev = x_in.device
    nbytes = int(getattr(_lib.lib(), stem + "_workspace_bytes")(b, n, k, layers))
    if nbytes <= 0:
        raise NotImplementedError(f"{stem[6:]} does not serve B = {b}, N = {n}, K = {k}, L = {layers} ({rows})")
    workspace = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    x_out = torch.empty((b, n, d), dtype=torch.float32, device=dev)
    w_out = torch.empty(tuple(w_in.shape), dtype=torch.float32, device=dev)
    stats = torch.empty((layers, 6, d), dtype=torch.float32, device=dev)
    a.workspace_bytes = nbytes
    values.update(workspace=workspace, x_out=x_out, w_out=w_out, stats=stats)
    _nargnn_train_launch(stem + "_forward", a, values, err, dev)
    return x_out, w_out, stats, workspace


def _nargnn_train_backward(graph, neighbors, csr_ptr, csr_src, x_in, w_in, lin_w, lin_b, bn_w, bn_b, stats, workspace, grad_x_out,
                           grad_w_out, eps, err) -> dict:
    stem = _NARGNN_TRAIN_GRAPHS[graph][0]
    a, values, (b, n, k, d, layers) = _nargnn_train_args(neighbors, csr_ptr, csr_src, x_in, w_in, lin_w, lin_b, bn_w, bn_b, eps, graph)
    dev = x_in.device
    for name, t, shape in (("grad_x_out", grad_x_out, (b, n, d)), ("grad_w_out", grad_w_out, tuple(w_in.shape)),
                           ("stats", stats, (layers, 6, d))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
        _dev(t, torch.float32, name)
    nbytes = int(getattr(_lib.lib(), stem + "_workspace_bytes")(b, n, k, layers))
    if _dev(workspace, torch.float32, "workspace").numel() * 4 < nbytes or nbytes <= 0:
        raise ValueError(f"workspace must hold {nbytes} bytes, got {workspace.numel() * 4}")
    grads = dict(x_in=torch.empty_like(x_in), w_in=torch.empty_like(w_in), lin_w=torch.empty_like(lin_w),
                 lin_b=torch.empty_like(lin_b), bn_w=torch.empty_like(bn_w), bn_b=torch.empty_like(bn_b))
    a.workspace_bytes = workspace.numel() * 4
    values.update(workspace=workspace, stats=stats, grad_x_out=grad_x_out, grad_w_out=grad_w_out,
                  **{"grad_" + key: t for key, t in grads.items()})
    _nargnn_train_launch(stem + "_backward", a, values, err, dev)
    return grads


def nargnn_train_forward(neighbors: Tensor, csr_ptr: Tensor, csr_src: Tensor, x_in: Tensor, w_in: Tensor, *, lin_w: Tensor,
                         lin_b: Tensor, bn_w: Tensor, bn_b: Tensor, eps: float = 1e-5, err: Tensor | None = None):
    """The L-layer GNN stack of the TSP heatmap encoder on BATCH statistics (rl4co_nargnn_train_forward), fp32.

    ``neighbors`` [B, N, K] int32, ``(csr_ptr, csr_src)`` from :func:`incoming_csr`, ``x_in`` [B, N, 64] and ``w_in``
    [B, N, K, 64] (the activated embeddings), ``lin_w`` [L, 5, 64, 64], ``lin_b`` [L, 5, 64], ``bn_w`` / ``bn_b`` [L, 2, 64]
    (gamma / beta of v_bn, e_bn). Returns ``(x_out, w_out, stats [L, 6, 64], workspace)``; ``stats[l]`` = (mu_v, r_v, var_v,
    mu_e, r_e, var_e), the variances biased. ``workspace`` holds what :func:`nargnn_train_backward` reads. Without ``err``
    the error word is read back and a bad neighbour list or CSR raises; the outputs are then not returned."""
    return _nargnn_train_forward("regular", neighbors, csr_ptr, csr_src, x_in, w_in, lin_w, lin_b, bn_w, bn_b, eps, err)


def nargnn_train_backward(neighbors: Tensor, csr_ptr: Tensor, csr_src: Tensor, x_in: Tensor, w_in: Tensor, *, lin_w: Tensor,
                          lin_b: Tensor, bn_w: Tensor, bn_b: Tensor, stats: Tensor, workspace: Tensor, grad_x_out: Tensor,
                          grad_w_out: Tensor, eps: float = 1e-5, err: Tensor | None = None) -> dict:
    """The backward of :func:`nargnn_train_forward` (rl4co_nargnn_train_backward) given its inputs, ``stats`` and
    ``workspace`` and the gradients of its two outputs. Returns the gradients by name: ``x_in``, ``w_in``, ``lin_w``,
    ``lin_b``, ``bn_w``, ``bn_b``."""
    return _nargnn_train_backward("regular", neighbors, csr_ptr, csr_src, x_in, w_in, lin_w, lin_b, bn_w, bn_b, stats, workspace,
                                  grad_x_out, grad_w_out, eps, err)


def nargnn_depot_train_workspace_bytes(b: int, n: int, k: int, layers: int) -> int:
    """Bytes of workspace the train-mode GNN stack needs on the depot graph (N with the depot; the formula is in
    include/rl4co_amd.h); 0 outside the served range."""
    return int(_lib.lib().rl4co_nargnn_depot_train_workspace_bytes(int(b), int(n), int(k), int(layers)))


def nargnn_depot_train_forward(neighbors: Tensor, csr_ptr: Tensor, csr_src: Tensor, x_in: Tensor, w_in: Tensor, *, lin_w: Tensor,
                               lin_b: Tensor, bn_w: Tensor, bn_b: Tensor, eps: float = 1e-5, err: Tensor | None = None):
    """:func:`nargnn_train_forward` on the depot graph of CVRP, OP and PCTSP (rl4co_nargnn_depot_train_forward).

    ``neighbors`` [B, N - 1, K] int32 with values in 1 .. N - 1, ``(csr_ptr, csr_src)`` from :func:`depot_incoming_csr`,
    ``x_in`` [B, N, 64] (node 0 the depot) and ``w_in`` [B, E, 64] over the E = (N - 1)(K + 2) edge rows in the reference's
    order (the kNN rows by source, every ``i -> 0``, every ``0 -> i``); the parameters and the return value as there, ``w_out``
    [B, E, 64]. A neighbour of 0 (the depot) is refused like one outside the instance."""
    return _nargnn_train_forward("depot", neighbors, csr_ptr, csr_src, x_in, w_in, lin_w, lin_b, bn_w, bn_b, eps, err)


def nargnn_depot_train_backward(neighbors: Tensor, csr_ptr: Tensor, csr_src: Tensor, x_in: Tensor, w_in: Tensor, *,
                                lin_w: Tensor, lin_b: Tensor, bn_w: Tensor, bn_b: Tensor, stats: Tensor, workspace: Tensor,
                                grad_x_out: Tensor, grad_w_out: Tensor, eps: float = 1e-5, err: Tensor | None = None) -> dict:
    """The backward of :func:`nargnn_depot_train_forward` (rl4co_nargnn_depot_train_backward); see
    :func:`nargnn_train_backward`."""
    return _nargnn_train_backward("depot", neighbors, csr_ptr, csr_src, x_in, w_in, lin_w, lin_b, bn_w, bn_b, stats, workspace,
                                  grad_x_out, grad_w_out, eps, err)


# ---- GFACS's log-partition head on the stack's edge state (csrc/nargnn_logz.hip) -------------------------------------------------
LOGZ_POOLING = {"reference": _lib.LOGZ_POOL_REFERENCE, "instance": _lib.LOGZ_POOL_INSTANCE}


def _nargnn_logz_args(w, W1, b1, W2, b2, batch, pooling):
    if pooling not in LOGZ_POOLING:
        raise ValueError(f"pooling must be one of {sorted(LOGZ_POOLING)}, got {pooling!r}")
    d = w.shape[-1]
    if d != 64:
        raise NotImplementedError(f"nargnn_logz serves embed_dim = 64 only, got {d}")
    z = W2.shape[0]
    if z not in (1, 2):
        raise NotImplementedError(f"nargnn_logz serves z_out_dim 1 or 2, got {z}")
    rows, batch = w.numel() // d, int(batch)
    if batch < 1 or rows < 1 or rows % batch:
        raise ValueError(f"w must hold B E >= 1 rows for B = {batch} >= 1, got {rows}")
    for name, t, shape in (("W1", W1, (d, d)), ("b1", b1, (d,)), ("W2", W2, (z, d)), ("b2", b2, (z,))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
    for name, t in (("w", w), ("W1", W1), ("b1", b1), ("W2", W2), ("b2", b2)):
        _dev(t, torch.float32, name)
    nbytes = int(_lib.lib().rl4co_nargnn_logz_workspace_bytes(rows))
    if nbytes <= 0:
        raise NotImplementedError(f"nargnn_logz does not serve {rows} rows (B E <= 2^24)")
    a = _lib.NargnnLogzArgs()
    a.B, a.E, a.Z, a.pooling, a.rows = batch, rows // batch, z, LOGZ_POOLING[pooling], rows
    a.workspace_bytes = nbytes
    values = dict(w=w, W1=W1, b1=b1, W2=W2, b2=b2, workspace=torch.empty(nbytes // 4, dtype=torch.float32, device=w.device))
    return a, values, z


def _nargnn_logz_launch(symbol: str, a, values: dict) -> None:
    for name, ctype in a._fields_:
        if ctype is C.c_void_p:
            setattr(a, name, _ptr(values.get(name)))
    _lib.check(getattr(_lib.lib(), symbol)(C.byref(a), _stream()), symbol)


def nargnn_logz_forward(w: Tensor, W1: Tensor, b1: Tensor, W2: Tensor, b2: Tensor, *, batch: int,
                        pooling: str = "reference") -> Tensor:
    """GFACS's log-partition head (gfacs/encoder.py:45-47, 62; rl4co_nargnn_logz_forward), fp32: ``w`` [..., 64] the GNN
    stack's edge state, flat and batch-major (``batch`` instances of E rows each), ``W1`` [64, 64], ``b1`` [64], ``W2``
    [Z, 64], ``b2`` [Z] the two linears of ``Z_net``, Z in {1, 2}. Returns ``logZ`` [B, Z]: the mean of the rows' scores over
    the rows r with ``r % B == b`` (``pooling="reference"``: the reference's reshape read literally) or over instance b's own
    rows (``"instance"``)."""
    a, values, z = _nargnn_logz_args(w, W1, b1, W2, b2, batch, pooling)
    values["logZ"] = torch.empty((a.B, z), dtype=torch.float32, device=w.device)
    _nargnn_logz_launch("rl4co_nargnn_logz_forward", a, values)
    return values["logZ"]


def nargnn_logz_backward(w: Tensor, W1: Tensor, b1: Tensor, W2: Tensor, b2: Tensor, grad_logz: Tensor, *, batch: int,
                         pooling: str = "reference") -> dict:
    """The backward of :func:`nargnn_logz_forward` (rl4co_nargnn_logz_backward) given its inputs and ``grad_logz`` [B, Z]; the
    hidden is recomputed. Returns the gradients by name: ``w``, ``W1``, ``b1``, ``W2``, ``b2``."""
    a, values, z = _nargnn_logz_args(w, W1, b1, W2, b2, batch, pooling)
    if tuple(grad_logz.shape) != (a.B, z):
        raise ValueError(f"grad_logz must be {(a.B, z)}, got {tuple(grad_logz.shape)}")
    grads = dict(w=torch.empty_like(w), W1=torch.empty_like(W1), b1=torch.empty_like(b1), W2=torch.empty_like(W2),
                 b2=torch.empty_like(b2))
    values.update(grad_logZ=_dev(grad_logz, torch.float32, "grad_logz"), **{"grad_" + key: t for key, t in grads.items()})
    _nargnn_logz_launch("rl4co_nargnn_logz_backward", a, values)
    return grads


# ---- the Ant System: one table of families, one launch path for the search, one for the backward ---------------------------
_ACO_PRIZE_ENVS = {"op": _lib.ENV_OP, "pctsp": _lib.ENV_PCTSP, "spctsp": _lib.ENV_PCTSP}  # spctsp: the caller's prize is the stochastic one
_ACO_DEPOT_GRAD_ENVS = {"cvrp": _lib.ENV_CVRP, **_ACO_PRIZE_ENVS}


def aco_cvrp_width(n: int) -> int:
    """W = max(C + 1, 2 C - 1), C = n - 1: the longest action row the reference's CVRP sampling loop can produce."""
    return max(n, 2 * n - 3)


def aco_depot_width(env: str, n: int) -> int:
    """The width of a sampled row: :func:`aco_cvrp_width` for cvrp, ``n`` for op / pctsp / spctsp."""
    return aco_cvrp_width(n) if env == "cvrp" else n


class AcoTensor(NamedTuple):
    """One fp32 instance tensor of a search binding. ``sample``: the SAMPLE phase needs it — always, never, or under these
    ``env`` values. ``flat``: taken as ``reshape(-1)`` ([B] or [B, 1])."""
    key: str
    shape: Callable[[int, int], tuple]  # of (b, n)
    text: str  # the shape as a message states it
    sample: bool | tuple[str, ...] = False
    flat: bool = False


class AcoFamily(NamedTuple):
    """One Ant System search kernel. The struct's field names are the binding's keywords and the returned dict's keys."""
    name: str  # the public binding
    symbol: str
    args: type
    envs: dict  # environment name -> RL4CO_ENV_*
    width: Callable[[int], int]  # of a sampled row
    lds_nodes: Callable[[int], int]  # of RL4CO_ENV_*: the *_lds_nodes query
    instance: tuple[AcoTensor, ...]
    ragged: bool  # depot graph: lengths / iter_lengths / final_iteration / T / iteration_base, zero-filled outputs
    start_nodes: bool
    scalars: tuple[str, ...]  # scalar struct fields beyond the shared ones
    cpu_refused: tuple[str, ...]  # tensors a NotImplementedError names before anything else is looked at (tsp: none)


_LOCS = AcoTensor("locs", lambda b, n: (b, n, 2), "[B, n, 2]")
ACO_FAMILIES = (
    AcoFamily("aco_tsp", "rl4co_aco_tsp", _lib.AcoTspArgs, {"tsp": _lib.ENV_TSP}, lambda n: n,
              lambda env: _lib.lib().rl4co_aco_tsp_lds_nodes(), (_LOCS,), False, True, (), ()),
    AcoFamily("aco_cvrp", "rl4co_aco_cvrp", _lib.AcoCvrpArgs, {"cvrp": _lib.ENV_CVRP}, aco_cvrp_width,
              lambda env: _lib.lib().rl4co_aco_cvrp_lds_nodes(),
              (_LOCS, AcoTensor("demand", lambda b, n: (b, n - 1), "[B, n - 1]", True),
               AcoTensor("vehicle_capacity", lambda b, n: (b,), "[B]", True, flat=True)),
              True, True, ("T", "iteration_base"), ("pheromone", "log_heuristic", "locs", "demand")),
    AcoFamily("aco_prize", "rl4co_aco_prize", _lib.AcoPrizeArgs, _ACO_PRIZE_ENVS, lambda n: n,
              lambda env: _lib.lib().rl4co_aco_prize_lds_nodes(env),
              (_LOCS._replace(sample=True), AcoTensor("prize", lambda b, n: (b, n), "[B, n]", True),
               AcoTensor("penalty", lambda b, n: (b, n), "[B, n]", ("pctsp", "spctsp")),
               AcoTensor("max_length", lambda b, n: (b, n), "[B, n]", ("op",))),
              True, False, ("T", "iteration_base", "env", "n_workgroups"),
              ("pheromone", "log_heuristic", "locs", "prize", "penalty", "max_length")),
)
# the environment's reset state -> the bindings' instance keywords: ((keyword, td key), ...); real_prize: the deterministic
# prize, or the stochastic one under SPCTSPEnv (the env's reset picked it)
ACO_TD_KEYS = {"tsp": (), "cvrp": (("demand", "demand"), ("vehicle_capacity", "vehicle_capacity")),
               "op": (("prize", "prize"), ("max_length", "max_length")),
               "pctsp": (("prize", "real_prize"), ("penalty", "penalty")),
               "spctsp": (("prize", "real_prize"), ("penalty", "penalty"))}


def aco_family(env: str) -> AcoFamily:
    return next(fam for fam in ACO_FAMILIES if env in fam.envs)


def heatmap_decode_opts(greedy, top_k, top_p, n: int):
    """``rl4co_heatmap_decode_opts`` of a decode over ``n`` nodes, ``top_k`` / ``top_p`` normalised by
    :func:`decoding_filter`; None when every option is off (the launch then goes to the symbol without ``_opts``)."""
    k, p = decoding_filter(top_k, top_p, n)
    if not (greedy or k or p):
        return None
    return _lib.HeatmapDecodeOpts(greedy=int(bool(greedy)), top_k=k, top_p=p, reserved0=0)


def aco_search(env: str, pheromone: Tensor, **kw) -> dict:
    """:func:`aco_tsp`, :func:`aco_cvrp` or :func:`aco_prize`, whichever serves ``env``. ``greedy=``, ``top_k=`` and
    ``top_p=`` (utils/decoding.py:109-188 at every step; ``greedy``: the argmax of the log-probs, no noise) go to the
    family's ``*_opts`` symbol when any of them is on, with the binding's own keywords and defaults."""
    fam = aco_family(env)
    binding = globals()[fam.name]
    opts = heatmap_decode_opts(kw.pop("greedy", False), kw.pop("top_k", 0), kw.pop("top_p", 0.0), pheromone.shape[-1])
    if "env" in fam.scalars:
        kw["env"] = env
    if opts is None:
        return binding(pheromone, **kw)
    bound = inspect.signature(binding).bind(pheromone, **kw)
    bound.apply_defaults()
    if opts.greedy and bound.arguments.get("ln_noise") is not None:
        raise ValueError("greedy reads no noise: ln_noise must be None")
    return _aco_search(fam, **{"env": env, **bound.arguments}, decode_opts=opts)


def _aco_launch(symbol: str, a, values: dict, err: Tensor | None, dev, opts=None) -> None:
    """Fill the struct ``a`` field by field from ``values`` (tensors as pointers, a pointer without a value NULL), launch and
    check. With ``err`` the sticky bits are OR-ed into the caller's word; without, the launch's own word is read back.
    ``opts``: a ``HeatmapDecodeOpts`` for ``symbol + "_opts"``."""
    own = err is None
    values["err"] = new_error_word(dev) if own else _dev(err, torch.int32, "err")
    for name, ctype in a._fields_:
        setattr(a, name, _ptr(values.get(name)) if ctype is C.c_void_p else values[name])
    if opts is None:
        st = getattr(_lib.lib(), symbol)(C.byref(a), _stream())
    else:
        symbol += "_opts"
        st = getattr(_lib.lib(), symbol)(C.byref(a), C.byref(opts), _stream())
    _lib.check(st, symbol)
    if own:
        raise_if_error(values["err"])


def _aco_search(fam: AcoFamily, pheromone, *, n_ants, phases, iterations, log_heuristic, alpha, beta, decay, Q, temperature,
                ln_noise, philox_seed, philox_offset, philox_seed_dev, forced_actions, actions, reward, final_reward,
                final_actions, has_best, all_logps, record_iterations, err, env, start_nodes=None, final_iteration=None,
                iteration_base=0, n_workgroups=0, decode_opts=None, **given) -> dict:
    """The one body of the three search bindings; ``given``: the family's instance tensors by keyword; ``decode_opts``:
    :func:`heatmap_decode_opts` (None: the symbol without them)."""
    who, d = fam.name, "n" if fam.ragged else "N"
    if env not in fam.envs:
        raise NotImplementedError(f"{who} ({fam.symbol}) serves {sorted(fam.envs)}, got env = {env!r}")
    for name in fam.cpu_refused:
        t = {"pheromone": pheromone, "log_heuristic": log_heuristic, **given}[name]
        if t is not None and not t.is_cuda:
            raise NotImplementedError(f"{who} runs inside the MI355X kernel ({fam.symbol}) only: {name} on {t.device}")
    pheromone = _dev(pheromone, torch.float32, "pheromone")
    if pheromone.dim() != 3 or pheromone.shape[1] != pheromone.shape[2]:
        raise ValueError(f"pheromone must be [B, {d}, {d}], got {tuple(pheromone.shape)}")
    b, n, _ = pheromone.shape
    if not 2 <= n <= 1024:
        raise NotImplementedError(f"{who} serves 2..1024 nodes{' (depot included)' if fam.ragged else ''}, got {d} = {n}")
    n_ants, iterations = int(n_ants), int(iterations)
    rows, w = n_ants * b, fam.width(n)
    dev = pheromone.device
    sample, update = bool(phases & _lib.ACO_SAMPLE), bool(phases & _lib.ACO_UPDATE)
    new = torch.zeros if fam.ragged else torch.empty  # a ragged row is zero-filled after its length

    def shaped(t, dtype, shape, name):
        if t is None:
            return None
        t = _dev(t, dtype, name)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be {tuple(shape)}, got {tuple(t.shape)}")
        return t

    log_heuristic = shaped(log_heuristic, torch.float32, (b, n, n), "log_heuristic")
    for it in fam.instance:
        t = given[it.key]
        given[it.key] = shaped(t.reshape(-1) if it.flat and t is not None else t, torch.float32, it.shape(b, n), it.key)
    if fam.start_nodes:
        start_nodes = shaped(start_nodes, torch.int64, (iterations, rows), "start_nodes")
    ln_noise = shaped(ln_noise, torch.float32, (iterations, w if fam.ragged else n - 1, rows, n), "ln_noise")
    forced_actions = shaped(forced_actions, torch.int64, (rows, w), "forced_actions")
    t = w
    if sample:
        if actions is not None or reward is not None:
            raise ValueError("actions / reward are outputs of the SAMPLE phase")
        needs = [it for it in fam.instance if it.sample is True or (it.sample and env in it.sample)]
        if any(given[it.key] is None for it in needs):
            texts = [f"{it.key} {it.text}" for it in needs]
            raise ValueError("the SAMPLE phase takes " + ", ".join(texts[:-1]) + " and " + texts[-1])
        actions = new((rows, w), dtype=torch.int64, device=dev)
        reward = torch.zeros(rows, dtype=torch.float32, device=dev)
    elif actions is None or reward is None:
        raise ValueError(f"the UPDATE phase alone takes actions [rows, {'T' if fam.ragged else 'N'}] and reward [rows]")
    elif fam.ragged:
        t = actions.shape[-1]
        if t < 2:
            raise ValueError(f"actions must be [rows, T] with T >= 2, got {tuple(actions.shape)}")
    actions = shaped(actions, torch.int64, (rows, t), "actions")
    reward = shaped(reward, torch.float32, (rows,), "reward")
    out = {"actions": actions, "reward": reward}
    if sample:
        if fam.ragged:
            out["lengths"] = torch.zeros(rows, dtype=torch.int32, device=dev)
        out["logps"] = new((rows, w), dtype=torch.float32, device=dev)
        if all_logps:
            out["all_logps"] = new((rows, w, n), dtype=torch.float32, device=dev)
        if record_iterations:
            out["iter_actions"] = new((iterations, rows, w), dtype=torch.int64, device=dev)
            if fam.ragged:
                out["iter_lengths"] = torch.zeros((iterations, rows), dtype=torch.int32, device=dev)
            out["iter_reward"] = torch.zeros((iterations, rows), dtype=torch.float32, device=dev)
    if update:
        if (final_reward is None) != (final_actions is None):
            raise ValueError("final_reward and final_actions come together")
        if final_reward is None:
            if has_best:
                raise ValueError("has_best needs final_reward and final_actions")
            final_reward = torch.zeros(b, dtype=torch.float32, device=dev)
            final_actions = torch.zeros((b, t), dtype=torch.int64, device=dev)
        out["final_reward"] = shaped(final_reward, torch.float32, (b,), "final_reward")
        out["final_actions"] = shaped(final_actions, torch.int64, (b, t), "final_actions")
        if fam.ragged:
            if final_iteration is None:
                final_iteration = torch.full((b,), -1, dtype=torch.int32, device=dev)
            out["final_iteration"] = shaped(final_iteration, torch.int32, (b,), "final_iteration")
        out["final_reward_cache"] = torch.zeros((iterations, b), dtype=torch.float32, device=dev)
    scratch = torch.empty((b, n, n), dtype=torch.float32, device=dev) if n > int(fam.lds_nodes(fam.envs[env])) else None
    extra = dict(T=t, iteration_base=int(iteration_base), env=fam.envs[env], n_workgroups=int(n_workgroups))
    values = dict(out, B=b, N=n, n_ants=n_ants, iterations=iterations, phases=int(phases), has_best=int(bool(has_best)),
                  alpha=alpha, beta=beta, decay=decay, Q=Q, temperature=temperature, reserved0=0,
                  philox_seed=int(philox_seed) & (2**64 - 1), philox_offset=int(philox_offset) & (2**64 - 1),
                  philox_seed_dev=philox_seed_dev, log_heuristic=log_heuristic, pheromone=pheromone, start_nodes=start_nodes,
                  ln_noise=ln_noise, forced_actions=forced_actions, logits_scratch=scratch, **given,
                  **{key: extra[key] for key in fam.scalars})
    _aco_launch(fam.symbol, fam.args(), values, err, dev, decode_opts)
    return out


def aco_lds_nodes() -> int:
    """Largest node count at which the Ant System kernel keeps logits and pheromone in LDS (a host query)."""
    return int(_lib.lib().rl4co_aco_tsp_lds_nodes())


def aco_cvrp_lds_nodes() -> int:
    """Largest node count (depot included) at which the CVRP Ant System kernel keeps logits and pheromone in LDS."""
    return int(_lib.lib().rl4co_aco_cvrp_lds_nodes())


def aco_prize_lds_nodes(env: str) -> int:
    """Largest node count (depot included) at which the OP / PCTSP Ant System kernel keeps logits and pheromone in LDS."""
    return int(_lib.lib().rl4co_aco_prize_lds_nodes(_ACO_PRIZE_ENVS[env]))


def aco_tsp(pheromone: Tensor, *, n_ants: int, phases: int = _lib.ACO_SAMPLE | _lib.ACO_UPDATE, iterations: int = 1,
            log_heuristic: Tensor | None = None, locs: Tensor | None = None, start_nodes: Tensor | None = None,
            alpha: float = 1.0, beta: float = 1.0, decay: float = 0.95, Q: float = 1.0, temperature: float = 1.0,
            ln_noise: Tensor | None = None, philox_seed: int = 0, philox_offset: int = 0,
            philox_seed_dev: Tensor | None = None, forced_actions: Tensor | None = None, actions: Tensor | None = None,
            reward: Tensor | None = None, final_reward: Tensor | None = None, final_actions: Tensor | None = None,
            has_best: bool = False, all_logps: bool = False, record_iterations: bool = False,
            err: Tensor | None = None) -> dict:
    """Ant System iterations on ``pheromone`` [B, N, N] (fp32, updated IN PLACE) in one launch (rl4co_aco_tsp; the header
    states the arithmetic). Rows are ant-major: row ``j * B + b`` is ant ``j`` of instance ``b``.

    ``phases``: SAMPLE | UPDATE runs ``iterations`` whole iterations; SAMPLE alone samples (or, with ``forced_actions``
    [rows, N], evaluates) once; UPDATE alone takes ``actions`` [rows, N] and ``reward`` [rows] and updates once.
    ``start_nodes`` int64 [iterations, rows]; ``ln_noise`` fp32 [iterations, N - 1, rows, N] (parity mode) or None for
    the in-kernel Philox. ``final_reward`` [B] / ``final_actions`` [B, N] are updated in place when given
    (``has_best``: they hold a record already), else created. Returns a dict of the tensors the launch wrote:
    actions, reward, logps, final_reward, final_actions, final_reward_cache [iterations, B] and, on request, all_logps
    [rows, N, N], iter_actions [iterations, rows, N], iter_reward [iterations, rows]. With ``err`` the sticky bits are
    OR-ed into the caller's word and nothing is synchronised; without it the word is read back and a set bit raises."""
    return _aco_search(ACO_FAMILIES[0], env="tsp", **locals())  # (locals(): the arguments as they came)


def aco_cvrp(pheromone: Tensor, *, n_ants: int, phases: int = _lib.ACO_SAMPLE | _lib.ACO_UPDATE, iterations: int = 1,
             log_heuristic: Tensor | None = None, locs: Tensor | None = None, demand: Tensor | None = None,
             vehicle_capacity: Tensor | None = None, start_nodes: Tensor | None = None,
             alpha: float = 1.0, beta: float = 1.0, decay: float = 0.95, Q: float = 1.0, temperature: float = 1.0,
             ln_noise: Tensor | None = None, philox_seed: int = 0, philox_offset: int = 0,
             philox_seed_dev: Tensor | None = None, forced_actions: Tensor | None = None, actions: Tensor | None = None,
             reward: Tensor | None = None, final_reward: Tensor | None = None, final_actions: Tensor | None = None,
             final_iteration: Tensor | None = None, has_best: bool = False, iteration_base: int = 0,
             all_logps: bool = False, record_iterations: bool = False, err: Tensor | None = None) -> dict:
    """Ant System iterations for CVRP on ``pheromone`` [B, n, n] (fp32, the depot is node 0, updated IN PLACE) in one
    launch (rl4co_aco_cvrp; the header states the arithmetic). Rows are ant-major as in :func:`aco_tsp`; sampled rows are
    ``W = aco_cvrp_width(n)`` wide, zero-filled after ``lengths[row]``.

    ``locs`` [B, n, 2] with the depot at 0, ``demand`` [B, n - 1], ``vehicle_capacity`` [B] or [B, 1]. ``start_nodes``
    int64 [iterations, rows] of customers (multistart) or None (multisample: every ant starts at the depot).
    ``ln_noise`` fp32 [iterations, W, rows, n] (parity mode) or None for the in-kernel Philox. SAMPLE alone samples (or,
    with ``forced_actions`` [rows, W], evaluates) once; UPDATE alone takes ``actions`` [rows, T] of any width T >= 2 and
    ``reward`` [rows]. The reward is the one of the W-wide padded row (``CVRPEnv.get_reward`` on it, bit for bit).
    ``final_reward`` [B] / ``final_actions`` [B, T] / ``final_iteration`` [B] (int32, ``iteration_base + it`` of the last
    replacement, -1 where none happened) are updated in place when given, else created. Returns a dict of the tensors the
    launch wrote: actions, lengths, reward, logps, final_reward, final_actions, final_iteration, final_reward_cache
    [iterations, B] and, on request, all_logps [rows, W, n], iter_actions [iterations, rows, W], iter_lengths and
    iter_reward [iterations, rows]. ``err`` as in :func:`aco_tsp`."""
    return _aco_search(ACO_FAMILIES[1], env="cvrp", **locals())


def aco_prize(pheromone: Tensor, *, env: str, n_ants: int, phases: int = _lib.ACO_SAMPLE | _lib.ACO_UPDATE,
              iterations: int = 1, log_heuristic: Tensor | None = None, locs: Tensor | None = None,
              prize: Tensor | None = None, penalty: Tensor | None = None, max_length: Tensor | None = None,
              alpha: float = 1.0, beta: float = 1.0, decay: float = 0.95, Q: float = 1.0, temperature: float = 1.0,
              ln_noise: Tensor | None = None, philox_seed: int = 0, philox_offset: int = 0,
              philox_seed_dev: Tensor | None = None, forced_actions: Tensor | None = None, actions: Tensor | None = None,
              reward: Tensor | None = None, final_reward: Tensor | None = None, final_actions: Tensor | None = None,
              final_iteration: Tensor | None = None, has_best: bool = False, iteration_base: int = 0,
              all_logps: bool = False, record_iterations: bool = False, n_workgroups: int = 0,
              err: Tensor | None = None) -> dict:
    """Ant System iterations for the prize problems (``env``: "op", "pctsp" or "spctsp") on ``pheromone`` [B, n, n] (fp32, the
    depot is node 0, updated IN PLACE) in one launch (rl4co_aco_prize; the header states the arithmetic). Rows are
    ant-major as in :func:`aco_tsp`; sampled rows are ``W = n`` wide, zero-filled after ``lengths[row]``.

    ``locs`` [B, n, 2] with the depot at 0; ``prize`` [B, n] with 0 at the depot (OP: ``td["prize"]``; PCTSP:
    ``td["real_prize"]``); ``penalty`` [B, n] (PCTSP); ``max_length`` [B, n], the environment's per-node table (OP).
    ``ln_noise`` fp32 [iterations, W, rows, n] (parity mode) or None for the in-kernel Philox. SAMPLE alone samples (or,
    with ``forced_actions`` [rows, W], evaluates) once; UPDATE alone takes ``actions`` [rows, T] of any width T >= 2 and
    ``reward`` [rows]. The reward is the environment's ``get_reward`` on the W-wide row. ``n_workgroups``: 0 for one
    workgroup per instance, else that many workgroups striding over the instances (the same results). The record
    arguments, the returned dict and ``err`` are :func:`aco_cvrp`'s."""
    return _aco_search(ACO_FAMILIES[2], **locals())


class AcoGradFamily(NamedTuple):
    """One backward kernel of the ants' log-likelihoods. ``needs``: environment -> the instance tensors it takes as
    ``(keyword, shape of (b, n))``; ``scratch``: the struct's pointer for the table kept outside LDS, and what to allocate
    for ``parts`` workgroups."""
    name: str
    symbol: str
    args: type
    envs: dict
    depot: bool  # node 0 is the depot: the binding takes ``env`` and instance tensors
    width: Callable[[str, int], int]
    lds_entries: Callable[[], int]
    scratch: tuple[str, Callable]  # (struct field, (parts, n_ants, n, device) -> Tensor)
    needs: dict


def aco_grad_lds_entries() -> int:
    """Largest ``n_ants * N`` whose inverse-permutation table the log-likelihood backward keeps in LDS (a host query)."""
    return int(_lib.lib().rl4co_aco_tsp_grad_lds_entries())


def aco_depot_grad_lds_entries() -> int:
    """Largest ``n_ants * N`` whose replay table the depot-graph log-likelihood backward keeps in LDS (a host query)."""
    return int(_lib.lib().rl4co_aco_depot_grad_lds_entries())


def aco_grad_row_split(b: int, n: int, cus: int) -> int:
    """Workgroups per instance of :func:`aco_tsp_logp_grad` when the caller names none: about two workgroups per CU, at
    least sixteen heatmap rows per workgroup (each repeats the table build). An estimate, not a measured optimum."""
    return max(1, min(n // 16, (2 * cus) // b))


_PRIZE_NEEDS = (("prize", lambda b, n: (b, n)),)
ACO_GRAD_FAMILIES = (
    AcoGradFamily("aco_tsp_logp_grad", "rl4co_aco_tsp_logp_grad", _lib.AcoTspGradArgs, {"tsp": _lib.ENV_TSP},
                  False, lambda env, n: n, aco_grad_lds_entries,
                  ("pos_scratch",
                   lambda parts, ants, n, dev: torch.empty((parts, ants, n), dtype=torch.int16, device=dev)), {"tsp": ()}),
    AcoGradFamily("aco_depot_logp_grad", "rl4co_aco_depot_logp_grad", _lib.AcoDepotGradArgs, _ACO_DEPOT_GRAD_ENVS,
                  True, aco_depot_width, aco_depot_grad_lds_entries,
                  ("scratch", lambda parts, ants, n, dev: torch.empty(
                      parts * int(_lib.lib().rl4co_aco_depot_grad_scratch_bytes(ants, n)), dtype=torch.uint8, device=dev)),
                  {"cvrp": (("demand", lambda b, n: (b, n - 1)), ("vehicle_capacity", lambda b, n: (b,))),
                   "op": (("locs", lambda b, n: (b, n, 2)), ("max_length", lambda b, n: (b, n))),
                   "pctsp": _PRIZE_NEEDS, "spctsp": _PRIZE_NEEDS}),
)


def aco_grad_family(env: str) -> AcoGradFamily:
    return next(fam for fam in ACO_GRAD_FAMILIES if env in fam.envs)


def aco_logp_grad(env: str, heatmap: Tensor, actions: Tensor, grad_ll: Tensor, **kw) -> Tensor:
    """:func:`aco_tsp_logp_grad` or :func:`aco_depot_logp_grad`, whichever serves ``env``. ``top_k=`` / ``top_p=``: the
    forward's filter — each contribution runs over its step's kept set, removed nodes get 0 (the family's ``*_opts``
    symbol); ``greedy=`` is accepted and changes nothing (it is the forward's selector)."""
    fam = aco_grad_family(env)
    binding = globals()[fam.name]
    kw.pop("greedy", None)
    opts = heatmap_decode_opts(False, kw.pop("top_k", 0), kw.pop("top_p", 0.0), heatmap.shape[-1])
    if fam.depot:
        kw["env"] = env
    if opts is None:
        return binding(heatmap, actions, grad_ll, **kw)
    bound = inspect.signature(binding).bind(heatmap, actions, grad_ll, **kw)
    bound.apply_defaults()
    args = {"env": env, **bound.arguments}
    args["in_scratch"] = args.pop("table_in_scratch" if fam.depot else "pos_in_scratch")
    return _aco_logp_grad(fam, **args, decode_opts=opts)


def _aco_logp_grad(fam: AcoGradFamily, heatmap, actions, grad_ll, *, env, grad_steps, temperature, row_split, in_scratch, err,
                   multistart=False, decode_opts=None, **given) -> Tensor:
    """The one body of the two gradient bindings; ``given``: the instance tensors by keyword; ``decode_opts``:
    :func:`heatmap_decode_opts` (None: the symbol without them)."""
    who, depot = fam.name, fam.depot
    d, wd = ("n", "W") if depot else ("N", "N")
    if env not in fam.envs:
        raise NotImplementedError(f"{who} ({fam.symbol}) serves {sorted(fam.envs)}, got env = {env!r}")
    for name, t, dtype in (("heatmap", heatmap, torch.float32), ("actions", actions, torch.int64),
                           ("grad_ll", grad_ll, torch.float32), ("grad_steps", grad_steps, torch.float32),
                           *((name, t, torch.float32) for name, t in given.items())):
        if t is not None and t.dtype != dtype:
            raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if heatmap.dim() != 3 or heatmap.shape[1] != heatmap.shape[2]:
        raise ValueError(f"heatmap must be [B, {d}, {d}], got {tuple(heatmap.shape)}")
    b, n, _ = heatmap.shape
    if not 2 <= n <= 1024:
        raise NotImplementedError(f"{who} serves 2..1024 nodes{' (depot included)' if depot else ''}, got {d} = {n}")
    w = fam.width(env, n)
    if actions.dim() != 2 or actions.shape[1] != w or actions.shape[0] == 0 or actions.shape[0] % b:
        raise ValueError(f"actions must be [n_ants * B, {wd}] = [k * {b}, {w}], got {tuple(actions.shape)}")
    rows = actions.shape[0]
    n_ants = rows // b
    if tuple(grad_ll.shape) != (rows,):
        raise ValueError(f"grad_ll must be {(rows,)}, got {tuple(grad_ll.shape)}")
    if grad_steps is not None and tuple(grad_steps.shape) != (rows, w):
        raise ValueError(f"grad_steps must be {(rows, w)}, got {tuple(grad_steps.shape)}")
    if given.get("vehicle_capacity") is not None:
        given["vehicle_capacity"] = given["vehicle_capacity"].reshape(-1)
    needs = {name: given[name] for name, _ in fam.needs[env]}
    for name, shape in fam.needs[env]:
        if needs[name] is None or tuple(needs[name].shape) != shape(b, n):
            raise ValueError(f"env {env!r} takes {name} {shape(b, n)}, got "
                             f"{None if needs[name] is None else tuple(needs[name].shape)}")
    if multistart and env != "cvrp":
        raise NotImplementedError(f"multistart is served for cvrp only, got env = {env!r}")
    if not temperature > 0:
        raise ValueError(f"temperature must be positive, got {temperature}")
    if row_split is not None and not 1 <= int(row_split) <= n:
        raise ValueError(f"row_split must be in [1, {d} = {n}], got {row_split}")
    for name, t in (("heatmap", heatmap), ("actions", actions), ("grad_ll", grad_ll), ("grad_steps", grad_steps), *needs.items()):
        if t is not None:
            _dev(t, None, name)
    dev = heatmap.device
    if row_split is None:
        row_split = aco_grad_row_split(b, n, torch.cuda.get_device_properties(dev).multi_processor_count)
    fits = n_ants * n <= fam.lds_entries()
    field, alloc = fam.scratch
    if in_scratch is None:
        in_scratch = not fits
    elif not in_scratch and not fits:
        raise ValueError(f"n_ants * {d} = {n_ants * n} is above the LDS table's {fam.lds_entries()} entries")
    grad = torch.empty((b, n, n), dtype=torch.float32, device=dev)
    values = dict(needs, env=fam.envs[env], B=b, N=n, n_ants=n_ants, row_split=int(row_split), multistart=int(bool(multistart)),
                  temperature=float(temperature), reserved0=0, heatmap=heatmap, actions=actions, grad_ll=grad_ll,
                  grad_steps=grad_steps, grad_heatmap=grad)
    values[field] = alloc(b * int(row_split), n_ants, n, dev) if in_scratch else None
    _aco_launch(fam.symbol, fam.args(), values, err, dev, decode_opts)
    return grad


def aco_tsp_logp_grad(heatmap: Tensor, actions: Tensor, grad_ll: Tensor, *, grad_steps: Tensor | None = None,
                      temperature: float = 1.0, row_split: int | None = None, pos_in_scratch: bool | None = None,
                      err: Tensor | None = None) -> Tensor:
    """The gradient of the ants' log-likelihoods with respect to the heatmap in one launch (rl4co_aco_tsp_logp_grad; the
    header states the arithmetic): ``heatmap`` [B, N, N] fp32 (the logits the forward sampled from, not divided by the
    temperature), ``actions`` [rows, N] int64 with rows = n_ants * B ant-major, ``grad_ll`` [rows] fp32 and optionally
    ``grad_steps`` [rows, N] fp32 (column 0 ignored) -> ``grad_heatmap`` [B, N, N] fp32, every word written.

    ``row_split``: workgroups per instance (None: :func:`aco_grad_row_split`); any value gives the same bits.
    ``pos_in_scratch``: keep the inverse-permutation table in a global scratch instead of LDS (None: only above
    :func:`aco_grad_lds_entries`). ``err`` as in :func:`aco_tsp`."""
    return _aco_logp_grad(ACO_GRAD_FAMILIES[0], heatmap, actions, grad_ll, env="tsp", grad_steps=grad_steps,
                          temperature=temperature, row_split=row_split, in_scratch=pos_in_scratch, err=err)


def aco_depot_logp_grad(heatmap: Tensor, actions: Tensor, grad_ll: Tensor, *, env: str, grad_steps: Tensor | None = None,
                        locs: Tensor | None = None, demand: Tensor | None = None, vehicle_capacity: Tensor | None = None,
                        prize: Tensor | None = None, max_length: Tensor | None = None, multistart: bool = False,
                        temperature: float = 1.0, row_split: int | None = None, table_in_scratch: bool | None = None,
                        err: Tensor | None = None) -> Tensor:
    """The gradient of the ants' log-likelihoods with respect to the heatmap on a depot graph in one launch
    (rl4co_aco_depot_logp_grad; the header states the arithmetic). ``env``: "cvrp", "op", "pctsp" or "spctsp"; ``heatmap``
    [B, n, n] fp32 (the depot is node 0; the logits the forward sampled from, not divided by the temperature), ``actions``
    [rows, W] int64 as :func:`aco_cvrp` / :func:`aco_prize` write them (W = :func:`aco_depot_width`, rows = n_ants * B
    ant-major, zero-filled after each row's length), ``grad_ll`` [rows] fp32 and optionally ``grad_steps`` [rows, W] fp32
    -> ``grad_heatmap`` [B, n, n] fp32, every word written.

    The instance: cvrp ``demand`` [B, n - 1] and ``vehicle_capacity`` [B] or [B, 1]; op ``locs`` [B, n, 2] and ``max_length``
    [B, n]; pctsp / spctsp ``prize`` [B, n] (the prize the forward stepped with). ``multistart`` (cvrp): column 0 is a given
    customer and contributes nothing. ``row_split``: workgroups per instance (None: :func:`aco_grad_row_split`); any value
    gives the same bits. ``table_in_scratch``: keep the replay table in a global scratch instead of LDS (None: only above
    :func:`aco_depot_grad_lds_entries`); the same bits. ``err`` as in :func:`aco_tsp`."""
    return _aco_logp_grad(ACO_GRAD_FAMILIES[1], heatmap, actions, grad_ll, env=env, grad_steps=grad_steps, locs=locs,
                          demand=demand, vehicle_capacity=vehicle_capacity, prize=prize, max_length=max_length,
                          multistart=multistart, temperature=temperature, row_split=row_split, in_scratch=table_in_scratch,
                          err=err)


def decoding_filter(top_k, top_p, n: int) -> tuple[int, float]:
    """The top-k / top-p arguments of utils/decoding.py:109-188 as the kernel takes them: ``top_k <= 0`` is off and is
    clamped to ``n`` (k >= n removes nothing: 0); ``top_p <= 0`` or ``>= 1`` is off (0.0); ``top_p > 1`` raises the
    reference's AssertionError (decoding.py:147)."""
    k = int(top_k or 0)
    p = float(top_p or 0.0)
    assert p <= 1.0, "top-p should be in (0, 1]."
    k = min(k, n) if k > 0 else 0
    if k >= n:
        k = 0
    if not (0.0 < p < 1.0):
        p = 0.0
    return k, p


def op_max_length(locs: Tensor, max_length: Tensor) -> Tensor:
    """op/env.py:118-122: table[b,j] = (max_length[b] - |loc_0 - loc_j|) - 1e-6 (locs include the depot)."""
    b, n, _ = locs.shape
    locs = _dev(locs, torch.float32, "locs")
    ml = _dev(max_length.reshape(-1).contiguous(), torch.float32, "max_length")
    out = torch.empty((b, n), dtype=torch.float32, device=locs.device)
    st = _lib.lib().rl4co_op_max_length(_ptr(locs), _ptr(ml), b, n, _ptr(out), _stream())
    _lib.check(st, "rl4co_op_max_length")
    return out


def op_step(action: Tensor | None, locs: Tensor, max_length: Tensor, tour_length: Tensor, visited: Tensor,
            current_node: Tensor, step_i: Tensor, action_mask: Tensor, done: Tensor, err: Tensor | None = None) -> None:
    """In-place OPEnv._step + get_action_mask (op/env.py:67-98,137-154); action=None -> mask only."""
    b, n = action_mask.shape
    _check_rows(b, action=action, tour_length=tour_length, visited=visited, current_node=current_node, i=step_i, done=done)
    st = _lib.lib().rl4co_op_step(
        _ptr(None if action is None else _dev(action, torch.int64, "action")), _ptr(_dev(locs, torch.float32, "locs")),
        _ptr(_dev(max_length, torch.float32, "max_length")), _ptr(_dev(tour_length, torch.float32, "tour_length")),
        _ptr(_u8(visited, "visited")), _ptr(_dev(current_node, torch.int64, "current_node")),
        _ptr(_dev(step_i, torch.int64, "i")), _ptr(_u8(action_mask, "action_mask")), _ptr(_u8(done, "done")),
        b, locs.shape[0], n, _ptr(err), _stream())
    _lib.check(st, "rl4co_op_step")


def cvrptw_step(action: Tensor | None, demand: Tensor, locs: Tensor, time_windows: Tensor, durations: Tensor,
                used_capacity: Tensor, vehicle_capacity: Tensor, current_time: Tensor, visited: Tensor, current_node: Tensor,
                action_mask: Tensor, done: Tensor | None, err: Tensor | None = None) -> None:
    """In-place CVRPTWEnv._step + get_action_mask (cvrptw/env.py:83-113); action=None -> mask only.
    ``time_windows`` [B_inst,N,2] and ``durations`` [B_inst,N] are fp32 (the reference's integer windows cast)."""
    b, n = action_mask.shape
    _check_rows(b, action=action, used_capacity=used_capacity, vehicle_capacity=vehicle_capacity, current_time=current_time,
                visited=visited, current_node=current_node, done=done)
    st = _lib.lib().rl4co_cvrptw_step(
        _ptr(None if action is None else _dev(action, torch.int64, "action")), _ptr(_dev(demand, torch.float32, "demand")),
        _ptr(_dev(locs, torch.float32, "locs")), _ptr(_dev(time_windows, torch.float32, "time_windows")),
        _ptr(_dev(durations, torch.float32, "durations")), _ptr(_dev(used_capacity, torch.float32, "used_capacity")),
        _ptr(_dev(vehicle_capacity, torch.float32, "vehicle_capacity")), _ptr(_dev(current_time, torch.float32, "current_time")),
        _ptr(_u8(visited, "visited")), _ptr(_dev(current_node, torch.int64, "current_node")),
        _ptr(_u8(action_mask, "action_mask")), _ptr(None if done is None else _u8(done, "done")),
        b, demand.shape[0], n, _ptr(err), _stream())
    _lib.check(st, "rl4co_cvrptw_step")


def cvrptw_check_solution(actions: Tensor, locs: Tensor, time_windows: Tensor, durations: Tensor, err: Tensor) -> None:
    """cvrptw/env.py:151-190 (the part on top of the CVRP check) into the sticky error word."""
    b, t = actions.shape
    st = _lib.lib().rl4co_cvrptw_check_solution(
        _ptr(_dev(actions, torch.int64, "actions")), _ptr(_dev(locs, torch.float32, "locs")),
        _ptr(_dev(time_windows, torch.float32, "time_windows")), _ptr(_dev(durations, torch.float32, "durations")),
        b, locs.shape[0], locs.shape[1], t, _ptr(_dev(err, torch.int32, "err")), _stream())
    _lib.check(st, "rl4co_cvrptw_check_solution")


def pdp_step(action: Tensor | None, available: Tensor, to_deliver: Tensor, current_node: Tensor, step_i: Tensor,
             action_mask: Tensor, done: Tensor, err: Tensor | None = None) -> None:
    """In-place PDPEnv._step (pdp/env.py:64-99); action=None -> mask = available & to_deliver only."""
    b, n = action_mask.shape
    _check_rows(b, action=action, available=available, to_deliver=to_deliver, current_node=current_node, i=step_i, done=done)
    st = _lib.lib().rl4co_pdp_step(
        _ptr(None if action is None else _dev(action, torch.int64, "action")), _ptr(_u8(available, "available")),
        _ptr(_u8(to_deliver, "to_deliver")), _ptr(_dev(current_node, torch.int64, "current_node")),
        _ptr(_dev(step_i, torch.int64, "i")), _ptr(_u8(action_mask, "action_mask")), _ptr(_u8(done, "done")),
        b, n, _ptr(err), _stream())
    _lib.check(st, "rl4co_pdp_step")


def env_replay(env_name: str, state: dict, actions: Tensor, rem_base: Tensor | None, err: Tensor | None = None,
               mask_bits: bool = False) -> dict:
    """``T`` environment transitions of the given trajectories in ONE launch (``rl4co_env_replay``): the state tensors of
    ``policy._initial_state`` are stepped in place with ``actions[:, t]`` exactly as ``T`` calls of the env's step entry
    would, and what the decoder saw BEFORE each step is tabulated — ``masks`` [B,T,N] bool, ``prev`` [B,T] and, by
    environment, ``first`` / ``use_placeholder`` (TSP), ``rem`` (the context scalar: ``rem_base`` minus the running
    capacity / length / prize), ``now`` (CVRPTW), ``mask_bits`` [B,T,W] int32 on request. The `evaluate` decoding's state
    sequence (decoding.py:448-461)."""
    sp = spec(env_name)
    if not sp.replay:
        served = sorted(name for name, s in SPECS.items() if s.replay)
        raise NotImplementedError(f"the one-launch replay (rl4co_env_replay) serves {served}, not {sp.name}: use "
                                  "env_replay_stepwise")
    b, n = state["action_mask"].shape
    acts = _dev(actions, torch.int64, "actions")
    if acts.dim() != 2 or acts.shape[0] != b:
        raise ValueError(f"actions must be [B = {b}, T], got {tuple(acts.shape)}")
    t_len = acts.shape[1]
    dev = acts.device
    a = _lib.EnvReplayArgs()
    a.env, a.B, a.N, a.T = sp.env_id, b, n, t_len
    out = _replay_tables(sp, b, t_len, n, dev)
    if mask_bits:  # the same masks as bits, rows padded to whole 128-key chunks (train_ops.glimpse_attention's mask)
        a.mask_words = 4 * ((n + 127) // 128)
        out["mask_bits"] = torch.empty((b, t_len, a.mask_words), dtype=torch.int32, device=dev)
    if sp.scalar is not None:
        if rem_base is None:
            raise ValueError(f"{env_name}: rem_base (the context scalar's minuend, one per trajectory) is required")
        base = _dev(rem_base, torch.float32, "rem_base")
        _check_rows(b, rem_base=base)
        a.rem_base = base.data_ptr()
    a.B_inst = bind_env_state(a, sp, state, b, n)
    a.actions, a.err = acts.data_ptr(), _ptr(err)
    for k, t in out.items():  # (the output slots carry the names of the tables)
        setattr(a, k, t.data_ptr())
    st = _lib.lib().rl4co_env_replay(C.byref(a), _stream())
    _lib.check(st, "rl4co_env_replay")
    return out


def _replay_tables(sp: EnvSpec, b: int, t_len: int, n: int, dev) -> dict:
    """The tables a replay fills, by the environment's context layout (envspec.py)."""
    def new(dtype, *tail):
        return torch.empty((b, t_len, *tail), dtype=dtype, device=dev)

    out = {"masks": new(torch.bool, n), "prev": new(torch.int64)}
    if sp.ctx_first:
        out["first"], out["use_placeholder"] = new(torch.int64), new(torch.bool)
    if sp.scalar is not None:
        out["rem"] = new(torch.float32)
        if sp.scalar.clock:
            out["now"] = new(torch.float32)
    if sp.feats is not None:
        out["feats"] = new(torch.float32, len(sp.feats.names))
    return out


def context_features(sp: EnvSpec, state: dict) -> Tensor:
    """The running scalars of ``sp.feats`` from a state, [B, len(names)] fp32 in the layer's column order
    (env_embeddings/context.py:265-280). For the training re-evaluation: "depot_distance" is torch's ``norm`` on the
    state's device, as the reference computes it there — NOT bound to the decode kernels' ``sqrt(fma(dy, dy, dx * dx))``
    (the last bit may differ on the GPU; the re-evaluated log-probs are compared under a tolerance, never bit for bit)."""
    b = state["current_node"].shape[0]
    inst = lambda x: x if x.shape[0] == b else x.repeat(b // x.shape[0], *([1] * (x.dim() - 1)))  # noqa: E731
    cols = []
    for name in sp.feats.names:
        if name == "remaining_agents":
            cols.append((inst(state["num_agents"]) - state["agent_idx"]).float())
        elif name == "depot_distance":
            locs = inst(state["locs"])
            here = locs.gather(1, state["current_node"].view(b, 1, 1).expand(b, 1, 2))[:, 0]
            cols.append((here - locs[:, 0]).norm(p=2, dim=-1))
        else:
            cols.append(state[name].float())
    return torch.stack(cols, -1)


def env_replay_stepwise(env_name: str, state: dict, actions: Tensor, rem_base: Tensor | None, err: Tensor | None = None,
                        mask_bits: bool = False, record: str | None = None) -> dict:
    """``env_replay``'s tables from ``T`` calls of the step entry, tabulated in between (what the kernel loops on the
    device): the tests' cross-check of the one-launch form, and its stand-in where a test plays the device."""
    assert not mask_bits, "the mask bits come from the one-launch form only"
    sp = spec(env_name)
    b, t_len = actions.shape
    out = _replay_tables(sp, b, t_len, state["action_mask"].shape[1], actions.device)
    err = new_error_word(actions.device) if err is None else err
    if record is not None:  # a state tensor the decoder read besides the context (SDVRP: the remaining demands)
        out[record] = torch.empty((b, t_len, *state[record].shape[1:]), dtype=state[record].dtype, device=actions.device)
    for t in range(t_len):
        if record is not None:
            out[record][:, t] = state[record]
        out["masks"][:, t] = state["action_mask"]
        out["prev"][:, t] = state["current_node"]
        if sp.ctx_first:
            out["first"][:, t] = state["first_node"]
            out["use_placeholder"][:, t] = state["i"] < 1
        if sp.scalar is not None:
            rem = rem_base - state[sp.scalar.running]
            out["rem"][:, t] = torch.clamp(rem, min=0) if sp.scalar.clamp else rem
            if sp.scalar.clock:
                out["now"][:, t] = state[sp.scalar.clock]
        if sp.feats is not None:
            out["feats"][:, t] = context_features(sp, state)
        env_step(env_name, state, actions[:, t].contiguous(), err)
    return out


def pdp_check_solution(actions: Tensor, num_nodes: int, force_start_at_depot: bool, err: Tensor) -> None:
    """pdp/env.py:204-223 into the sticky error word (NOT_ALL_NODES / DEPOT_MIDDLE / NO_PICKUP)."""
    b, t = actions.shape
    st = _lib.lib().rl4co_pdp_check_solution(_ptr(_dev(actions, torch.int64, "actions")), b, num_nodes, t,
                                             int(force_start_at_depot), _ptr(_dev(err, torch.int32, "err")), _stream())
    _lib.check(st, "rl4co_pdp_check_solution")


def pctsp_step(action: Tensor | None, real_prize: Tensor, cur_total_prize: Tensor, visited: Tensor, current_node: Tensor,
               step_i: Tensor, action_mask: Tensor, done: Tensor, err: Tensor | None = None) -> None:
    """In-place PCTSPEnv._step + get_action_mask (pctsp/env.py:62-91,141-148); action=None -> mask only.
    ``real_prize`` [B_inst, N] carries 0 in the depot column."""
    b, n = action_mask.shape
    _check_rows(b, action=action, cur_total_prize=cur_total_prize, visited=visited, current_node=current_node, i=step_i,
                done=done)
    st = _lib.lib().rl4co_pctsp_step(
        _ptr(None if action is None else _dev(action, torch.int64, "action")),
        _ptr(_dev(real_prize, torch.float32, "real_prize")), _ptr(_dev(cur_total_prize, torch.float32, "cur_total_prize")),
        _ptr(_u8(visited, "visited")), _ptr(_dev(current_node, torch.int64, "current_node")),
        _ptr(_dev(step_i, torch.int64, "i")), _ptr(_u8(action_mask, "action_mask")), _ptr(_u8(done, "done")),
        b, real_prize.shape[0], n, _ptr(err), _stream())
    _lib.check(st, "rl4co_pctsp_step")


def pctsp_check_solution(actions: Tensor, real_prize: Tensor, err: Tensor) -> None:
    """pctsp/env.py:175-201 into the sticky error word (RL4CO_EBIT_DUPLICATES / RL4CO_EBIT_PRIZE)."""
    b, t = actions.shape
    prize_sum = gather_sum(real_prize, actions)
    st = _lib.lib().rl4co_pctsp_check_solution(_ptr(_dev(actions, torch.int64, "actions")), _ptr(prize_sum), b,
                                               real_prize.shape[1], t, _ptr(_dev(err, torch.int32, "err")), _stream())
    _lib.check(st, "rl4co_pctsp_check_solution")


def gather_sum(values: Tensor, actions: Tensor) -> Tensor:
    """out[b] = sum_t values[b % B_values, actions[b, t]] in ATen's inner-dim sum order (op/env.py:156-166)."""
    b, t = actions.shape
    values = _dev(values, torch.float32, "values")
    out = torch.empty((b,), dtype=torch.float32, device=actions.device)
    st = _lib.lib().rl4co_gather_sum_f32(_ptr(values), _ptr(_dev(actions, torch.int64, "actions")), b, values.shape[0],
                                         values.shape[1], t, _ptr(out), _stream())
    _lib.check(st, "rl4co_gather_sum_f32")
    return out


def op_check_solution(actions: Tensor, locs: Tensor, max_length: Tensor, err: Tensor) -> None:
    """op/env.py:168-194 into the sticky error word (RL4CO_EBIT_DUPLICATES / RL4CO_EBIT_MAX_LENGTH)."""
    b, t = actions.shape
    st = _lib.lib().rl4co_op_check_solution(_ptr(_dev(actions, torch.int64, "actions")), _ptr(_dev(locs, torch.float32, "locs")),
                                            _ptr(_dev(max_length, torch.float32, "max_length")), b, locs.shape[0],
                                            locs.shape[1], t, _ptr(_dev(err, torch.int32, "err")), _stream())
    _lib.check(st, "rl4co_op_check_solution")


def hbm_read_probe(buf: Tensor, sink: Tensor) -> None:
    st = _lib.lib().rl4co_hbm_read_probe(_ptr(buf), buf.numel() * buf.element_size(), _ptr(sink), _stream())
    _lib.check(st, "rl4co_hbm_read_probe")


def math_probe(fn: str, x: Tensor) -> Tensor:
    """exp / log / tanh of csrc/rl4co_math.h evaluated on the device (tests/test_math.py)."""
    x = _dev(x.contiguous(), torch.float32, "x")
    y = torch.empty_like(x)
    st = _lib.lib().rl4co_math_probe_f32({"exp": 0, "log": 1, "tanh": 2}[fn], _ptr(x), x.numel(), _ptr(y), _stream())
    _lib.check(st, "rl4co_math_probe_f32")
    return y


def uniform(shape, low: float, high: float, seed: int, stream_id: int, device, demand_capacity: float | None = None) -> Tensor:
    """U(low, high) drawn on the device in one launch (rl4co_uniform_f32, Philox4x32-10 keyed by ``seed`` /
    ``stream_id``); ``demand_capacity``: CVRP's integer-demand map ``(trunc(v) + 1) / capacity`` on top."""
    out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
    _dev(out, torch.float32, "out")
    st = _lib.lib().rl4co_uniform_f32(_ptr(out), out.numel(), float(low), float(high), int(seed) & ((1 << 64) - 1), int(stream_id),
                                      0 if demand_capacity is None else 1, float(demand_capacity or 1.0), _stream())
    _lib.check(st, "rl4co_uniform_f32")
    return out


# ---- N3: state augmentation and the POMO evaluation epilogue (csrc/augment.hip) -------------------------------------

def augment_dihedral8(xy: Tensor) -> Tensor:
    """[B, N, 2] -> [8 * B, N, 2], aug-major: the 8 symmetries of the unit square (data/transforms.py:16-46)."""
    b, n, two = xy.shape
    assert two == 2
    xy = _dev(xy, torch.float32, "xy")
    out = torch.empty((8 * b, n, 2), dtype=torch.float32, device=xy.device)
    st = _lib.lib().rl4co_augment_dihedral8_f32(_ptr(xy), b, n, _ptr(out), _stream())
    _lib.check(st, "rl4co_augment_dihedral8_f32")
    return out


def augment_symmetric(xy: Tensor, cos_phi: Tensor, sin_phi: Tensor, swap_axes: Tensor, offset: float = 0.5) -> Tensor:
    """[B, N, 2] and one (cos, sin, swap) per OUTPUT row [A * B] -> [A * B, N, 2] (data/transforms.py:49-69)."""
    b, n, two = xy.shape
    rows = cos_phi.numel()
    assert two == 2 and rows % b == 0 and sin_phi.numel() == rows and swap_axes.numel() == rows
    xy = _dev(xy, torch.float32, "xy")
    out = torch.empty((rows, n, 2), dtype=torch.float32, device=xy.device)
    st = _lib.lib().rl4co_augment_symmetric_f32(_ptr(xy), _ptr(_dev(cos_phi, torch.float32, "cos_phi")),
                                                _ptr(_dev(sin_phi, torch.float32, "sin_phi")), _ptr(_u8(swap_axes, "swap_axes")),
                                                b, rows // b, n, float(offset), _ptr(out), _stream())
    _lib.check(st, "rl4co_augment_symmetric_f32")
    return out


def pomo_best(reward: Tensor, actions: Tensor | None, num_augment: int, num_starts: int) -> dict:
    """Best start per augmentation and best augmentation per instance of a multistart rollout over an augmented batch
    (rows (s * A + a) * B + b), with the selected action rows, in one launch (zoo/pomo/model.py:112-140)."""
    a, s = int(num_augment), int(num_starts)
    rows = reward.numel()
    assert rows % (a * s) == 0
    b = rows // (a * s)
    reward = _dev(reward.reshape(-1), torch.float32, "reward")
    dev = reward.device
    out = {"max_reward": torch.empty((b, a), dtype=torch.float32, device=dev),
           "best_start": torch.empty((b, a), dtype=torch.int64, device=dev),
           "max_aug_reward": torch.empty(b, dtype=torch.float32, device=dev),
           "best_aug": torch.empty(b, dtype=torch.int64, device=dev)}
    t = 0
    if actions is not None:
        actions = _dev(actions, torch.int64, "actions")
        assert actions.shape[0] == rows
        t = actions.shape[1]
        out["best_multistart_actions"] = torch.empty((b, a, t), dtype=torch.int64, device=dev)
        out["best_aug_actions"] = torch.empty((b, t), dtype=torch.int64, device=dev)
    st = _lib.lib().rl4co_pomo_best(_ptr(reward), _ptr(actions), a, s, b, t, _ptr(out["max_reward"]), _ptr(out["best_start"]),
                                    _ptr(out["max_aug_reward"]), _ptr(out["best_aug"]), _ptr(out.get("best_multistart_actions")),
                                    _ptr(out.get("best_aug_actions")), _stream())
    _lib.check(st, "rl4co_pomo_best")
    return out
