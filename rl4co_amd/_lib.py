"""ctypes binding of the C-ABI declared in ``include/rl4co_amd.h``.

The library is the product: there is NO CPU fallback. Importing this module is cheap;
the first call to :func:`lib` loads ``librl4co_amd.so`` and raises if it is missing.
"""
from __future__ import annotations

import ctypes as C
import os
from functools import lru_cache

from . import build as _build

RL4CO_OK = 0
ABI_VERSION = 29  # RL4CO_ABI_VERSION of include/rl4co_amd.h this binding's argument lists were written for
ENV_TSP, ENV_CVRP, ENV_OP, ENV_PCTSP, ENV_PDP, ENV_CVRPTW, ENV_SDVRP, ENV_MTSP = 0, 1, 2, 3, 4, 5, 6, 7
DECODE_GREEDY, DECODE_SAMPLE, DECODE_EVALUATE = 0, 1, 2
DT_F32, DT_BF16, DT_F16 = 0, 1, 2
VARIANT_AUTO, VARIANT_STREAM, VARIANT_LDS, VARIANT_WIDE, VARIANT_MS, VARIANT_STREAM_REG = 0, 1, 2, 3, 4, 5

EBIT_NAN_LOGIT = 1
EBIT_INFEASIBLE = 2
EBIT_INVALID_TOUR = 4
EBIT_CAPACITY = 8
EBIT_MAX_STEPS = 16
EBIT_NEG_INF_LOGP = 32
EBIT_DUPLICATES = 64
EBIT_MAX_LENGTH = 128
EBIT_PRIZE = 256
EBIT_NOT_ALL_NODES = 512
EBIT_DEPOT_MIDDLE = 1024
EBIT_NO_PICKUP = 2048
EBIT_TW_NEGATIVE, EBIT_TW_RETURN, EBIT_TW_DURATION, EBIT_TW_EMPTY, EBIT_TW_DEADLINE = 4096, 8192, 16384, 32768, 65536
EBIT_BEAM_INFEASIBLE = 131072
EBIT_TOUR_INDEX = 262144
ACO_SAMPLE, ACO_UPDATE = 1, 2
LOGZ_POOL_REFERENCE, LOGZ_POOL_INSTANCE = 0, 1

# Reference assertion messages (file:line in the reference checkout) per sticky bit.
ERROR_MESSAGES = {
    EBIT_NAN_LOGIT: "Logits contain NaNs",  # nn/attention.py:296
    EBIT_INFEASIBLE: "infeasible action selected",  # utils/decoding.py:393,409
    EBIT_INVALID_TOUR: "Invalid tour",  # tsp/env.py:164, cvrp/env.py:163
    EBIT_CAPACITY: "Used more than capacity",  # cvrp/env.py:176
    EBIT_MAX_STEPS: "Exceeded maximum number of steps during decoding",  # constructive/base.py:237
    EBIT_NEG_INF_LOGP: "Logprobs should not be -inf, check sampling procedure!",  # decoding.py:56
    EBIT_DUPLICATES: "Duplicates",  # op/env.py:181
    EBIT_MAX_LENGTH: "Max length exceeded",  # op/env.py:192-194
    EBIT_PRIZE: "Total prize does not satisfy min total prize",  # pctsp/env.py:192-201
    EBIT_NOT_ALL_NODES: "Not visiting all nodes",  # pdp/env.py:208-213
    EBIT_DEPOT_MIDDLE: "Going back to depot in the middle of the tour (not allowed)",  # pdp/env.py:216-218
    EBIT_NO_PICKUP: "Deliverying without pick-up",  # pdp/env.py:220-223
    EBIT_TW_NEGATIVE: "Time windows must be non-negative.",  # cvrptw/env.py:153
    EBIT_TW_RETURN: "vehicle cannot perform service and get back to depot in time.",  # cvrptw/env.py:154-157
    EBIT_TW_DURATION: "Service durations must be non-negative.",  # cvrptw/env.py:158
    EBIT_TW_EMPTY: "there are unfeasible time windows",  # cvrptw/env.py:159-161
    EBIT_TW_DEADLINE: "vehicle cannot start service before deadline",  # cvrptw/env.py:176-179
    EBIT_BEAM_INFEASIBLE: "infeasible action selected",  # utils/decoding.py:485 (beam search kept a -inf candidate)
    EBIT_TOUR_INDEX: "tour index out of range",  # rl4co_tsp_two_opt: an index outside [0, N) (no reference message)
}

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float


class AmDecodeArgs(C.Structure):
    """Mirror of ``struct rl4co_am_decode_args`` (field order and types must match the header)."""

    _fields_ = [
        ("env", _i32), ("B", _i32), ("B_inst", _i32), ("N", _i32),
        ("mode", _i32), ("max_steps", _i32), ("mask_inner", _i32), ("mask_logits", _i32),
        ("tanh_clipping", _f32), ("temperature", _f32),
        ("cache_dtype", _i32), ("variant", _i32),
        ("glimpse_key", _vp), ("glimpse_val", _vp), ("logit_key", _vp),
        ("kvl_row_stride", _i64), ("kvl_batch_stride", _i64),
        ("ctx_first", _vp), ("ctx_cur", _vp), ("q_bias", _vp), ("q_step0", _vp), ("w_cap", _vp),
        ("unfold", _i32), ("ctx_width", _i32), ("node_embed", _vp), ("w_ctx_t", _vp), ("w_out_t", _vp),
        ("w_placeholder", _vp),
        ("action_mask", _vp), ("first_node", _vp), ("current_node", _vp), ("step_i", _vp),
        ("done", _vp),
        ("demand", _vp), ("used_capacity", _vp), ("vehicle_capacity", _vp), ("visited", _vp),
        ("locs", _vp), ("max_length", _vp), ("to_deliver", _vp),
        ("time_windows", _vp), ("durations", _vp), ("current_time", _vp), ("w_time", _vp),
        ("dyn_vectors", _vp), ("demand_state", _vp),
        ("exp_noise", _vp), ("philox_seed", C.c_uint64), ("philox_offset", C.c_uint64), ("philox_seed_dev", _vp),
        ("forced_actions", _vp),
        ("t0", _i32), ("out_stride", _i32),
        ("actions", _vp), ("logps", _vp), ("all_logps", _vp), ("entropy", _vp),
        ("n_steps", _vp), ("steps_summary", _vp), ("err", _vp),
        ("mtsp_ctx", _vp), ("num_agents", _vp),
        ("ctx_dtype", _i32), ("reserved0", _i32), ("ctx_row_stride", _i64), ("ctx_batch_stride", _i64),
        ("top_k", _i32), ("top_p", _f32), ("kept_bits", _vp), ("kept_words", _i32), ("reserved1", _i32),
    ]


class AmDecodeBeamArgs(C.Structure):
    """Mirror of ``struct rl4co_am_decode_beam_args`` (field order and types must match the header)."""

    _fields_ = [
        ("env", _i32), ("B_inst", _i32), ("N", _i32), ("beam_width", _i32),
        ("max_steps", _i32), ("mask_inner", _i32), ("mask_logits", _i32), ("cache_dtype", _i32),
        ("tanh_clipping", _f32), ("temperature", _f32),
        ("glimpse_key", _vp), ("glimpse_val", _vp), ("logit_key", _vp),
        ("kvl_row_stride", _i64), ("kvl_batch_stride", _i64),
        ("ctx_first", _vp), ("ctx_cur", _vp), ("q_bias", _vp), ("q_step0", _vp), ("w_cap", _vp),
        ("action_mask", _vp), ("first_node", _vp), ("current_node", _vp), ("step_i", _vp), ("done", _vp),
        ("demand", _vp), ("used_capacity", _vp), ("vehicle_capacity", _vp), ("visited", _vp),
        ("out_stride", _i32), ("reserved0", _i32),
        ("actions", _vp), ("logps", _vp), ("step_nodes", _vp), ("step_logps", _vp), ("parents", _vp), ("cum_logp", _vp),
        ("steps_summary", _vp), ("err", _vp),
    ]


class TspTwoOptArgs(C.Structure):
    """Mirror of ``struct rl4co_tsp_two_opt_args`` (field order and types must match the header)."""

    _fields_ = [
        ("B", _i32), ("N", _i32), ("T", _i32), ("max_iterations", _i32),
        ("locs", _vp), ("distances", _vp), ("actions", _vp), ("out_actions", _vp), ("iterations", _vp), ("err", _vp),
    ]


class TspNlsArgs(C.Structure):
    """Mirror of ``struct rl4co_tsp_nls_args`` (field order and types must match the header)."""

    _fields_ = [
        ("R", _i32), ("n_instances", _i32), ("N", _i32), ("T", _i32),
        ("ls_max_iterations", _i32), ("perturb_max_iterations", _i32), ("n_perturbations", _i32), ("reserved0", _i32),
        ("locs", _vp), ("perturb_distances", _vp), ("actions", _vp), ("out_actions", _vp), ("out_reward", _vp),
        ("scans", _vp), ("accepted", _vp), ("err", _vp),
    ]


class NargnnArgs(C.Structure):
    """Mirror of ``struct rl4co_nargnn_args`` (field order and types must match the header)."""

    _fields_ = [
        ("B", _i32), ("N", _i32), ("K", _i32), ("D", _i32), ("L", _i32), ("H", _i32), ("n_workgroups", _i32), ("reserved0", _i32),
        ("small_value", _f32), ("fill_value", _f32),
        ("locs", _vp), ("neighbors", _vp), ("edge_cost", _vp), ("init_w", _vp), ("init_b", _vp), ("edge_w", _vp), ("edge_b", _vp),
        ("lin_w", _vp), ("lin_b", _vp), ("bn", _vp), ("mlp_w", _vp), ("mlp_b", _vp), ("out_w", _vp), ("out_b", _vp),
        ("scratch", _vp), ("scratch_bytes", _i64), ("heatmap", _vp), ("node_embed", _vp), ("err", _vp),
    ]


class NargnnDepotArgs(C.Structure):
    """Mirror of ``struct rl4co_nargnn_depot_args`` (field order and types must match the header)."""

    _fields_ = [
        ("B", _i32), ("N", _i32), ("K", _i32), ("F", _i32), ("D", _i32), ("L", _i32), ("H", _i32), ("n_workgroups", _i32),
        ("small_value", _f32), ("fill_value", _f32),
        ("locs", _vp), ("feats", _vp), ("neighbors", _vp), ("edge_cost", _vp), ("depot_cost", _vp),
        ("init_w", _vp), ("init_b", _vp), ("depot_w", _vp), ("depot_b", _vp), ("edge_w", _vp), ("edge_b", _vp),
        ("lin_w", _vp), ("lin_b", _vp), ("bn", _vp), ("mlp_w", _vp), ("mlp_b", _vp), ("out_w", _vp), ("out_b", _vp),
        ("scratch", _vp), ("scratch_bytes", _i64), ("heatmap", _vp), ("node_embed", _vp), ("err", _vp),
    ]


class NargnnTrainArgs(C.Structure):
    """Mirror of ``struct rl4co_nargnn_train_args`` (field order and types must match the header)."""

    _fields_ = [
        ("B", _i32), ("N", _i32), ("K", _i32), ("D", _i32), ("L", _i32), ("reserved0", _i32), ("eps", _f32), ("reserved1", _i32),
        ("neighbors", _vp), ("csr_ptr", _vp), ("csr_src", _vp), ("x_in", _vp), ("w_in", _vp),
        ("lin_w", _vp), ("lin_b", _vp), ("bn_w", _vp), ("bn_b", _vp), ("workspace", _vp), ("workspace_bytes", _i64),
        ("x_out", _vp), ("w_out", _vp), ("stats", _vp), ("grad_x_out", _vp), ("grad_w_out", _vp),
        ("grad_x_in", _vp), ("grad_w_in", _vp), ("grad_lin_w", _vp), ("grad_lin_b", _vp), ("grad_bn_w", _vp),
        ("grad_bn_b", _vp), ("err", _vp),
    ]


class NargnnDepotTrainArgs(C.Structure):
    """Mirror of ``struct rl4co_nargnn_depot_train_args``: the fields of ``rl4co_nargnn_train_args`` over the depot graph's
    rows."""

    _fields_ = list(NargnnTrainArgs._fields_)


class NargnnLogzArgs(C.Structure):
    """Mirror of ``struct rl4co_nargnn_logz_args`` (field order and types must match the header)."""

    _fields_ = [
        ("B", _i32), ("E", _i32), ("Z", _i32), ("pooling", _i32), ("rows", _i64),
        ("w", _vp), ("W1", _vp), ("b1", _vp), ("W2", _vp), ("b2", _vp), ("workspace", _vp), ("workspace_bytes", _i64),
        ("logZ", _vp), ("grad_logZ", _vp), ("grad_w", _vp), ("grad_W1", _vp), ("grad_b1", _vp), ("grad_W2", _vp),
        ("grad_b2", _vp),
    ]


class AcoTspArgs(C.Structure):
    """Mirror of ``struct rl4co_aco_tsp_args`` (field order and types must match the header)."""

    _fields_ = [
        ("B", _i32), ("N", _i32), ("n_ants", _i32), ("iterations", _i32), ("phases", _i32), ("has_best", _i32),
        ("alpha", _f32), ("beta", _f32), ("decay", _f32), ("Q", _f32), ("temperature", _f32), ("reserved0", _i32),
        ("philox_seed", C.c_uint64), ("philox_offset", C.c_uint64), ("philox_seed_dev", _vp),
        ("log_heuristic", _vp), ("pheromone", _vp), ("locs", _vp), ("start_nodes", _vp), ("ln_noise", _vp),
        ("forced_actions", _vp), ("logits_scratch", _vp), ("actions", _vp), ("reward", _vp), ("logps", _vp),
        ("all_logps", _vp), ("iter_actions", _vp), ("iter_reward", _vp), ("final_reward", _vp), ("final_actions", _vp),
        ("final_reward_cache", _vp), ("err", _vp),
    ]


class AcoTspGradArgs(C.Structure):
    """Mirror of ``struct rl4co_aco_tsp_grad_args`` (field order and types must match the header)."""

    _fields_ = [
        ("B", _i32), ("N", _i32), ("n_ants", _i32), ("row_split", _i32), ("temperature", _f32), ("reserved0", _i32),
        ("heatmap", _vp), ("actions", _vp), ("grad_ll", _vp), ("grad_steps", _vp), ("pos_scratch", _vp),
        ("grad_heatmap", _vp), ("err", _vp),
    ]


class AcoDepotGradArgs(C.Structure):
    """Mirror of ``struct rl4co_aco_depot_grad_args`` (field order and types must match the header)."""

    _fields_ = [
        ("env", _i32), ("B", _i32), ("N", _i32), ("n_ants", _i32), ("row_split", _i32), ("multistart", _i32),
        ("temperature", _f32), ("reserved0", _i32),
        ("heatmap", _vp), ("actions", _vp), ("grad_ll", _vp), ("grad_steps", _vp), ("locs", _vp), ("demand", _vp),
        ("vehicle_capacity", _vp), ("prize", _vp), ("max_length", _vp), ("scratch", _vp), ("grad_heatmap", _vp), ("err", _vp),
    ]


class AcoCvrpArgs(C.Structure):
    """Mirror of ``struct rl4co_aco_cvrp_args`` (field order and types must match the header)."""

    _fields_ = [
        ("B", _i32), ("N", _i32), ("n_ants", _i32), ("iterations", _i32), ("phases", _i32), ("has_best", _i32),
        ("T", _i32), ("iteration_base", _i32),
        ("alpha", _f32), ("beta", _f32), ("decay", _f32), ("Q", _f32), ("temperature", _f32), ("reserved0", _i32),
        ("philox_seed", C.c_uint64), ("philox_offset", C.c_uint64), ("philox_seed_dev", _vp),
        ("log_heuristic", _vp), ("pheromone", _vp), ("locs", _vp), ("demand", _vp), ("vehicle_capacity", _vp),
        ("start_nodes", _vp), ("ln_noise", _vp), ("forced_actions", _vp), ("logits_scratch", _vp), ("actions", _vp),
        ("lengths", _vp), ("reward", _vp), ("logps", _vp), ("all_logps", _vp), ("iter_actions", _vp), ("iter_lengths", _vp),
        ("iter_reward", _vp), ("final_reward", _vp), ("final_actions", _vp), ("final_iteration", _vp),
        ("final_reward_cache", _vp), ("err", _vp),
    ]


class AcoPrizeArgs(C.Structure):
    """Mirror of ``struct rl4co_aco_prize_args`` (field order and types must match the header)."""

    _fields_ = [
        ("B", _i32), ("N", _i32), ("n_ants", _i32), ("iterations", _i32), ("phases", _i32), ("has_best", _i32),
        ("T", _i32), ("iteration_base", _i32), ("env", _i32), ("n_workgroups", _i32),
        ("alpha", _f32), ("beta", _f32), ("decay", _f32), ("Q", _f32), ("temperature", _f32), ("reserved0", _i32),
        ("philox_seed", C.c_uint64), ("philox_offset", C.c_uint64), ("philox_seed_dev", _vp),
        ("log_heuristic", _vp), ("pheromone", _vp), ("locs", _vp), ("prize", _vp), ("penalty", _vp), ("max_length", _vp),
        ("ln_noise", _vp), ("forced_actions", _vp), ("logits_scratch", _vp), ("actions", _vp),
        ("lengths", _vp), ("reward", _vp), ("logps", _vp), ("all_logps", _vp), ("iter_actions", _vp), ("iter_lengths", _vp),
        ("iter_reward", _vp), ("final_reward", _vp), ("final_actions", _vp), ("final_iteration", _vp),
        ("final_reward_cache", _vp), ("err", _vp),
    ]


class HeatmapDecodeOpts(C.Structure):
    """Mirror of ``struct rl4co_heatmap_decode_opts`` (field order and types must match the header)."""

    _fields_ = [("greedy", _i32), ("top_k", _i32), ("top_p", _f32), ("reserved0", _i32)]


class EnvReplayArgs(C.Structure):
    """Mirror of ``struct rl4co_env_replay_args``."""

    _fields_ = [
        ("env", _i32), ("B", _i32), ("B_inst", _i32), ("N", _i32), ("T", _i32), ("reserved0", _i32),
        ("actions", _vp),
        ("action_mask", _vp), ("current_node", _vp), ("done", _vp), ("first_node", _vp), ("step_i", _vp), ("visited", _vp),
        ("to_deliver", _vp), ("scalar", _vp), ("current_time", _vp),
        ("vehicle_capacity", _vp), ("demand", _vp), ("locs", _vp), ("max_length", _vp), ("time_windows", _vp),
        ("durations", _vp), ("rem_base", _vp),
        ("masks", _vp), ("prev", _vp), ("first", _vp), ("use_placeholder", _vp), ("rem", _vp), ("now", _vp), ("err", _vp),
        ("mask_bits", _vp), ("mask_words", _i32), ("reserved1", _i32),
    ]


class CrossAttnArgs(C.Structure):
    """Mirror of ``struct rl4co_cross_attn_args``."""

    _fields_ = [
        ("B", _i32), ("B_inst", _i32), ("T", _i32), ("N", _i32),
        ("q", _vp), ("q_stride", _i64), ("kv", _vp), ("kv_stride", _i64),
        ("mask", _vp), ("mask_words", _i32), ("reserved0", _i32),
        ("out", _vp), ("lse", _vp), ("dout", _vp), ("dq", _vp), ("dkv", _vp), ("dq_partial", _vp),
    ]


# name -> (restype, argtypes); every symbol include/rl4co_amd.h declares.
SYMBOLS = {
    "rl4co_version": (C.c_char_p, []),
    "rl4co_last_error": (C.c_char_p, []),
    "rl4co_abi_version": (C.c_int, []),
    "rl4co_gather_by_index_f32": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    "rl4co_tour_length_f32": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_tour_length_dyn_f32": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_tsp_check_solution": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_cvrp_check_solution": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_tsp_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_cvrp_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_sdvrp_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_mtsp_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_op_max_length": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_op_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_gather_sum_f32": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_op_check_solution": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_pctsp_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_pctsp_check_solution": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_cvrptw_step": (C.c_int, [_vp] * 12 + [C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_cvrptw_check_solution": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_pdp_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_pdp_check_solution": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_env_replay": (C.c_int, [C.POINTER(EnvReplayArgs), _vp]),
    "rl4co_am_decode": (C.c_int, [C.POINTER(AmDecodeArgs), _vp]),
    "rl4co_am_teacher_backward": (C.c_int, [_vp, _vp]),
    "rl4co_am_teacher_max_nodes": (C.c_int, []),
    "rl4co_am_teacher_variant": (C.c_int, [_vp]),
    "rl4co_skip_inorm_fwd": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, C.c_float, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),  # (dtype id first: RL4CO_DT_BF16 / RL4CO_DT_F16)
    "rl4co_skip_inorm_bwd": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),  # (dtype id first: RL4CO_DT_BF16 / RL4CO_DT_F16)
    "rl4co_skip_lnorm_fwd": (C.c_int, [C.c_int, _vp, _vp, C.c_float, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),  # (dtype id first: RL4CO_DT_BF16 / RL4CO_DT_F16)
    "rl4co_skip_lnorm_bwd": (C.c_int, [C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp]),  # (dtype id first: RL4CO_DT_BF16 / RL4CO_DT_F16)
    "rl4co_skip_inorm_max_nodes": (C.c_int, []),
    "rl4co_mlp_input_grad": (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, C.c_int, _vp, _vp, _vp]),
    "rl4co_skip_bnorm_stats": (C.c_int, [C.c_int, _vp, _vp, C.c_int64, _vp, _vp, _vp]),  # (dtype id first: RL4CO_DT_BF16 / RL4CO_DT_F16)
    "rl4co_bnorm_apply": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp]),  # (dtype id first: RL4CO_DT_BF16 / RL4CO_DT_F16)
    "rl4co_skip_bnorm_eval": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp]),  # (dtype id first: RL4CO_DT_BF16 / RL4CO_DT_F16)
    "rl4co_bnorm_bwd": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp, _vp]),  # (dtype id first: RL4CO_DT_BF16 / RL4CO_DT_F16)
    "rl4co_init_embed": (C.c_int, [C.c_int, _vp, _vp, _vp, C.c_int64, C.c_int, _vp, _vp]),  # (dtype id first: RL4CO_DT_BF16 / RL4CO_DT_F16)
    "rl4co_init_embed_wgrad": (C.c_int, [C.c_int, _vp, _vp, C.c_int64, C.c_int, _vp, _vp, _vp]),  # (dtype id first: RL4CO_DT_BF16 / RL4CO_DT_F16)
    "rl4co_linear": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, _vp]),  # (dtype id first: RL4CO_DT_BF16 / RL4CO_DT_F16)
    "rl4co_attn_fwd": (C.c_int, [C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),  # (dtype id first: RL4CO_DT_BF16 / RL4CO_DT_F16)
    "rl4co_attn_bwd": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp]),  # (dtype id first: RL4CO_DT_BF16 / RL4CO_DT_F16)
    "rl4co_attn_max_nodes": (C.c_int, []),
    "rl4co_attn_bwd_wide": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),  # (dtype id first)
    "rl4co_attn_wide_max_nodes": (C.c_int, []),
    "rl4co_cross_attn_fwd": (C.c_int, [C.c_int, C.POINTER(CrossAttnArgs), _vp]),
    "rl4co_cross_attn_bwd": (C.c_int, [C.c_int, C.POINTER(CrossAttnArgs), _vp]),
    "rl4co_cross_attn_chunks": (C.c_int, [C.c_int]),
    "rl4co_logit_logp_fwd": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int64, C.c_int, C.c_float, C.c_float, _vp, _vp, _vp, _vp]),
    "rl4co_logit_logp_bwd": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int64, C.c_int, C.c_float, C.c_float, _vp, _vp]),
    "rl4co_skip_inorm_wide_max_nodes": (C.c_int, []),
    "rl4co_attn_flash": (C.c_int, [C.c_int, _vp, C.c_int, C.c_int, _vp, _vp]),  # (dtype id first: RL4CO_DT_BF16 / RL4CO_DT_F16)
    "rl4co_attn_flash_pre": (C.c_int, [C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, _vp]),  # (dtype id first: RL4CO_DT_BF16 / RL4CO_DT_F16)
    "rl4co_wgrad": (C.c_int, [C.c_int, _vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int64, _vp]),  # (dtype id first: RL4CO_DT_BF16 / RL4CO_DT_F16)
    "rl4co_am_encoder": (C.c_int, [_vp, _vp]),
    "rl4co_am_encoder_max_nodes": (C.c_int, []),
    "rl4co_am_encoder_train_fwd": (C.c_int, [_vp, _vp, _vp]),
    "rl4co_am_encoder_tokens16": (C.c_int, [_vp, _vp, C.c_int64, _vp]),
    "rl4co_am_encoder_tokens16_workspace": (C.c_int64, [C.c_int, C.c_int]),
    "rl4co_am_encoder_f32": (C.c_int, [_vp, _vp]),
    "rl4co_am_encoder_tokens_f32": (C.c_int, [_vp, _vp, C.c_int64, _vp]),
    "rl4co_am_encoder_tokens_f32_workspace": (C.c_int64, [C.c_int, C.c_int]),
    "rl4co_am_encoder_init_embeds16": (C.c_int, [_vp, _vp, _vp]),
    "rl4co_am_encoder_init_embeds_f32": (C.c_int, [_vp, _vp, _vp]),
    "rl4co_am_fold_tables_f32": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp]),
    "rl4co_am_decode_lds_bytes": (C.c_int, [C.c_int, C.c_int]),
    "rl4co_am_decode_row_groups": (C.c_int, [C.POINTER(AmDecodeArgs)]),
    "rl4co_am_decode_variant": (C.c_int, [C.POINTER(AmDecodeArgs)]),
    "rl4co_am_decode_beam": (C.c_int, [C.POINTER(AmDecodeBeamArgs), _vp]),
    "rl4co_am_decode_beam_max_width": (C.c_int, [C.c_int]),
    "rl4co_tsp_two_opt": (C.c_int, [C.POINTER(TspTwoOptArgs), _vp]),
    "rl4co_tsp_two_opt_lds_nodes": (C.c_int, []),
    "rl4co_aco_tsp": (C.c_int, [C.POINTER(AcoTspArgs), _vp]),
    "rl4co_aco_tsp_lds_nodes": (C.c_int, []),
    "rl4co_aco_tsp_logp_grad": (C.c_int, [C.POINTER(AcoTspGradArgs), _vp]),
    "rl4co_aco_tsp_grad_lds_entries": (C.c_int, []),
    "rl4co_aco_depot_logp_grad": (C.c_int, [C.POINTER(AcoDepotGradArgs), _vp]),
    "rl4co_aco_depot_grad_lds_entries": (C.c_int, []),
    "rl4co_aco_depot_grad_scratch_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "rl4co_aco_cvrp": (C.c_int, [C.POINTER(AcoCvrpArgs), _vp]),
    "rl4co_aco_cvrp_lds_nodes": (C.c_int, []),
    "rl4co_aco_prize": (C.c_int, [C.POINTER(AcoPrizeArgs), _vp]),
    "rl4co_aco_prize_lds_nodes": (C.c_int, [C.c_int]),
    "rl4co_aco_tsp_opts": (C.c_int, [C.POINTER(AcoTspArgs), C.POINTER(HeatmapDecodeOpts), _vp]),
    "rl4co_aco_cvrp_opts": (C.c_int, [C.POINTER(AcoCvrpArgs), C.POINTER(HeatmapDecodeOpts), _vp]),
    "rl4co_aco_prize_opts": (C.c_int, [C.POINTER(AcoPrizeArgs), C.POINTER(HeatmapDecodeOpts), _vp]),
    "rl4co_aco_tsp_logp_grad_opts": (C.c_int, [C.POINTER(AcoTspGradArgs), C.POINTER(HeatmapDecodeOpts), _vp]),
    "rl4co_aco_depot_logp_grad_opts": (C.c_int, [C.POINTER(AcoDepotGradArgs), C.POINTER(HeatmapDecodeOpts), _vp]),
    "rl4co_tsp_nls": (C.c_int, [C.POINTER(TspNlsArgs), _vp]),
    "rl4co_tsp_nls_lds_nodes": (C.c_int, []),
    "rl4co_nargnn_heatmap": (C.c_int, [C.POINTER(NargnnArgs), _vp]),
    "rl4co_nargnn_lds_nodes": (C.c_int, [C.c_int]),
    "rl4co_nargnn_scratch_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "rl4co_nargnn_depot_heatmap": (C.c_int, [C.POINTER(NargnnDepotArgs), _vp]),
    "rl4co_nargnn_depot_lds_nodes": (C.c_int, [C.c_int]),
    "rl4co_nargnn_depot_scratch_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "rl4co_nargnn_train_forward": (C.c_int, [C.POINTER(NargnnTrainArgs), _vp]),
    "rl4co_nargnn_train_backward": (C.c_int, [C.POINTER(NargnnTrainArgs), _vp]),
    "rl4co_nargnn_train_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "rl4co_nargnn_depot_train_forward": (C.c_int, [C.POINTER(NargnnDepotTrainArgs), _vp]),
    "rl4co_nargnn_depot_train_backward": (C.c_int, [C.POINTER(NargnnDepotTrainArgs), _vp]),
    "rl4co_nargnn_depot_train_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "rl4co_nargnn_logz_forward": (C.c_int, [C.POINTER(NargnnLogzArgs), _vp]),
    "rl4co_nargnn_logz_backward": (C.c_int, [C.POINTER(NargnnLogzArgs), _vp]),
    "rl4co_nargnn_logz_workspace_bytes": (C.c_int64, [C.c_int64]),
    "rl4co_select_start_nodes": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    "rl4co_augment_dihedral8_f32": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "rl4co_augment_symmetric_f32": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_float, _vp, _vp]),
    "rl4co_pomo_best": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rl4co_hbm_read_probe": (C.c_int, [_vp, _i64, _vp, _vp]),
    "rl4co_math_probe_f32": (C.c_int, [C.c_int, _vp, _i64, _vp, _vp]),
    "rl4co_uniform_f32": (C.c_int, [_vp, _i64, C.c_float, C.c_float, C.c_uint64, C.c_uint32, C.c_int, C.c_float, _vp]),
    # IEEE-half twins of the training-encoder / attention kernels (csrc/elem16.h)
}


class AmTrainSave(C.Structure):
    """Mirror of ``struct rl4co_am_train_save`` (field order and types must match the header)."""

    _fields_ = [("x0", _vp), ("out", _vp), ("qkv", _vp), ("att", _vp), ("y1", _vp), ("x1", _vp), ("h", _vp), ("y2", _vp),
                ("lse", _vp), ("stats", _vp)]


def dtype_id(dtype) -> int:
    """torch dtype of the cache planes -> RL4CO_DT_*"""
    import torch

    try:
        return {torch.float32: DT_F32, torch.bfloat16: DT_BF16, torch.float16: DT_F16}[dtype]
    except KeyError:
        raise TypeError(f"cache dtype must be float32, bfloat16 or float16, got {dtype}") from None


class Rl4coLibraryError(RuntimeError):
    pass


@lru_cache(maxsize=None)
def lib() -> C.CDLL:
    """Load ``librl4co_amd.so`` (building it in-tree first if it is stale or absent).

    torch is imported FIRST on purpose: the PyTorch-ROCm wheel bundles its own HIP runtime
    (``torch/lib/libamdhip64.so``, soname ``libamdhip64.so.7``). Our library needs the same soname,
    so once torch's copy is resident the dynamic loader binds us to it and kernels, streams and
    device pointers all live in ONE runtime. Loaded the other way round the process ends up with
    two HIP runtimes (ours from /opt/rocm, torch's bundled one) and torch's stream handles are
    meaningless to ours ("no ROCm-capable device is detected")."""
    import torch  # noqa: F401  (see above)

    # RL4CO_AMD_LIB: load a specific build instead (tools/enc_probe.sh times instrumented variants of one kernel)
    path = os.environ.get("RL4CO_AMD_LIB") or _build.build_library()
    try:
        handle = C.CDLL(str(path))
    except OSError as exc:  # pragma: no cover - depends on the environment
        raise Rl4coLibraryError(
            f"cannot load {path}: {exc}. The HIP extension is required; there is no CPU fallback."
        ) from exc
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(handle, name)  # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    got = handle.rl4co_abi_version()
    if got != ABI_VERSION:  # a stale build under unchanged symbol names would run with shifted arguments: refuse
        raise Rl4coLibraryError(f"{path} was built for ABI version {got}, this binding is written for {ABI_VERSION}: rebuild the library")
    return handle


def decode_row_groups(num_nodes: int, cache_dtype_id: int, max_steps: int, variant: int = VARIANT_AUTO,
                      num_trajectories: int = 1 << 20, num_instances: int | None = None) -> int:
    """Row groups G (the glimpse summation tree) of the kernel variant that serves this shape —
    a pure host query, usable without a GPU; the specified-order oracle mirrors it."""
    a = AmDecodeArgs()
    a.N, a.cache_dtype, a.max_steps, a.variant = int(num_nodes), int(cache_dtype_id), int(max_steps), int(variant)
    a.B = int(num_trajectories)
    a.B_inst = int(num_trajectories if num_instances is None else num_instances)
    g = lib().rl4co_am_decode_row_groups(C.byref(a))
    if g < 0:
        raise Rl4coLibraryError(f"no decode kernel variant {variant} for N={num_nodes}, dtype id {cache_dtype_id}")
    return g


def check(status: int, what: str) -> None:
    if status != RL4CO_OK:
        msg = lib().rl4co_last_error().decode("utf-8", "replace")
        raise Rl4coLibraryError(f"{what} failed with status {status}: {msg}")


def raise_for_error_bits(bits: int) -> None:
    """Re-raise the reference's assertion for the lowest sticky error bit set."""
    if bits == 0:
        return
    for bit, msg in ERROR_MESSAGES.items():
        if bits & bit:
            raise AssertionError(msg)
    raise AssertionError(f"rollout kernel reported error bits {bits:#x}")


_warned: set[str] = set()


def warn_fallback(key: str, message: str) -> None:
    """One ``RuntimeWarning`` per distinct reason when a part of the path leaves the hand-written kernels for the torch
    implementation (a shape or precision regime no kernel serves). The results stay correct — torch runs the same
    algebra — but the speed is torch's; silent fallbacks hid that."""
    if key in _warned:
        return
    _warned.add(key)
    import warnings

    warnings.warn(f"rl4co_amd: {message}", RuntimeWarning, stacklevel=3)
