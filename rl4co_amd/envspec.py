"""One table of per-environment facts behind the host-side kernel bindings.

The kernels take the environment as a template parameter and a fixed set of argument slots (``rl4co_am_decode_args``:
``demand``, ``used_capacity``, ``vehicle_capacity``, ``visited``, ``locs``, ...). Which state tensor of which environment
rides in which slot is stated HERE, once; ``kernels.bind_env_state`` / ``kernels.env_step``, ``policy`` (state, final
TensorDict, replay, horizon), ``teacher.run_backward`` and the encoder's feature columns read it. Adding an environment
means adding a record below: what the code must know about an environment — its context layout, its init embedding, which
kernels serve it — is a field here, and no binding asks for an environment by name. Data only: nothing here touches the GPU or
loads the library.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import torch

from . import _lib

# environments that share another one's kernels (same state, masks, embeddings): stochastic PCTSP only
# differs in which generated prize its reset() calls "real" (spctsp/env.py:8-21)
KERNEL_ENV = {"spctsp": "pctsp"}


def canonical_env(env_name: str) -> str:
    return KERNEL_ENV.get(env_name, env_name)


class Field(NamedTuple):
    """One state tensor. ``kind`` "traj": per trajectory — expanded over the starts s-major and cloned, the kernels write
    it; "inst": instance data — shared [B_inst, ...], contiguous, cast to ``dtype``. ``slot``: the field of
    ``rl4co_am_decode_args`` it rides in (the running context scalar rides in ``scalar`` of ``rl4co_env_replay_args``).
    ``shape``: "B" / "BN" as in the state; "B1": [B] in the state, [B, 1] in the final TensorDict; instance data: the
    dims behind B_inst ("N-1" = one entry per customer, "" = one value per instance)."""
    key: str
    kind: str
    dtype: str  # "i64" | "f32" | "u8" (bool or uint8: the same storage)
    slot: str | None
    shape: str


class Scalar(NamedTuple):
    """The context scalar ``base - state[running]`` (context.py:105-213). ``base``: a per-trajectory state key, or an
    instance table whose column 0 is repeated over the starts (``base_col0``: OP's entry limit of the depot = max_length).
    ``clamp``: at 0 from below (PCTSP, context.py:195). ``clock``: a second scalar taken as it is (CVRPTW's current time)."""
    running: str
    base: str
    base_col0: bool = False
    clamp: bool = False
    clock: str | None = None


class Features(NamedTuple):
    """``Scalar``'s sibling for a context of SEVERAL running scalars behind a linear layer of their own (mTSP,
    context.py:246-280: ``W_ctx [h_cur ; W_dyn f]``): ``names`` are the columns of ``f`` in the order of ``W_dyn``'s input —
    state keys, or derived quantities the kernels and the stepwise replay compute ("remaining_agents" = num_agents -
    agent_idx, "depot_distance" = |loc_cur - loc_0|). ``weight``: the layer's attribute on ``decoder.context_embedding``.
    The fold is one fp32 [len(names), 128] table (``cache.fold_features``, ``rl4co_am_decode_args.mtsp_ctx``)."""
    names: tuple[str, ...]
    weight: str


class Dynamic(NamedTuple):
    """Keys and values that move with a per-trajectory state tensor (SDVRP, zoo/am/decoder.py:142-152: a dynamic embedding
    ``Linear(1 -> 3 * 128)`` of state ``key``). ``weight``: the layer's attribute on ``decoder.dynamic_embedding``; ``slot``:
    where its fold (``cache.fold_dynamic``, fp32 [3, 128]) rides in ``rl4co_am_decode_args``."""
    key: str
    weight: str
    slot: str


class EnvSpec(NamedTuple):
    name: str
    env_id: int  # RL4CO_ENV_* of include/rl4co_amd.h
    has_depot: bool
    horizon: Callable[[int], int]  # longest rollout over n nodes (depot included)
    fields: tuple[Field, ...]
    scalar: Scalar | None
    step: tuple[str, tuple[str, ...]]  # the ``kernels`` step entry and the state keys it takes between action and err
    passthrough: tuple[str, ...]  # td keys the final TensorDict repeats over the starts as they are
    # customer init-embedding columns behind (x, y): (td key, drop the depot column, columns)
    features: tuple[tuple[str, bool, int], ...] = ()
    # init embedding: "all" every node alike | "depot" depot | customers with ``features`` behind (x, y), possibly none |
    # "pairs" depot | pickups | deliveries (the encoder kernels' three modes)
    init: str = "depot"
    ctx_first: bool = False  # context = (first node, current node), placeholder at step 0; else current node (+ scalars)
    feats: Features | None = None  # several running scalars through a second linear layer (instead of ``scalar``)
    dynamic: Dynamic | None = None
    # the reward is carried in the state and ONE non-neutral padding step follows the read-back: one trajectory per
    # instance (no multistart / multisample rows), no captured graph
    state_reward: bool = False
    fixed_horizon: bool = False  # every row takes exactly horizon(n) steps: a training step's status read-back may be asynchronous
    length_reward: bool = False  # the reward is a tour length: it can go out before the read-back (get_reward(horizon=...))
    depot_flag: str | None = None  # env attribute: the tour starts at the depot; without it the depot is never visited (n - 1 steps)
    # what serves it besides the decode kernels: the unfolded parity mode, the one-launch rl4co_env_replay, the
    # teacher-forced backward kernels (else ``no_teacher``: why not, as the fallback warning says it)
    unfold: bool = False
    replay: bool = True
    no_teacher: str | None = None

    @property
    def teacher(self) -> bool:
        return self.no_teacher is None

    @property
    def feature_width(self) -> int:
        return sum(width for _, _, width in self.features)

    def keys(self, kind: str | None = None) -> tuple[str, ...]:
        return tuple(f.key for f in self.fields if kind in (None, f.kind))

    @property
    def teacher_keys(self) -> tuple[str, ...]:
        """What the backward kernels read of the INSTANCE (td keys): the instance data and a per-instance scalar base."""
        base = () if self.scalar is None or self.scalar.base_col0 else (self.scalar.base,)
        return self.keys("inst") + base


def _fields(current_node: str, *own: tuple) -> tuple[Field, ...]:
    common = (("action_mask", "traj", "u8", "action_mask", "BN"), ("current_node", "traj", "i64", "current_node", current_node),
              ("done", "traj", "u8", "done", "B"))
    return tuple(Field(*f) for f in common + own)


_I = ("i", "traj", "i64", "step_i", "B")
_VISITED = ("visited", "traj", "u8", "visited", "BN")
_CVRP_FIELDS = (("demand", "inst", "f32", "demand", "N-1"), ("used_capacity", "traj", "f32", "used_capacity", "B1"),
                ("vehicle_capacity", "traj", "f32", "vehicle_capacity", "B1"), _VISITED)

SPECS = {s.name: s for s in (
    # TSP: exactly n steps
    EnvSpec("tsp", _lib.ENV_TSP, False, lambda n: n,
            _fields("B", ("first_node", "traj", "i64", "first_node", "B"), ("i", "traj", "i64", "step_i", "B1")),
            None, ("tsp_step", ("action_mask", "first_node", "current_node", "i", "done")),
            ("locs",), init="all", ctx_first=True, fixed_horizon=True, length_reward=True, unfold=True),
    # CVRP: every customer + at most one depot visit per customer + 1
    EnvSpec("cvrp", _lib.ENV_CVRP, True, lambda n: 2 * n, _fields("B1", *_CVRP_FIELDS),
            Scalar("used_capacity", "vehicle_capacity"),
            ("cvrp_step", ("demand", "used_capacity", "vehicle_capacity", "visited", "current_node", "action_mask", "done")),
            ("locs", "demand"), features=(("demand", False, 1),), length_reward=True, unfold=True),
    # OP: every customer once, the closing depot visit, and a depot pick at step 0 costs one more. The tour length rides
    # in the used_capacity slot; the per-node entry limits (max_length table) and the coordinates are instance data
    EnvSpec("op", _lib.ENV_OP, True, lambda n: n + 2,
            _fields("B1", ("locs", "inst", "f32", "locs", "N2"), ("max_length", "inst", "f32", "max_length", "N"),
                    ("tour_length", "traj", "f32", "used_capacity", "B"), _I, _VISITED),
            Scalar("tour_length", "max_length", base_col0=True),
            ("op_step", ("locs", "max_length", "tour_length", "visited", "current_node", "i", "action_mask", "done")),
            ("locs", "prize", "max_length"), features=(("prize", True, 1),)),
    # PCTSP: every customer once and the closing depot visit (the depot is masked at step 0). The real prize per node
    # (depot column 0) rides in the demand slot, the prize collected so far in used_capacity, prize_required in
    # vehicle_capacity
    EnvSpec("pctsp", _lib.ENV_PCTSP, True, lambda n: n,
            _fields("B", ("real_prize", "inst", "f32", "demand", "N"), ("cur_total_prize", "traj", "f32", "used_capacity", "B"),
                    ("prize_required", "traj", "f32", "vehicle_capacity", "B"), _I, _VISITED),
            Scalar("cur_total_prize", "prize_required", clamp=True),
            ("pctsp_step", ("real_prize", "cur_total_prize", "visited", "current_node", "i", "action_mask", "done")),
            ("locs", "real_prize", "expected_prize", "penalty"), features=(("expected_prize", False, 1), ("penalty", True, 1))),
    # PDP: every node once (the depot too under force_start_at_depot: else it is never visited and a rollout is exactly one
    # step per location). `available` rides in the visited slot; no scalar
    EnvSpec("pdp", _lib.ENV_PDP, True, lambda n: n,
            _fields("B1", ("available", "traj", "u8", "visited", "BN"), ("to_deliver", "traj", "u8", "to_deliver", "BN"),
                    ("i", "traj", "i64", "step_i", "B1")),
            None, ("pdp_step", ("available", "to_deliver", "current_node", "i", "action_mask", "done")),
            ("locs",), init="pairs", length_reward=True, depot_flag="force_start_at_depot"),
    # CVRPTW: CVRP + clock; coordinates, (start, end) windows and service times as fp32 instance data (the reference
    # keeps integer-valued windows)
    EnvSpec("cvrptw", _lib.ENV_CVRPTW, True, lambda n: 2 * n,
            _fields("B1", *_CVRP_FIELDS, ("locs", "inst", "f32", "locs", "N2"),
                    ("time_windows", "inst", "f32", "time_windows", "N2"), ("durations", "inst", "f32", "durations", "N"),
                    ("current_time", "traj", "f32", "current_time", "B1")),
            Scalar("used_capacity", "vehicle_capacity", clock="current_time"),
            ("cvrptw_step", ("demand", "locs", "time_windows", "durations", "used_capacity", "vehicle_capacity", "current_time",
                             "visited", "current_node", "action_mask", "done")),
            ("locs", "demand", "time_windows", "durations"),
            features=(("demand", False, 1), ("time_windows", True, 2), ("durations", True, 1)), length_reward=True),
    # SDVRP (sdvrp/env.py:56-123), a DYNAMIC embedding (zoo/am/decoder.py:142-152): the state moves the keys and values
    # every step, so the per-trajectory state tensor is also an operand of the attention. Served by the decode kernels
    # (STREAM / LDS / WIDE) alone. CVRP's instance, but a visit delivers min(remaining demand, remaining capacity) and a
    # customer stays until its demand is 0. `demand_with_depot` [B, N] is per trajectory and written by the kernels; the
    # init embedding reads the INITIAL `demand`. Horizon: a customer visit either zeroes that customer's demand (at most
    # n - 1 such visits, a zeroed customer is masked for good) or fills the vehicle (used = cap). After a fill, cap - used
    # of later loads stays an exact difference of the fp32 demands delivered since the depot (Sterbenz), so each customer
    # is the filling visit at most twice: <= 2 (n - 1) fills. At most one depot visit follows each customer visit (the
    # depot is masked while the vehicle stands on it and a customer is feasible): <= 2 * 3 (n - 1) < 6 n steps.
    EnvSpec("sdvrp", _lib.ENV_SDVRP, True, lambda n: 6 * n,
            _fields("B1", ("demand_with_depot", "traj", "f32", "demand_state", "BN"),
                    ("used_capacity", "traj", "f32", "used_capacity", "B1"),
                    ("vehicle_capacity", "traj", "f32", "vehicle_capacity", "B1")),
            Scalar("used_capacity", "vehicle_capacity"),
            ("sdvrp_step", ("demand_with_depot", "used_capacity", "vehicle_capacity", "current_node", "action_mask", "done")),
            ("locs", "demand"), features=(("demand", False, 1),), length_reward=True, replay=False,
            dynamic=Dynamic("demand_with_depot", "projection", "dyn_vectors"),
            no_teacher="the dynamic embedding (remaining demand in keys and values) is not in the backward kernels"),
    # mTSP (mtsp/env.py:63-131), a min-max objective: the REWARD is carried in the state and the context holds several
    # running scalars (`Features`). Decode kernels alone, one trajectory per instance. n nodes INCLUDING the depot; up to num_agents subtours from the depot, the reward is the
    # longest. The mask is the state (the reference's `available`). agent_idx rides in step_i, current_length in
    # used_capacity, max_subtour_length in current_time. Horizon: n - 1 customer visits; every depot visit follows a
    # customer visit (the depot is closed while the agent stands on it) and comes before done (the rollout ends AT done):
    # at most 2 (n - 1) < 2 n steps.
    EnvSpec("mtsp", _lib.ENV_MTSP, True, lambda n: 2 * n,
            tuple(Field(*f) for f in (
                ("action_mask", "traj", "u8", "action_mask", "BN"), ("current_node", "traj", "i64", "current_node", "B"),
                ("done", "traj", "u8", "done", "B1"),
                ("locs", "inst", "f32", "locs", "N2"), ("num_agents", "inst", "i64", "num_agents", ""),
                ("agent_idx", "traj", "i64", "step_i", "B"), ("current_length", "traj", "f32", "used_capacity", "B"),
                ("max_subtour_length", "traj", "f32", "current_time", "B"))),
            None,
            ("mtsp_step", ("locs", "num_agents", "agent_idx", "current_length", "max_subtour_length", "current_node",
                           "action_mask", "done")),
            ("locs", "num_agents"),
            feats=Features(("remaining_agents", "current_length", "max_subtour_length", "depot_distance"), "proj_dynamic_feats"),
            state_reward=True, replay=False,
            no_teacher="the four-scalar context (proj_dynamic_feats) and the min-max state are not in the backward kernels"),
)}


def spec(env_name: str) -> EnvSpec:
    return SPECS[canonical_env(env_name)]


def rem_base(sp: EnvSpec, state: dict, b: int):
    """The context scalar's minuend, one per trajectory (None: no scalar)."""
    if sp.scalar is None:
        return None
    base = state[sp.scalar.base]
    if sp.scalar.base_col0:
        base = base[:, 0]
        base = (base if base.shape[0] == b else base.repeat(b // base.shape[0])).contiguous()
    return base


def customer_features(sp: EnvSpec, td, dtype=torch.float32) -> list:
    """The customers' init-embedding features behind the coordinates (env_embeddings/init.py), ``dtype`` [B, n - 1, k] each
    in the order of the embedding's input columns."""
    cols = [(td[key][:, 1:] if drop_depot else td[key]).to(dtype) for key, drop_depot, _ in sp.features]
    return [c if c.dim() == 3 else c[..., None] for c in cols]
