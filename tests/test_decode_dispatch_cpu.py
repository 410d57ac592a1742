"""The host side of the decode launch without a device: which variant serves and the row groups, entry by entry against
the table recorded before the launchers read csrc/env_table.h (oracle/gen_dispatch_table.py), and the argument refusals of
the entries per environment. Nothing here can reach a launch: the two queries are pure host functions, and every call of an
entry carries a scalar its last (decode) or an early (beam) requirement refuses."""
import ctypes

import numpy as np
import pytest

from oracle import gen_dispatch_table as G
from rl4co_amd import _lib
from rl4co_amd.teacher import AmTeacherArgs

ERR_ARG = 1
DUMMY = 0x10000  # non-null, 16-byte aligned, never followed
ENV_IDS = {"tsp": 0, "cvrp": 1, "op": 2, "pctsp": 3, "pdp": 4, "cvrptw": 5, "sdvrp": 6, "mtsp": 7}
NO_ENV = (-1, 8, 99)

# the slots rl4co_am_decode requires per environment, as its chain of requirements stood before the table (folded mode)
REQUIRED = {
    "tsp": ("ctx_first", "q_step0", "first_node", "step_i"),
    "cvrp": ("w_cap", "demand", "used_capacity", "vehicle_capacity", "visited"),
    "cvrptw": ("w_cap", "w_time", "demand", "used_capacity", "vehicle_capacity", "visited", "locs", "time_windows",
               "durations", "current_time"),
    "sdvrp": ("w_cap", "dyn_vectors", "demand_state", "used_capacity", "vehicle_capacity"),
    "mtsp": ("mtsp_ctx", "num_agents", "locs", "used_capacity", "current_time", "step_i"),
    "pdp": ("visited", "to_deliver", "step_i"),
    "pctsp": ("w_cap", "demand", "used_capacity", "vehicle_capacity", "step_i", "visited"),
    "op": ("w_cap", "locs", "max_length", "used_capacity", "step_i", "visited"),
}


def test_variant_and_row_groups_equal_the_record():
    rec = np.load(G.GOLDEN)
    assert rec["axes"].tolist() == list(G.AXES) and rec["nodes"].tolist() == list(G.NODES)
    assert rec["steps"].tolist() == [0 if s is None else s for s in G.STEPS] and rec["flags"].tolist() == list(G.FLAGS)
    assert rec["batches"].tolist() == [list(b) for b in G.BATCHES]
    assert rec["variant"].dtype == np.int8 and rec["row_groups"].dtype == np.int8
    variant, groups = G.table()
    assert variant.shape == rec["variant"].shape == (8, 3, 10, 4, 10, 6, 6)
    for name, got, want in (("variant", variant, rec["variant"]), ("row_groups", groups, rec["row_groups"])):
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{name}: {len(bad)} entries differ, first at {dict(zip(G.AXES, bad[0].tolist()))}: " \
                              f"{got[tuple(bad[0])]} != recorded {want[tuple(bad[0])]}"
    # the grid reaches every variant and both "no kernel" answers
    assert set(np.unique(variant).tolist()) == {-1, 1, 2, 3, 4, 5} and -1 in groups and 0 in groups


def _pointers(struct):
    return [name for name, kind in struct._fields_ if kind is ctypes.c_void_p]


def _decode_args(env):
    """Every slot set, every scalar valid, except the variant: refused by the last requirement before the launch."""
    a = _lib.AmDecodeArgs()
    for name in _pointers(_lib.AmDecodeArgs):
        setattr(a, name, DUMMY)
    a.env, a.B, a.B_inst, a.N, a.mode, a.max_steps = env, 64, 64, 21, _lib.DECODE_GREEDY, 4  # (PDP: an even customer count)
    a.tanh_clipping, a.temperature, a.cache_dtype, a.variant = 10.0, 1.0, _lib.DT_BF16, 99
    a.kvl_row_stride, a.kvl_batch_stride = 128, 21 * 128
    a.t0, a.out_stride, a.top_p, a.kept_words = 0, 4, 1.0, 4
    return a


def _refused(fn, a):
    assert fn(ctypes.byref(a), None) == ERR_ARG
    return _lib.lib().rl4co_last_error()


@pytest.mark.parametrize("env_name", list(ENV_IDS))
def test_decode_requires_each_environments_slots(env_name):
    decode = _lib.lib().rl4co_am_decode
    assert b"a.variant" in _refused(decode, _decode_args(ENV_IDS[env_name]))  # all slots there: only the variant is wrong
    for slot in REQUIRED[env_name]:
        a = _decode_args(ENV_IDS[env_name])
        setattr(a, slot, None)
        msg = _refused(decode, a)
        assert b"a.variant" not in msg and ("a.%s" % slot).encode() in msg, (slot, msg)


def test_beam_admits_tsp_and_cvrp_with_all_slots():
    beam = _lib.lib().rl4co_am_decode_beam
    for env in range(8):
        a = _lib.AmDecodeBeamArgs()
        for name in _pointers(_lib.AmDecodeBeamArgs):
            setattr(a, name, DUMMY)
        a.env, a.B_inst, a.N, a.beam_width, a.max_steps, a.out_stride = env, 64, 21, 1, 20, 21
        a.cache_dtype, a.tanh_clipping, a.temperature = _lib.DT_BF16, 10.0, 1.0
        a.kvl_row_stride, a.kvl_batch_stride = 128, 21 * 128
        msg = _refused(beam, a)
        assert (b"beam_width >= 2" in msg) if env in (0, 1) else (b"a.env" in msg), (env, msg)


def test_an_id_that_is_no_admitted_environment_is_refused():
    handle = _lib.lib()
    for env in NO_ENV:
        assert b"a.env" in _refused(handle.rl4co_am_decode, _decode_args(env))
        b = _lib.AmDecodeBeamArgs()
        b.env, b.beam_width = env, 1
        assert b"a.env" in _refused(handle.rl4co_am_decode_beam, b)
    # the teacher-forced backward: its six environments pass the range requirement (the next one refuses the empty
    # struct), the decode-only ones and the ids beyond do not
    for env in tuple(range(8)) + NO_ENV:
        t = AmTeacherArgs()
        t.env = env
        msg = _refused(handle.rl4co_am_teacher_backward, t)
        assert (b"a.env" in msg) == (env not in range(6)), (env, msg)
        assert handle.rl4co_am_teacher_variant(ctypes.byref(t)) == -1
