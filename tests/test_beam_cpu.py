"""Beam search without a device: the torch restatement of the reference's bookkeeping against torch.topk and a brute-force
enumeration, the C-ABI of the beam entry (header, ctypes mirror, prototypes, the width limit), and the policy's parsing and
the refusals that need no GPU."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from tests import beam_ref

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "rl4co_amd.h").read_text()


def _c_fields(struct_name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct_name, struct_name), HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)\s*;", body)


def test_struct_and_prototypes():
    from rl4co_amd import _lib

    fields = _c_fields("rl4co_am_decode_beam_args")
    assert fields == [f[0] for f in _lib.AmDecodeBeamArgs._fields_]
    for must in ("beam_width", "max_steps", "actions", "logps", "parents", "cum_logp", "err", "steps_summary", "glimpse_key",
                 "ctx_cur", "action_mask", "first_node", "current_node", "step_i", "done", "demand", "used_capacity",
                 "vehicle_capacity", "visited"):
        assert must in fields, must
    assert ctypes.sizeof(_lib.AmDecodeBeamArgs) % 8 == 0
    assert re.search(r"int rl4co_am_decode_beam\(const rl4co_am_decode_beam_args\* args, void\* stream\);", HEADER)
    assert _lib.SYMBOLS["rl4co_am_decode_beam"] == (ctypes.c_int, [ctypes.POINTER(_lib.AmDecodeBeamArgs), ctypes.c_void_p])
    # a new sticky bit above the existing ones, which keep their values
    assert _lib.EBIT_BEAM_INFEASIBLE == 131072 and "#define RL4CO_EBIT_BEAM_INFEASIBLE 131072" in HEADER
    assert (_lib.EBIT_INFEASIBLE, _lib.EBIT_MAX_STEPS, _lib.EBIT_TW_DEADLINE) == (2, 16, 65536)
    with pytest.raises(AssertionError, match="infeasible action selected"):
        _lib.raise_for_error_bits(_lib.EBIT_BEAM_INFEASIBLE)


def test_max_width_is_declared_and_follows_the_lds_budget():
    from rl4co_amd import _lib
    from rl4co_amd import kernels as K

    assert re.search(r"int rl4co_am_decode_beam_max_width\(int N\);", HEADER)
    assert _lib.SYMBOLS["rl4co_am_decode_beam_max_width"] == (ctypes.c_int, [ctypes.c_int])

    def lds(w, n):  # the byte count of the am_decode_beam.hip header
        nw, np_ = (n + 3) & ~3, (n + 63) & ~63
        return 8 * w * nw + 56 * w + 152 * np_ + 208 + 256  # (+ the kernels' static LDS)

    for n in (2, 20, 21, 65, 100, 128, 500, 1024):
        w = K.beam_max_width(n)
        assert w * n <= 16384 and lds(w, n) <= 160 * 1024
        assert (w + 1) * n > 16384 or lds(w + 1, n) > 160 * 1024
    assert K.beam_max_width(100) >= 100  # the reference's default width at the headline size
    assert K.beam_max_width(1) == 0 and K.beam_max_width(1025) == 0
    # the entry refuses on the host: no width 1 (decoding.py:494), nothing beyond the limit
    a = _lib.AmDecodeBeamArgs()
    a.env, a.B_inst, a.N, a.beam_width, a.max_steps, a.out_stride = 0, 1, 20, 1, 19, 20
    assert _lib.lib().rl4co_am_decode_beam(ctypes.byref(a), None) == 1  # RL4CO_ERR_ARG
    assert b"beam_width >= 2" in _lib.lib().rl4co_last_error()
    a.beam_width = K.beam_max_width(20) + 1
    assert _lib.lib().rl4co_am_decode_beam(ctypes.byref(a), None) == 1
    assert b"max_width" in _lib.lib().rl4co_last_error()


def test_policy_parses_beam_search_and_refuses_without_a_device():
    from rl4co_amd import policy as P
    from rl4co_amd.envs import get_env
    from rl4co_amd.tensordict import TensorDict

    assert P._parse_decode_type("beam_search") == ("beam_search", False)
    td = TensorDict({"locs": torch.rand(2, 9, 2), "action_mask": torch.ones(2, 9, dtype=torch.bool)}, batch_size=[2])
    for name in ("op", "pctsp", "pdp", "cvrptw", "sdvrp", "mtsp"):
        pol = P.AttentionModelPolicy(env_name=name).eval()
        with pytest.raises(NotImplementedError, match="beam search"):
            pol(td, get_env(name), phase="test", decode_type="beam_search", beam_width=4)
    env = get_env("tsp")
    with pytest.raises(NotImplementedError, match="fold=False"):
        P.AttentionModelPolicy(env_name="tsp", fold=False).eval()(td, env, phase="test", decode_type="beam_search", beam_width=4)
    pol = P.AttentionModelPolicy(env_name="tsp").eval()
    with pytest.raises(NotImplementedError, match="top-k / top-p"):
        pol(td, env, phase="test", decode_type="beam_search", beam_width=4, top_k=3)
    with pytest.raises(NotImplementedError, match="top-k / top-p"):
        pol(td, env, phase="test", decode_type="beam_search", beam_width=4, top_p=0.9)
    with pytest.raises(NotImplementedError, match="captured graphs"):
        pol(td, env, phase="test", decode_type="beam_search", beam_width=4, _defer_finish=True)
    with pytest.raises(NotImplementedError, match="MI355X"):  # CPU tensors: the strategy lives in the kernel alone
        pol(td, env, phase="test", decode_type="beam_search", beam_width=4)


@pytest.mark.parametrize("b,n,w", [(3, 7, 2), (4, 9, 5), (2, 6, 6)])
def test_restatement_against_enumeration(b, n, w):
    """Random log-prob rows with -inf entries and exact ties: the restated step keeps the W best (parent, node) pairs in
    descending order, equal values by flat index; where no ties exist it is torch.topk; backtracking the recorded steps
    reproduces the sequence of every final beam as enumerated by following its parents by hand."""
    g = torch.Generator().manual_seed(100 * n + w)
    steps = 5
    cum = torch.zeros(w * b)
    nodes, lps, pars = [torch.zeros(w * b, dtype=torch.int64)], [torch.zeros(w * b)], [torch.zeros(w * b, dtype=torch.int32)]
    for t in range(steps):
        lp = torch.randint(-6, 0, (w * b, n), generator=g).float() * 0.5  # coarse values: many exact ties
        if t % 2:
            lp = lp + torch.rand(w * b, n, generator=g) * 1e-3            # ... and steps without
        lp[torch.rand(w * b, n, generator=g) < 0.3] = float("-inf")
        lp[:, 0] = lp[:, 0].clamp(min=-5.0)  # at least one finite entry per row
        node, par, val = beam_ref.make_beam_step(lp, cum, w)
        stacked = torch.cat((lp + cum[:, None]).split(b), 1)
        for i in range(b):
            order = sorted(range(w * n), key=lambda k: (-stacked[i, k].item(), k))[:w]
            assert [int(par[j * b + i]) * n + int(node[j * b + i]) for j in range(w)] == order
            assert torch.equal(val[i::b], stacked[i, order])
        assert torch.equal(torch.hstack(torch.unbind(torch.topk(stacked, w, dim=1)[0], 1)), val)  # torch.topk's values
        nodes.append(node), lps.append(lp[torch.arange(b).repeat(w) + par.long() * b, node]), pars.append(par)
        cum = val
    sn, sl, sp = torch.stack(nodes, 1), torch.stack(lps, 1), torch.stack(pars, 1)
    acts, alp = beam_ref.backtrack(sn, sl, sp, w)
    for j in range(w):
        for i in range(b):
            c, seq = j, []
            for k in range(steps, -1, -1):
                seq.append(int(sn[c * b + i, k]))
                c = int(sp[c * b + i, k])
            assert acts[j * b + i].tolist() == seq[::-1]
    assert torch.equal(alp.sum(1), cum) or torch.allclose(alp.sum(1), cum, atol=1e-5)  # the aligned log-probs add up to the kept values
    # best beam: the largest reward, the lowest beam on ties
    rew = torch.tensor([1.0, 3.0, 3.0, 2.0]).repeat_interleave(b)[: 4 * b]
    assert beam_ref.select_best_beam(rew, 4).tolist() == [b + i for i in range(b)]


@pytest.mark.parametrize("case", list(beam_ref.CASES))
def test_restatement_reproduces_the_records(case):
    """The reference's own beam-search rollouts (tests/golden/reference/beam_*.npz): from the recorded per-step log-prob
    rows the restated step keeps exactly the reference's (parent, node) pairs and cumulative values; backtracking the
    recorded per-step selections gives exactly the recorded aligned beams; the best-beam rows are the recorded ones."""
    rec = beam_ref.record(case)
    _, _, w, _ = beam_ref.CASES[case]
    b, full = beam_ref.BATCH, beam_ref.FULL
    rows = torch.arange(w).repeat_interleave(full) * b + torch.arange(full).repeat(w)
    sn, sp = rec["step_nodes"].long(), rec["parents"].to(torch.int32)
    assert not sp[:, 0].any() and sn.shape == rec["actions"].shape
    step_lp = torch.zeros(w * full, sn.shape[1])
    for t in range(rec["full_rows"].shape[0]):
        node, par, val = beam_ref.make_beam_step(rec["full_rows"][t], rec["full_cum_in"][t], w)
        assert torch.equal(node, sn[rows, t + 1]) and torch.equal(par, sp[rows, t + 1]), t
        assert torch.equal(val, rec["full_cum"][t]), t
        assert torch.equal(val.view(w, full)[-1], rec["kept_min"][:full, t]), t
        step_lp[:, t + 1] = rec["full_rows"][t][torch.arange(full).repeat(w) + par.long() * full, node]
    acts, _ = beam_ref.backtrack(sn, torch.zeros(sn.shape), sp, w)
    assert torch.equal(acts, rec["actions"].long())
    # the aligned log-probs of the instances whose rows are kept
    _, alp = beam_ref.backtrack(sn[rows], step_lp, sp[rows], w)
    assert torch.equal(alp, rec["log_likelihood"][rows])
    best = beam_ref.select_best_beam(rec["reward"], w)
    assert torch.equal(rec["actions"][best], rec["best_actions"]) and torch.equal(rec["reward"][best], rec["best_reward"])
    # the start nodes are select_start_nodes' (ops.py:128-161), beam-major
    n_loc = 20
    want = torch.arange(w).repeat_interleave(b) % n_loc + (0 if case.startswith("tsp") else 1)
    assert torch.equal(sn[:, 0], want)
