"""Beam search on the MI355X (csrc/am_decode_beam.hip): every step's selection against the torch restatement on the log-prob
rows the existing STREAM kernel reports for the same beams (no tolerance), the aligned outputs against the torch backtrack
and against ``am_decode(mode="evaluate", variant="stream")`` bit for bit, the final state against the CPU restatements of
the environments, the policy surface, refusals and limits."""
from functools import lru_cache

import pytest
import torch

from tests import beam_ref

pytestmark = pytest.mark.gpu

B = 8
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CASES = [("tsp", n, w) for n in (21, 65) for w in (2, 5, 16)] + [("cvrp", 21, 8)]  # 65 crosses the 64-entry LDS pad


def _random_cache(env, b, n, dtype, seed=0):
    from rl4co_amd.cache import FoldedCache

    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    tsp = env == "tsp"
    return FoldedCache(env_name=env, kvl=(r(3, b, n, 128) * 0.5).to(dtype).cuda(), ctx_first=r(b, n, 128).cuda() if tsp else None,
                       ctx_cur=r(b, n, 128).cuda(), q_bias=r(b, 128).cuda(), q_step0=r(128).cuda() if tsp else None,
                       w_cap=None if tsp else r(128).cuda())


def _start_state(env, n, w, start=None):
    if env == "tsp":
        return beam_ref.tsp_state(B, n, w, start)
    g = torch.Generator().manual_seed(n)
    demand = torch.randint(1, 10, (B, n - 1), generator=g).float() / 30.0  # several returns to the depot: ragged horizons
    return beam_ref.cvrp_state(demand, w, start)


def _cuda(st):
    return {k: v.clone().cuda() for k, v in st.items()}


@lru_cache(maxsize=None)
def _run(env, n, w, dt):
    """One launch of the beam kernel on a random cache; every output on the CPU."""
    from rl4co_amd import kernels as K

    cache = _random_cache(env, B, n, DTYPES[dt], seed=n + w)
    st0, start = _start_state(env, n, w)
    st = _cuda(st0)
    t_len = n if env == "tsp" else 2 * n
    rows = w * B
    # (aligned buffers zeroed as the policy does: an instance that finishes before the batch's last step keeps the padding)
    out = {"actions": torch.zeros((rows, t_len), dtype=torch.int64), "logps": torch.zeros((rows, t_len)),
           "step_nodes": torch.full((rows, t_len), -7, dtype=torch.int32), "step_logps": torch.full((rows, t_len), 7.0),
           "parents": torch.full((rows, t_len), -7, dtype=torch.int32), "cum_logp": torch.full((rows, t_len), 7.0)}
    out = {k: v.cuda() for k, v in out.items()}
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    K.am_decode_beam(cache, st, w, t_len - 1, err=status[:1], steps_summary=status[2:4], **out)
    torch.cuda.synchronize()
    return cache, st0, start, {k: v.cpu() for k, v in st.items()}, {k: v.cpu() for k, v in out.items()}, status.cpu().tolist()


def _single_step_rows(cache, env, st_cpu):
    """The full log-prob row of every beam row's NEXT step from the existing STREAM kernel (one single-step launch)."""
    from rl4co_amd import kernels as K

    st = _cuda(st_cpu)
    rows, n = st["action_mask"].shape
    acts = torch.zeros((rows, 1), dtype=torch.int64, device="cuda")
    lps = torch.zeros((rows, 1), device="cuda")
    alp = torch.zeros((rows, 1, n), device="cuda")
    K.am_decode(cache, st, mode="greedy", max_steps=1, actions=acts, logps=lps, err=K.new_error_word("cuda"), all_logps=alp,
                variant="stream")
    return alp[:, 0].cpu()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("env,n,w", CASES)
def test_selection_is_exact(env, n, w, dt):
    cache, st0, start, st_end, out, status = _run(env, n, w, dt)
    assert status[0] == 0, hex(status[0])
    t_used = 1 + status[2]
    assert t_used == n if env == "tsp" else n <= t_used <= 2 * n
    sn, sl, sp, sc = (out[k][:, :t_used].clone() for k in ("step_nodes", "step_logps", "parents", "cum_logp"))
    # column 0: the start node, log-prob 0, parent 0
    assert torch.equal(sn[:, 0].long(), start) and not sl[:, 0].any() and not sp[:, 0].any() and not sc[:, 0].any()
    st = {k: v.clone() for k, v in st0.items()}
    cum = torch.zeros(w * B)
    inst = torch.arange(B).repeat(w)
    ident = torch.arange(w, dtype=torch.int32).repeat_interleave(B)
    for t in range(1, t_used):
        lp = _single_step_rows(cache, env, st)  # [W*B, N] of the parents, from the existing kernel
        node, par, val = beam_ref.make_beam_step(lp, cum, w)
        # an instance whose beams are all done has left the kernel (one workgroup per instance): its columns stay unwritten.
        # The reference pads such steps: every beam keeps itself as parent, takes the depot at log-prob 0, cum unchanged
        fin = st["done"].view(w, B).all(0).repeat(w)
        if bool(fin.any()):
            assert torch.equal(par[fin], ident[fin]) and not node[fin].any() and torch.equal(val[fin], cum[fin])
            assert bool((sn[fin, t] == -7).all()) and bool((sp[fin, t] == -7).all()) and bool((sc[fin, t] == 7.0).all())
            sn[fin, t], sp[fin, t], sc[fin, t], sl[fin, t] = 0, ident[fin], cum[fin], 0.0
        before = {k: v.clone() for k, v in st.items()}
        # the kept set is the descending top-W under the stated tie rule (so every rejected candidate is <= the smallest
        # kept one), bit for bit; the chosen log-prob is the parent's row entry
        assert torch.equal(sp[:, t], par), t
        assert torch.equal(sn[:, t].long(), node), t
        assert torch.equal(sc[:, t], val), t
        kept = val.view(w, B)
        assert bool((kept[:-1] >= kept[1:]).all()) and bool(torch.isfinite(kept).all())
        stacked = torch.cat((lp + cum[:, None]).split(B), 1)
        assert bool(((stacked <= kept[-1][:, None]).sum(1) >= w * n - w).all())
        prow = inst + par.long() * B
        assert torch.equal(sl[:, t], lp[prow, node]), t
        assert bool(st["action_mask"][prow, node].all()), t  # feasible in the parent's mask
        st = beam_ref.reparent(st, env, par, w)
        beam_ref.env_step(env, st, node)
        for k, v in st.items():  # (the finished instances' rows stay as the kernel left them)
            if k != "demand":
                v[fin] = before[k][fin]
        cum = val
    # the final state is the CPU restatement's along the beams
    for k, v in st.items():
        assert torch.equal(st_end[k].to(v.dtype).view(v.shape), v), k
    assert bool(st["done"].all())
    # aligned outputs = the torch backtrack of the raw per-step outputs, bit for bit; nothing behind the used columns
    acts, alp = beam_ref.backtrack(sn.long(), sl, sp, w)
    assert torch.equal(out["actions"][:, :t_used], acts) and torch.equal(out["logps"][:, :t_used], alp)
    assert not out["actions"][:, t_used:].any() and not out["logps"][:, t_used:].any()
    for k in ("step_nodes", "parents"):
        assert bool((out[k][:, t_used:] == -7).all())


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("env,n,w", CASES)
def test_logps_equal_stream_evaluate(env, n, w, dt):
    """The aligned log-probs of every final beam are what the existing STREAM kernel reports for those actions."""
    from rl4co_amd import kernels as K

    cache, st0, start, _, out, status = _run(env, n, w, dt)
    t_used = 1 + status[2]
    forced = out["actions"][:, :t_used].contiguous().cuda()
    acts, lps = torch.zeros_like(forced), torch.zeros(forced.shape, device="cuda")
    err = K.new_error_word("cuda")
    # (a final beam starts at its root ancestor's start node, not at its own row's)
    st_eval, _ = _start_state(env, n, w, out["actions"][:, 0].clone())
    K.am_decode(cache, _cuda(st_eval), mode="evaluate", max_steps=t_used - 1, t0=1, actions=acts, logps=lps, err=err,
                forced_actions=forced, variant="stream")
    assert int(err.item()) == 0
    assert torch.equal(acts[:, 1:].cpu(), out["actions"][:, 1:t_used])
    assert torch.equal(lps[:, 1:].cpu(), out["logps"][:, 1:t_used])  # (a finished CVRP beam: 0 on both sides)


def _policy(env_name, **kw):
    from rl4co_amd.policy import AttentionModelPolicy

    torch.manual_seed(7)
    return AttentionModelPolicy(env_name=env_name, **kw).eval().cuda()


def _batch(env_name, n, b, seed=11):
    from rl4co_amd.envs import get_env

    env = get_env(env_name, generator_params=dict(num_loc=n, device="cuda"), device="cuda", check_solution=True)
    torch.manual_seed(seed)
    return env, env.reset(env.generator(batch_size=[b]))


@pytest.mark.parametrize("env_name", ["tsp", "cvrp"])
def test_policy_surface(env_name):
    env, td = _batch(env_name, 20, 6)
    pol = _policy(env_name)
    allb = pol(td.clone(), env, phase="test", decode_type="beam_search", beam_width=5, select_best=False)
    t = allb["actions"].shape[1]
    assert allb["actions"].shape == (30, t) and allb["reward"].shape == (30,) and allb["log_likelihood"].shape == (30,)
    assert not allb["log_likelihood"].requires_grad
    best = pol(td.clone(), env, phase="test", decode_type="beam_search", beam_width=5)  # select_best=True is the default
    assert best["actions"].shape == (6, t) and best["reward"].shape == (6,)
    per = allb["reward"].view(5, 6)
    assert torch.equal(best["reward"], per.max(0).values)
    rows = beam_ref.select_best_beam(allb["reward"], 5)
    assert torch.equal(best["actions"], allb["actions"][rows]) and torch.equal(best["log_likelihood"], allb["log_likelihood"][rows])
    steps = pol(td.clone(), env, phase="train", decode_type="beam_search", beam_width=5, select_best=False,
                return_sum_log_likelihood=False, return_actions=False, calc_reward=False)
    assert "actions" not in steps and steps["log_likelihood"].shape == (30, t) and not steps["log_likelihood"].requires_grad
    assert torch.equal(steps["log_likelihood"].sum(1), allb["log_likelihood"])
    if env_name == "tsp":  # beam_width=None: env.get_num_starts = N beams
        assert pol(td.clone(), env, phase="test", decode_type="beam_search", select_best=False)["actions"].shape == (6 * 20, 20)


def test_headline_size_runs():
    """W = N = 100, bf16 planes: the reference's default width at TSP-100."""
    env, td = _batch("tsp", 100, 4)
    pol = _policy("tsp")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = pol(td.clone(), env, phase="test", decode_type="beam_search", beam_width=100, select_best=False)
    assert out["actions"].shape == (400, 100)
    env.check_solution_validity(td, out["actions"])
    assert bool(torch.isfinite(out["reward"]).all())


def test_refusals_and_limits():
    from rl4co_amd import _lib
    from rl4co_amd import kernels as K
    from rl4co_amd.graph import GraphedRollout

    env, td = _batch("tsp", 20, 4)
    pol = _policy("tsp")
    with pytest.raises(AssertionError, match="beam width must be larger than 1"):
        pol(td.clone(), env, phase="test", decode_type="beam_search", beam_width=1)
    limit = K.beam_max_width(20)
    with pytest.raises(NotImplementedError, match=str(limit)):
        pol(td.clone(), env, phase="test", decode_type="beam_search", beam_width=limit + 1)
    with pytest.raises(NotImplementedError, match="top-k / top-p"):
        pol(td.clone(), env, phase="test", decode_type="beam_search", beam_width=4, top_k=3)
    with pytest.raises(NotImplementedError, match="does not take"):
        pol(td.clone(), env, phase="test", decode_type="beam_search", beam_width=4, num_starts=4)
    with pytest.raises(NotImplementedError, match="entropy"):
        pol(td.clone(), env, phase="test", decode_type="beam_search", beam_width=4, return_entropy=True)
    with pytest.raises(NotImplementedError, match="fold=False"):
        _policy("tsp", fold=False)(td.clone(), env, phase="test", decode_type="beam_search", beam_width=4)
    with pytest.raises(NotImplementedError, match="captured graphs"):
        GraphedRollout(pol, env, td.clone(), decode_type="beam_search", beam_width=4)
    for name in ("op", "pctsp", "pdp", "cvrptw", "sdvrp", "mtsp"):
        with pytest.raises(NotImplementedError, match="beam search"):
            _policy(name)(td.clone(), name, phase="test", decode_type="beam_search", beam_width=4)
    # max_steps too short: the sticky bit, and nothing behind the given columns
    n, w = 21, 5
    cache = _random_cache("tsp", B, n, torch.bfloat16)
    st0, _ = beam_ref.tsp_state(B, n, w)
    rows, t_len = w * B, n
    out = {k: torch.full((rows, t_len), -7, dtype=dt, device="cuda")  # (one instance-level horizon on TSP: sentinels everywhere)
           for k, dt in (("actions", torch.int64), ("logps", torch.float32), ("step_nodes", torch.int32),
                         ("step_logps", torch.float32), ("parents", torch.int32), ("cum_logp", torch.float32))}
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    short = 6
    with pytest.raises(ValueError):
        K.am_decode_beam(cache, _cuda(st0), w, t_len, err=status[:1], **out)  # more steps than columns behind the start
    K.am_decode_beam(cache, _cuda(st0), w, short, err=status[:1], steps_summary=status[2:4], **out)
    torch.cuda.synchronize()
    assert status[0].item() == _lib.EBIT_MAX_STEPS and status[2].item() == short
    for v in out.values():
        assert bool((v[:, short + 1:] == -7).all()) and bool((v[:, : short + 1] != -7).all())
    with pytest.raises(AssertionError, match="Exceeded maximum number of steps"):
        _lib.raise_for_error_bits(status[0].item())


# ---- parity with the reference's own beam-search rollouts (tests/golden/reference/beam_*.npz) ---------------------------
def _record_td(rec, env_name):
    from rl4co_amd.envs import get_env
    from rl4co_amd.tensordict import TensorDict

    b, num_loc = rec["in_locs"].shape[:2]
    env = get_env(env_name, generator_params=dict(num_loc=num_loc, device="cuda"), device="cuda")
    data = {k[3:]: v.cuda() for k, v in rec.items() if k.startswith("in_")}
    return env, env.reset(TensorDict(data, batch_size=[b]))


@pytest.mark.parametrize("case", list(beam_ref.CASES))
def test_parity_with_the_records(case):
    """The recorder's weights, fp32 planes, fp32 encoder. Per instance the set of final beams is the record's; at most 1/4
    of the instances may differ, each at a near-tie: at the first step whose selections differ, the W-th kept cumulative
    log-probs lie within 2 * STEP_TOL * (t + 1) (sums of t + 1 terms). Agreeing instances: rewards bit for bit, summed
    log-likelihood within ll_rtol, the select_best=True row the record's."""
    from rl4co_amd.policy import AttentionModelPolicy
    from tests.helpers import WEIGHT_SEED, ll_rtol
    from tests.mtsp_ref import STEP_TOL

    env_name, _, w, _ = beam_ref.CASES[case]
    rec = beam_ref.record(case)
    b = beam_ref.BATCH
    torch.manual_seed(WEIGHT_SEED)
    pol = AttentionModelPolicy(env_name, cache_dtype=torch.float32).cuda().eval()
    env, td = _record_td(rec, env_name)
    with torch.inference_mode():
        out = pol(td.clone(), env, phase="test", decode_type="beam_search", beam_width=w, select_best=False,
                  return_sum_log_likelihood=False)
        raw = {k: v.cpu() for k, v in pol.last_beam_steps.items()}
        best = pol(td.clone(), env, phase="test", decode_type="beam_search", beam_width=w)
    acts, lls, rew = out["actions"].cpu(), out["log_likelihood"].cpu(), out["reward"].cpu()
    strip = lambda r: tuple(r[: max(i for i, a in enumerate(r) if a != 0 or i == 0) + 1])  # noqa: E731
    got_sets, want_sets = beam_ref.beam_sets(acts, w), beam_ref.beam_sets(rec["actions"].long(), w)
    differ = [i for i in range(b) if got_sets[i] != want_sets[i]]
    print(f"{case}: {len(differ)} of {b} instances differ from the record: {differ}")
    assert len(differ) <= b // 4
    t_rec = rec["step_nodes"].shape[1]
    for i in differ:  # a near-tie at the first step whose (parent, node) selections differ
        mine = torch.stack((raw["parents"][i::b, :t_rec], raw["step_nodes"][i::b, :t_rec])).long()
        theirs = torch.stack((rec["parents"][i::b], rec["step_nodes"][i::b])).long()
        own = int((raw["cum_logp"][i::b] != 0).any(0).nonzero().max()) + 1  # the instance's own horizon (columns written)
        k = min(mine.shape[2], theirs.shape[2], own)
        col = (mine[:, :, :k] != theirs[:, :, :k]).any(0).any(0).nonzero()
        assert col.numel() > 0, i
        t = int(col[0])  # column t = decode step t (column 0 is the start): t + 1 terms in the sum
        gap = abs(float(raw["cum_logp"][(w - 1) * b + i, t]) - float(rec["kept_min"][i, t - 1]))
        print(f"  instance {i}: first differing step {t}, gap of the W-th kept cumulative log-prob {gap:.3e}")
        assert gap <= 2 * STEP_TOL * (t + 1), (i, t, gap)
    worst = 0.0
    for i in range(b):
        if i in differ:
            continue
        theirs = {strip(rec["actions"][j * b + i].tolist()): j * b + i for j in range(w)}
        for j in range(w):
            r = theirs[strip(acts[j * b + i].tolist())]
            assert rew[j * b + i].item() == rec["reward"][r].item(), (i, j)
            want = rec["log_likelihood"][r]
            k = min(want.shape[0], lls.shape[1])
            worst = max(worst, float((lls[j * b + i, :k] - want[:k]).abs().max()))
            assert abs(float(lls[j * b + i].sum()) - float(want.sum())) <= ll_rtol("cvrp", gpu=True) * abs(float(want.sum())), (i, j)
        assert strip(best["actions"][i].cpu().tolist()) == strip(rec["best_actions"][i].long().tolist()), i
        assert best["reward"][i].item() == rec["best_reward"][i].item(), i
    print(f"{case}: largest per-step log-prob deviation from the record {worst:.3e}")


def test_launch_at_the_width_limit():
    """An LDS-bound size: the kernel launches at exactly beam_max_width(n) (dynamic + static LDS within 160 KiB)."""
    from rl4co_amd import kernels as K

    n = 20
    w = K.beam_max_width(n)
    assert w * n < 16384  # (bound by the LDS bytes, not by the candidates per thread)
    cache = _random_cache("tsp", 1, n, torch.bfloat16)
    rows = w
    st, start = beam_ref.tsp_state(1, n, w)
    out = {k: torch.zeros((rows, n), dtype=dt, device="cuda")
           for k, dt in (("actions", torch.int64), ("logps", torch.float32), ("step_nodes", torch.int32),
                         ("step_logps", torch.float32), ("parents", torch.int32), ("cum_logp", torch.float32))}
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    K.am_decode_beam(cache, _cuda(st), w, n - 1, err=status[:1], steps_summary=status[2:4], **out)
    torch.cuda.synchronize()
    assert status[2].item() == n - 1
    acts = out["actions"].cpu()
    assert bool((acts.sort(1).values == torch.arange(n)).all())  # every final beam is a tour


def test_fewer_finite_candidates_than_beams_sets_the_bit():
    """Two of five beams enter with no feasible node and not done: 3 * 1 finite candidates < 5 beams -> the kernel keeps
    -inf candidates and says so (the reference's "infeasible action selected")."""
    from rl4co_amd import _lib
    from rl4co_amd import kernels as K

    n, w, b = 21, 5, 2
    cache = _random_cache("tsp", b, n, torch.float32)
    st, _ = beam_ref.tsp_state(b, n, w)
    st["action_mask"][:] = False
    st["action_mask"][: 3 * b, 7] = True  # beams 0..2: node 7 alone; beams 3, 4: nothing
    out = {k: torch.zeros((w * b, n), dtype=dt, device="cuda")
           for k, dt in (("actions", torch.int64), ("logps", torch.float32), ("step_nodes", torch.int32),
                         ("step_logps", torch.float32), ("parents", torch.int32), ("cum_logp", torch.float32))}
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    K.am_decode_beam(cache, _cuda(st), w, 1, err=status[:1], steps_summary=status[2:4], **out)
    torch.cuda.synchronize()
    assert status[0].item() & _lib.EBIT_BEAM_INFEASIBLE
    cum = out["cum_logp"][:, 1].cpu().view(w, b)
    assert bool((cum[:3] == 0).all()) and bool(torch.isinf(cum[3:]).all())  # the finite candidates first
    assert bool((out["step_nodes"][: 3 * b, 1] == 7).all())
    with pytest.raises(AssertionError, match="infeasible action selected"):
        _lib.raise_for_error_bits(status[0].item() & _lib.EBIT_BEAM_INFEASIBLE)
