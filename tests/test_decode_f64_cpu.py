"""The float64 decode-step oracle (tests/decode_f64_ref.py) proven without a GPU, before it judges the kernels
(tests/test_gpu_decode_f64.py): against the reference decoder's algebra evaluated in float64 on the unfolded decoder,
against the reference's recorded rollouts, and against the seeded mistakes the GPU test is meant to catch.

The fold is exact algebra only where it is evaluated exactly: ``tests.helpers.fold_cache`` rounds the planes and tables to
fp32 (one fp32 GEMM each), which alone moves a log-prob by ~1e-7. So the 1e-10 comparison folds in float64 (the formulas of
rl4co_amd/cache.py on widened weights), and the fp32 fold of ``fold_cache`` is compared within STEP_TOL — the class of
deviation (fp32, another operation order) that bound was measured for.

The second half of the file does the same for the six environments of the C specified-order oracle, and holds that oracle to
the restatement at the sizes where the kernels change shape (tests/test_gpu_decode_edges.py is the GPU side)."""
import copy
from dataclasses import replace

import pytest
import torch

from tests import decode_f64_ref as D
from tests import mtsp_ref, sdvrp_ref
from tests.helpers import WEIGHT_SEED, fold_cache

ENVS = ["sdvrp", "mtsp"]
RECORDS = [("sdvrp", c) for c in sdvrp_ref.CASES] + [("mtsp", c) for c in mtsp_ref.CASES]


def _policy(env_name):
    from rl4co_amd.policy import AttentionModelPolicy

    torch.manual_seed(WEIGHT_SEED)
    return AttentionModelPolicy(env_name).eval()


def _record_instances(env_name, rec, rows=None):
    """(encoder input, initial state) of a record's instances."""
    cut = lambda x: x if rows is None else x[:rows]  # noqa: E731
    if env_name == "sdvrp":
        locs = torch.cat((rec["in_depot"][:, None, :], rec["in_locs"]), 1)
        return {"locs": cut(locs), "demand": cut(rec["in_demand"])}, sdvrp_ref.initial_state(cut(rec["in_demand"]))
    return {"locs": cut(rec["in_locs"])}, mtsp_ref.initial_state(cut(rec["in_locs"]), cut(rec["in_num_agents"]))


def _fold_f64(pol, env_name, h):
    """rl4co_amd/cache.py's fold (fold_weights, fold_dynamic, fold_features, the graph context) in float64: exact algebra up
    to float64 rounding."""
    from rl4co_amd.cache import FoldedCache, fold_weights

    w = {k: (None if v is None else v.detach().double()) for k, v in pol.decoder.constant_weights().items()}
    w_node = pol.decoder.project_node_embeddings.weight.detach().double()
    h = h.double()
    blocks = fold_weights(env_name, w_node, w["w_out"], w["w_ctx"])
    kvl = torch.stack([h @ blk.t() for blk in blocks[:3]])
    q_bias = h.mean(1) @ pol.decoder.project_fixed_context.weight.detach().double().t()
    w_cap = dyn = feat = None
    if env_name == "sdvrp":
        w_cap = w["w_ctx"][:, 128].contiguous()
        u = w["w_dyn"].reshape(3, 128)
        dyn = torch.stack((u[0], u[1], w["w_out"].t() @ u[2]))
    else:
        feat = (w["w_ctx"][:, 128:256] @ w["w_feat"]).t().contiguous()
    return FoldedCache(env_name, kvl, None, h @ blocks[3].t(), q_bias, None, w_cap, None, dyn, feat)


@pytest.fixture(scope="module")
def encoded():
    """Per environment: the seeded policy, the first 8 instances of the 20-node record encoded in fp32, a random walk."""
    out = {}
    for env_name in ENVS:
        pol = _policy(env_name)
        rec = D.REFS[env_name].record(f"{env_name}20_greedy")
        td, st0 = _record_instances(env_name, rec, 8)
        with torch.inference_mode():
            h, _ = pol.encoder(td)
        if env_name == "sdvrp":
            acts, final = sdvrp_ref.random_walk(td["demand"], 6 * 21, seed=5)
        else:
            acts, final = mtsp_ref.random_walk(st0["locs"], st0["num_agents"], 2 * 20, seed=5)
        assert bool(final["done"].all())
        acts = acts[:, : int(mtsp_ref.row_lengths(acts).max()) + 2].contiguous()
        dec64 = copy.deepcopy(pol.decoder).double()
        with torch.inference_mode():
            _, want = D.REFS[env_name].decoder_step_logps(dec64, h.double(), st0, acts, all_logps=True)
        out[env_name] = (pol, h.clone(), st0, acts, want)
    return out


@pytest.mark.parametrize("env_name", ENVS)
def test_oracle_equals_the_reference_decoder_in_float64(encoded, env_name):
    pol, h, st0, acts, want = encoded[env_name]
    assert want.dtype == torch.float64
    got = D.rollout(_fold_f64(pol, env_name, h), st0, acts)
    ex = got["executed"]
    assert int(ex.sum()) > 8 * 19 and not bool(ex.all())  # whole rollouts, and padding behind them
    lp, ref = got["logps"][ex], want[ex]
    assert torch.equal(torch.isinf(lp), torch.isinf(ref)) and not bool(torch.isnan(lp).any())
    finite = torch.isfinite(ref)
    dev = float((lp - ref)[finite].abs().max())
    print(f"{env_name}: float64 fold, oracle against the unfolded reference decoder {dev:.3e} over {int(finite.sum())} log-probs")
    assert dev <= 1e-10
    # the fp32 fold the kernels are served with (one rounding per plane / table entry): the records' class of deviation
    got32 = D.rollout(fold_cache(pol, env_name, h), st0, acts)
    lp = got32["logps"][ex]
    assert torch.equal(torch.isinf(lp), torch.isinf(ref))
    dev = float((lp - ref)[finite].abs().max())
    print(f"{env_name}: fp32 fold (tests.helpers.fold_cache) {dev:.3e}")
    assert dev <= D.REFS[env_name].STEP_TOL


@pytest.mark.parametrize("env_name,case", RECORDS)
def test_oracle_equals_the_records(env_name, case):
    ref = D.REFS[env_name]
    rec = ref.record(case)
    pol = _policy(env_name)
    td, st0 = _record_instances(env_name, rec)
    with torch.inference_mode():
        h, _ = pol.encoder(td)
    got = D.rollout(fold_cache(pol, env_name, h), st0, rec["actions"])
    want = rec["log_likelihood"]
    finite = torch.isfinite(want)
    assert bool(finite[got["executed"]].all())
    dev = float((got["chosen"] - want)[finite].abs().max())
    print(f"{case}: oracle against the record, largest per-step deviation {dev:.3e} over {int(finite.sum())} steps")
    assert dev <= ref.STEP_TOL


# ---- the seeded mistakes ---------------------------------------------------------------------------------------------------------
def _swap_rows(t, i, j):
    t = t.clone()
    t[[i, j]] = t[[j, i]]
    return t


MUTATIONS = {  # name -> (cache, oracle arguments) of the mistaken evaluation
    "sdvrp": {
        "dyn[0] <-> dyn[1]": lambda c: (replace(c, dyn=_swap_rows(c.dyn, 0, 1)), {}),
        "dyn[1] <-> dyn[2]": lambda c: (replace(c, dyn=_swap_rows(c.dyn, 1, 2)), {}),
        "capacity column dropped": lambda c: (replace(c, w_cap=torch.zeros_like(c.w_cap)), {}),
        "depot's demand left in the dynamic term": lambda c: (c, dict(zero_depot=False)),
    },
    "mtsp": {
        "feat[0] <-> feat[1]": lambda c: (replace(c, feat=_swap_rows(c.feat, 0, 1)), {}),
        "feat[2] <-> feat[3]": lambda c: (replace(c, feat=_swap_rows(c.feat, 2, 3)), {}),
    },
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("env_name", ENVS)
def test_oracle_reacts_to_every_seeded_mistake(env_name, dtype):
    """The n = 21 case of the GPU test (its cache, instances and walk). Each mistake must move some log-prob of an executed
    step by more than 100 x the GPU test's tolerance for that case. The depot's stored demand is 0 in every state the
    environments produce, so that mistake only shows on a state whose depot column is not 0: the GPU test's ``depot``
    case (-0.25 until the first depot visit returns it to 0 — the transition's own arithmetic), used here too."""
    inst, acts = D.forced_case(env_name, 21, 8)
    cache = D.random_cache(env_name, 8, 21, dtype)
    st0 = D.initial_state(env_name, inst)
    base = D.rollout(cache, st0, acts)
    tol = D.tolerance(env_name, D.fp32_cost(base, D.rollout(cache, st0, acts, step=D.step_f32)))
    for name, mutate in MUTATIONS[env_name].items():
        st = {k: v.clone() for k, v in st0.items()}
        if "depot" in name:
            st["demand_with_depot"][:, 0] = -0.25
            ref = D.rollout(cache, st, acts)
            assert torch.equal(ref["masks"], base["masks"])  # the same walk is feasible
        else:
            ref = base
        c, kw = mutate(cache)
        got = D.rollout(c, st, acts, **kw)
        ok = torch.isfinite(ref["logps"]) & ref["executed"][:, :, None]
        moved = float((got["logps"] - ref["logps"])[ok].abs().max())
        print(f"{env_name} {name}: largest log-prob move {moved:.3e} = {moved / tol:.0f} x the tolerance {tol:.3e}")
        assert moved > 100 * tol, name


# ---- the six environments of the C specified-order oracle ------------------------------------------------------------------------
# The kernels equal oracle/rollout_ref.c bit for bit (tests/test_gpu_decode.py, tests/test_gpu_decode_edges.py), so the C
# oracle within the tolerance of the float64 restatement here is the arithmetic half of the argument, and needs no GPU.
def _fold_f64_six(pol, env_name, h):
    """rl4co_amd/cache.py's fold for the six (fold_weights, the graph context, fold_constants) in float64."""
    from rl4co_amd.cache import FoldedCache, fold_weights
    from rl4co_amd.envspec import spec
    from tests.helpers import decoder_weights

    sp = spec(env_name)
    w = {k: (None if v is None else v.detach().double()) for k, v in decoder_weights(pol).items()}
    h = h.double()
    blocks = fold_weights(env_name, w["w_node"], w["w_out"], w["w_ctx"])
    kvl = torch.stack([h @ blk.t() for blk in blocks[:3]])
    ctx = [h @ blk.t() for blk in blocks[3:]]
    ctx_first, ctx_cur = ctx if sp.ctx_first else (None, ctx[0])
    q_bias = h.mean(1) @ w["w_fixed"].t()
    q_step0 = w["w_ctx"] @ w["w_placeholder"] if sp.ctx_first else None
    w_cap = w["w_ctx"][:, 128].contiguous() if sp.scalar is not None else None
    w_time = w["w_ctx"][:, 129].contiguous() if sp.scalar is not None and sp.scalar.clock else None
    return FoldedCache(env_name, kvl, ctx_first, ctx_cur, q_bias, q_step0, w_cap, w_time)


@pytest.fixture(scope="module")
def encoded_six():
    """Per environment: the seeded reference policy, 8 generated instances of 21 nodes encoded in fp32, the forced walk of
    ``decode_f64_ref.forced_case`` and the reference decoder's float64 log-probs of every step along it (the reference
    environment stepped beside it: it keeps stepping a done row, whose steps are not compared)."""
    from oracle import reference_torch as R
    from tests.helpers import make_policy

    out = {}
    for env_name in D.SIX:
        st0, acts = D.forced_case(env_name, 21, 8)
        env, td = D.six_instances(env_name, 21, 8)
        pol = make_policy(env_name)
        with torch.inference_mode():
            h, _ = pol.encoder(td)
            dec64 = copy.deepcopy(pol.decoder).double()
            cached, cached32 = dec64._precompute_cache(h.double()), pol.decoder._precompute_cache(h)
            want, want32 = [], []
            for t in range(acts.shape[1]):
                logits, mask = dec64(td, cached)
                want.append(R.process_logits(logits, mask, temperature=1.0, tanh_clipping=10.0))
                logits, mask = pol.decoder(td, cached32)  # the reference decoder as it runs: fp32
                want32.append(R.process_logits(logits, mask, temperature=1.0, tanh_clipping=10.0))
                td["action"] = acts[:, t].clone()
                td = env.step(td)
        out[env_name] = (pol, h.clone(), st0, acts, torch.stack(want, 1), torch.stack(want32, 1))
    return out


@pytest.mark.parametrize("env_name", D.SIX)
def test_oracle_equals_the_reference_decoder_in_float64_for_the_six(encoded_six, env_name):
    """The bounds of ``test_oracle_equals_the_reference_decoder_in_float64``: 1e-10 on the float64 fold (this decides whether
    the restatement's algebra is the reference's), and the tolerance's floor (the six's STEP_TOL) on the fp32 fold of
    ``tests.helpers.fold_cache`` the kernels are served with — or 4 x what fp32 costs the reference decoder ITSELF on the same
    steps, where that is more: CVRPTW's clock runs to 480 and its coordinates to 150, unnormalised, so one fp32 rounding of
    a context row moves a log-prob by ~1e-3 whoever evaluates it (tests.helpers.ll_rtol; measured here: the reference's own
    fp32 decoder 1.2e-3 from its float64 self, the fp32 fold 2.1e-3)."""
    pol, h, st0, acts, want, want32 = encoded_six[env_name]
    assert want.dtype == torch.float64
    got = D.rollout(_fold_f64_six(pol, env_name, h), st0, acts)
    ex = got["executed"]
    assert int(ex.sum()) >= 8 * 4  # (an OP row goes home after a few customers)
    lp, ref = got["logps"][ex], want[ex]
    assert torch.equal(torch.isinf(lp), torch.isinf(ref)) and not bool(torch.isnan(lp).any())
    finite = torch.isfinite(ref)
    dev = float((lp - ref)[finite].abs().max())
    print(f"{env_name}: float64 fold, oracle against the unfolded reference decoder {dev:.3e} over {int(finite.sum())} log-probs")
    assert dev <= 1e-10
    got32 = D.rollout(fold_cache(pol, env_name, h), st0, acts)
    lp = got32["logps"][ex]
    assert torch.equal(torch.isinf(lp), torch.isinf(ref))
    dev = float((lp - ref)[finite].abs().max())
    ref32 = float((want32[ex].double() - ref)[finite].abs().max())
    bound = max(D.FLOOR, 4 * ref32)
    print(f"{env_name}: fp32 fold (tests.helpers.fold_cache) {dev:.3e}; the reference decoder in fp32 {ref32:.3e}, bound {bound:.3e}")
    assert dev <= bound


DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DTYPE_IDS = ["f32", "bf16", "f16"]
_SIX_REFS = {}


def _six_reference(case, dtype):
    """(state, walk, cache, float64 rollout, dev32, tolerance) of an edge case, computed once."""
    if (case, dtype) not in _SIX_REFS:
        env_name, n, b = case
        st0, acts = D.forced_case(env_name, n, b)
        cache = D.random_cache(env_name, b, n, dtype)
        want = D.rollout(cache, st0, acts)
        dev32 = D.fp32_cost(want, D.rollout(cache, st0, acts, step=D.step_f32))
        _SIX_REFS[(case, dtype)] = (st0, acts, cache, want, dev32, D.tolerance(env_name, dev32))
    return _SIX_REFS[(case, dtype)]


def _c_oracle_deviation(cache, st0, acts, want, groups, **kw):
    """The largest |C oracle - float64| over every finite log-prob of every executed step of the forced walk."""
    got = D.c_decode(cache, st0, "evaluate", acts.shape[1], groups, want_all=True, forced_actions=acts, **kw)
    ex = want["executed"]
    assert got["err"] == 0 and torch.equal(got["actions"], acts)
    assert torch.equal(torch.isfinite(got["all_logps"])[ex], torch.isfinite(want["logps"])[ex])
    ok = torch.isfinite(want["logps"]) & ex[:, :, None]
    chosen = (got["logps"].double() - want["chosen"])[ex].abs().max()
    return max(float((got["all_logps"].double() - want["logps"])[ok].abs().max()), float(chosen)), got


def test_lds_limit_is_the_librarys():
    from rl4co_amd import _lib, kernels

    for dtype in (torch.bfloat16, torch.float16):
        assert kernels.decode_row_groups(D.LDS_MAX_N, dtype, 2 * D.LDS_MAX_N, "lds", 6) == 16
        with pytest.raises(_lib.Rl4coLibraryError):
            kernels.decode_row_groups(D.LDS_MAX_N + 1, dtype, 2 * D.LDS_MAX_N + 2, "lds", 6)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", D.edge_cases(), ids=lambda c: f"{c[0]}-n{c[1]}-b{c[2]}")
def test_c_oracle_against_float64_at_the_edge_sizes(case, dtype):
    """Teacher-forced along the case's walk, with the row groups 2, 4 and 16 ``decode_row_groups`` returns for the variants
    (fp32 STREAM, 16-bit STREAM, LDS / WIDE): every log-prob of every executed step within ``decode_f64_ref.tolerance``."""
    st0, acts, cache, want, dev32, tol = _six_reference(case, dtype)
    assert bool(want["state"]["done"].all())
    for groups in (2, 4, 16):
        dev, got = _c_oracle_deviation(cache, st0, acts, want, groups)
        print(f"{case[0]}-n{case[1]} {dtype} G={groups}: dev32 {dev32:.3e}, C oracle {dev:.3e}, bound {tol:.3e}, "
              f"ratio {dev / tol:.3f} over {int(want['executed'].sum())} steps")
        assert dev <= tol
        for k, v in want["state"].items():
            assert torch.equal(got["state"][k], v), k


def _scalar_range(env_name, st0, acts):
    """(smallest, largest) of the context scalar ``base - running`` before the clamp and of the clock, (first != current at
    some step), over the executed steps of a walk."""
    from rl4co_amd.envspec import rem_base, spec

    sp = spec(env_name)
    st = {k: v.clone() for k, v in st0.items()}
    s_min, clock_max, differ = float("inf"), 0.0, False
    for t in range(acts.shape[1]):
        ex = ~st["done"].view(-1).bool()
        if sp.scalar is not None:
            s = rem_base(sp, st, ex.numel()).view(-1) - st[sp.scalar.running].view(-1)
            s_min = min(s_min, float(s[ex].min()) if bool(ex.any()) else s_min)
            if sp.scalar.clock:
                clock_max = max(clock_max, float(st[sp.scalar.clock].view(-1)[ex].max()) if bool(ex.any()) else 0.0)
        if sp.ctx_first:
            differ |= bool(((st["first_node"].view(-1) != st["current_node"].view(-1)) & ex & (st["i"].view(-1) > 0)).any())
        D.step_state(env_name, st, acts[:, t])
    return s_min, clock_max, differ


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("mistake", D.MISTAKES)
def test_tolerance_rejects_every_seeded_mistake_of_the_six(mistake, dtype):
    """The mistaken ``step_f64`` must leave the C oracle by more than the tolerance on the n = 65 edge case of its
    environment (``q_bias``: of every one of the six) — and the case is one on which the mistake matters: a PCTSP row passes
    its required prize, the OP walk leaves the depot (every other column of ``max_length`` is smaller than column 0),
    CVRPTW's clock runs, a TSP row's current node leaves its first."""
    envs = D.SIX if ":" not in mistake else (mistake.split(":")[0],)
    for env_name in envs:
        case = (env_name, 65, 6)
        assert case in D.edge_cases()
        st0, acts, cache, want, dev32, tol = _six_reference(case, dtype)
        s_min, clock_max, differ = _scalar_range(env_name, st0, acts)
        if mistake.startswith("pctsp"):
            assert s_min < -0.1
        if mistake.startswith("op"):
            assert bool((acts != 0).any()) and bool((st0["max_length"][:, 1:] < st0["max_length"][:, :1]).all())
        if mistake.startswith("cvrptw"):
            assert clock_max > 100
        if mistake.startswith("tsp"):
            assert differ
        wrong = D.rollout(cache, st0, acts, mistake=mistake)
        assert torch.equal(wrong["masks"], want["masks"])
        groups = 2 if dtype == torch.float32 else 4
        got = D.c_decode(cache, st0, "evaluate", acts.shape[1], groups, want_all=True, forced_actions=acts)
        ok = torch.isfinite(want["logps"]) & want["executed"][:, :, None]
        dev = float((got["all_logps"].double() - wrong["logps"])[ok].abs().max())
        print(f"{env_name} {mistake}: the C oracle leaves the mistaken step by {dev:.3e} = {dev / tol:.0f} x the tolerance {tol:.3e}")
        assert dev > 100 * tol, (env_name, mistake)
