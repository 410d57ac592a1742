"""The float64 decode-step oracle (tests/decode_f64_ref.py) proven without a GPU, before it judges the kernels
(tests/test_gpu_decode_f64.py): against the reference decoder's algebra evaluated in float64 on the unfolded decoder,
against the reference's recorded rollouts, and against the seeded mistakes the GPU test is meant to catch.

The fold is exact algebra only where it is evaluated exactly: ``tests.helpers.fold_cache`` rounds the planes and tables to
fp32 (one fp32 GEMM each), which alone moves a log-prob by ~1e-7. So the 1e-10 comparison folds in float64 (the formulas of
rl4co_amd/cache.py on widened weights), and the fp32 fold of ``fold_cache`` is compared within STEP_TOL — the class of
deviation (fp32, another operation order) that bound was measured for."""
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
