"""GPU (`-m gpu`): the SDVRP and mTSP builds of the fused decode kernels against the float64 restatement of the folded decode
step (tests/decode_f64_ref.py, itself pinned to the reference decoder and the records by tests/test_decode_f64_cpu.py) — what
the C specified-order oracle is to the six older environments. Every variant / plane-type pair, 2 to 257 nodes, batches that
are no multiple of 8, one agent and as many agents as customers; teacher-forced, free-running (greedy and sampling), with the
top-k / top-p filter, and through the policy at a size beyond the records.

Tolerance, per case and never from a kernel's output: ``max(STEP_TOL, 4 x dev32)``, ``dev32`` = the largest deviation of the
same step evaluated in float32 by torch from the float64 one on the same inputs (``decode_f64_ref.tolerance``). Every test
prints ``dev32``, the kernel's largest deviation and the bound.

Measured on the MI355X (kernel deviation / bound, the largest of each test): teacher-forced 0.307 (sdvrp, n = 65, fp32 planes:
1.47e-6 against 4.77e-6) and 0.259 (mtsp, n = 21, two agents); free-running 0.188 / 0.146, and no chosen node ever left the
oracle's own choice (largest gap 0); kept log-probs under the filter 0.307; through the policy at n = 129 0.129 / 0.100.

A pinned LDS-resident build at n >= 107 is refused by design (its planes do not fit half a CU's LDS): those cases assert the
refusal. Seeded on the kernel side (the two ``dyn`` rows swapped in the binding), every sdvrp case here fails by ~8e5 x the
bound while tests/test_gpu_sdvrp.py::test_state_is_the_restatements_bit_for_bit_in_every_variant still passes."""
import pytest
import torch

from tests import decode_f64_ref as D
from tests import mtsp_ref
from tests.topkp_ref import filter_f64, top_p_entry_margins, unpack_bits

pytestmark = pytest.mark.gpu

VARIANTS = [("stream", torch.float32), ("stream", torch.bfloat16), ("stream", torch.float16), ("lds", torch.bfloat16),
            ("lds", torch.float16), ("wide", torch.bfloat16), ("wide", torch.float16)]
VIDS = ["stream-f32", "stream-bf16", "stream-f16", "lds-bf16", "lds-f16", "wide-bf16", "wide-f16"]
# (n, B): the smallest instances, one LDS pad and its neighbours, a second and a third pad beyond the first (n > 128, n > 192,
# n > 256), batches of 1 and of no multiple of 8
SIZES = [(2, 5), (3, 13), (21, 8), (64, 9), (65, 8), (66, 1), (128, 6), (129, 6), (200, 4), (257, 3)]
# (env, n, B, extra). extra — sdvrp "depot": the state's depot column holds -0.25 until the first depot visit (the kernels take
# the depot's demand as 0 whatever is stored); mtsp: that many agents in every row (one; few; as many as customers)
CASES = ([("sdvrp", n, b, None) for n, b in SIZES] + [("sdvrp", 21, 8, "depot")] + [("mtsp", n, b, None) for n, b in SIZES]
         + [("mtsp", 21, 8, k) for k in (1, 2, 20)] + [("mtsp", 129, 6, k) for k in (1, 5)])
STATE_KEYS = {"sdvrp": ("demand_with_depot", "used_capacity", "action_mask", "done", "current_node"),
              "mtsp": mtsp_ref.STATE_KEYS}


def _cid(case):
    env_name, n, b, extra = case
    return f"{env_name}-n{n}-b{b}" + ("" if extra is None else f"-{extra}")


@pytest.fixture(scope="module")
def K():
    from rl4co_amd import kernels

    return kernels


_INSTANCES, _REFS = {}, {}


def _instance(case):
    """(initial state, forced actions) of a case, computed once."""
    if case not in _INSTANCES:
        env_name, n, b, extra = case
        inst, acts = D.forced_case(env_name, n, b, extra if env_name == "mtsp" else None)
        st0 = D.initial_state(env_name, inst)
        if extra == "depot":
            st0["demand_with_depot"][:, 0] = -0.25
        _INSTANCES[case] = (st0, acts)
    return _INSTANCES[case]


def _reference(cache, st0, acts, key):
    """The oracle along ``acts`` in float64 and the case's tolerance from its float32 twin, computed once per ``key``."""
    if key not in _REFS:
        want = D.rollout(cache, st0, acts)
        dev32 = D.fp32_cost(want, D.rollout(cache, st0, acts, step=D.step_f32))
        _REFS[key] = (want, dev32, D.tolerance(cache.env_name, dev32))
    return _REFS[key]


def _launch(K, cache, st0, steps, variant, mode, **kw):
    b = st0["action_mask"].shape[0]
    st = {k: v.clone().cuda() for k, v in st0.items()}
    out_a = torch.zeros(b, steps, dtype=torch.int64, device="cuda")
    lps = torch.zeros(b, steps, device="cuda")
    err = K.new_error_word("cuda")
    K.am_decode(cache.to("cuda"), st, mode=mode, max_steps=steps, actions=out_a, logps=lps, err=err, variant=variant, **kw)
    return {k: v.cpu() for k, v in st.items()}, out_a.cpu(), lps.cpu(), int(err.item())


def _refused(K, cache, st0, steps, variant, mode, **kw):
    """The LDS-resident build keeps a trajectory's three 16-bit planes in half a CU's LDS (80 KiB): pinned at a
    size whose planes alone exceed that (n >= 107), the library must refuse — no other kernel runs in its place. True if
    this launch is such a one (and was refused)."""
    from rl4co_amd import _lib

    n = cache.num_nodes
    if variant != "lds" or 3 * n * 128 * 2 <= 80 * 1024:
        return False
    with pytest.raises(_lib.Rl4coLibraryError, match="variant >= 0"):
        _launch(K, cache, st0, steps, variant, mode, **kw)
    return True


def _assert_state(env_name, st, want):
    for key in STATE_KEYS[env_name]:
        assert torch.equal(st[key], want[key]), key
    if env_name == "mtsp":  # the reward is carried in the state
        assert torch.equal(-st["max_subtour_length"], -want["max_subtour_length"])


# ---- teacher-forced ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,dtype", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_teacher_forced_log_probs_against_float64(K, case, variant, dtype):
    env_name, n, b, extra = case
    st0, acts = _instance(case)
    steps = acts.shape[1]
    if env_name == "sdvrp" and n >= 3:  # (a single customer's demand fits one vehicle: n = 2 has no split delivery)
        assert int(((acts[:, :, None] == torch.arange(1, n)).sum(1) > 1).sum()) > 0  # customers visited more than once
    if env_name == "mtsp" and extra is None and n >= 21 and b >= 4:  # one agent: no depot visit; two: one; many: many
        own = mtsp_ref.row_lengths(acts)
        depot_visits = torch.stack([(acts[r, : int(own[r])] == 0).sum() for r in range(b)])
        assert int(depot_visits[0]) == 0 and int(depot_visits[1]) == 1 and int(depot_visits.max()) >= 4
    cache = D.random_cache(env_name, b, n, dtype)
    if _refused(K, cache, st0, steps, variant, "evaluate", forced_actions=acts.cuda()):
        return
    want, dev32, tol = _reference(cache, st0, acts, (case, dtype))
    st, out_a, lps, err = _launch(K, cache, st0, steps, variant, "evaluate", forced_actions=acts.cuda())
    assert err == 0
    assert torch.equal(out_a, acts)
    _assert_state(env_name, st, want["state"])
    ex = want["executed"]
    assert bool(want["state"]["done"].all()) and bool(torch.isfinite(want["chosen"][ex]).all())
    dev = float((lps.double() - want["chosen"])[ex].abs().max())
    print(f"{_cid(case)} {variant}: dev32 {dev32:.3e}, kernel {dev:.3e}, bound {tol:.3e}, ratio {dev / tol:.3f} over "
          f"{int(ex.sum())} steps")
    assert dev <= tol
    assert bool((lps[~ex] == 0).all()) and bool((out_a[~ex] == 0).all())  # behind done: the padding action, log-prob 0


# ---- free-running -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,dtype", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("mode", ["greedy", "sampling"])
@pytest.mark.parametrize("n", [21, 65, 129])
@pytest.mark.parametrize("env_name", ["sdvrp", "mtsp"])
def test_free_running_rollout_against_float64(K, env_name, n, mode, variant, dtype):
    from rl4co_amd.envspec import spec

    b = 16
    inst = D.sdvrp_instances(n, b) if env_name == "sdvrp" else D.mtsp_instances(n, b)
    st0 = D.initial_state(env_name, inst)
    cache = D.random_cache(env_name, b, n, dtype)
    horizon = spec(env_name).horizon(n)
    noise = D.REFS[env_name].sample_noise(b, n, horizon, 4321 + n) if mode == "sampling" else None
    kw = {} if noise is None else dict(exp_noise=noise.cuda())
    if _refused(K, cache, st0, horizon, variant, mode, **kw):
        return
    st, acts, lps, err = _launch(K, cache, st0, horizon, variant, mode, **kw)
    assert err == 0
    steps = min(int(mtsp_ref.row_lengths(acts).max()) + 2, horizon)
    assert bool((acts[:, steps:] == 0).all()) and bool((lps[:, steps:] == 0).all())
    acts, lps = acts[:, :steps].contiguous(), lps[:, :steps].double()
    # the kernel's own actions through the oracle (the variants of one plane type usually agree: computed once per walk)
    want, dev32, tol = _reference(cache, st0, acts, (env_name, n, mode, dtype, acts.numpy().tobytes()))
    ex = want["executed"]
    assert bool(want["state"]["done"].all())  # every row finished inside the horizon
    _assert_state(env_name, st, want["state"])
    assert bool(want["masks"].gather(2, acts[:, :, None])[:, :, 0][ex].all())  # every chosen node is feasible
    key = want["logps"]  # greedy: the largest log-prob; sampling: the largest exp(lp) / noise, compared as log keys
    if mode == "sampling":
        key = key - torch.log(noise[:steps].double()).transpose(0, 1)
    gap = key.max(-1)[0] - key.gather(2, acts[:, :, None])[:, :, 0]
    dev = float((lps - want["chosen"])[ex].abs().max())
    print(f"{env_name}-n{n} {mode} {variant}: dev32 {dev32:.3e}, kernel {dev:.3e}, bound {tol:.3e}, ratio {dev / tol:.3f}, "
          f"largest gap to the oracle's choice {float(gap[ex].max()):.3e} over {int(ex.sum())} steps")
    assert bool((gap[ex] <= 2 * tol).all()), float(gap[ex].max())  # the oracle's choice, or a near-tie with it
    assert dev <= tol
    assert bool((lps[~ex] == 0).all()) and bool((acts[~ex] == 0).all())


# ---- top-k / top-p -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,dtype", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("top_k,top_p", [(5, 0.0), (0, 0.5), (5, 0.5)], ids=["k5", "p0.5", "k5-p0.5"])
@pytest.mark.parametrize("env_name", ["sdvrp", "mtsp"])
def test_kept_set_against_float64(K, env_name, top_k, top_p, variant, dtype):
    """The kept set of every executed step of the n = 65 forced walk against ``filter_f64`` on the oracle's processed logits.
    An entry is not judged where the cut is closer to a tie than the tolerance: its ``top_p_entry_margins`` under it, or —
    top-k — a logit within it of the k-th largest (then the step's survivors are open, and so is its top-p cut). The walk is
    forced, so which entries are judged follows from the oracle alone: with these seeds 0 of 855 (sdvrp) and at most 1 of 526
    (mtsp: p = 0.5 on bf16 planes; 0.2 %) (row, step) pairs hold an unjudged entry (bound: 2 %)."""
    from rl4co_amd import _lib

    case = (env_name, 65, 8, None)
    st0, acts = _instance(case)
    b, steps = acts.shape
    n = 65
    cache = D.random_cache(env_name, b, n, dtype)
    want, dev32, tol = _reference(cache, st0, acts, (case, dtype))
    ex = want["executed"]
    z = want["z"]
    keep = filter_f64(z, top_k, top_p)
    open_k = torch.zeros_like(ex)
    if top_k > 0:
        zf = z.masked_fill(~want["masks"], float("-inf"))
        tau = torch.topk(zf, top_k, dim=-1)[0][..., -1:]  # (-inf where fewer than k nodes are feasible: nothing is cut)
        open_k = (((zf - tau).abs() < tol) & (zf != tau)).any(-1)
    judged = (top_p_entry_margins(z, top_k, top_p) >= tol) & ~open_k[:, :, None]
    unjudged = (~judged).any(-1)[ex]
    print(f"{env_name} k={top_k} p={top_p} {variant}: {int(unjudged.sum())} of {unjudged.numel()} (row, step) pairs hold an "
          f"unjudged entry; dev32 {dev32:.3e}, bound {tol:.3e}")
    assert int(unjudged.sum()) * 50 <= unjudged.numel()
    kept = torch.zeros(b, steps, 4 * ((n + 127) // 128), dtype=torch.int32, device="cuda")
    st, out_a, lps, err = _launch(K, cache, st0, steps, variant, "evaluate", forced_actions=acts.cuda(), top_k=top_k,
                                  top_p=top_p, kept_bits=kept)
    assert err & ~_lib.EBIT_NEG_INF_LOGP == 0  # (a forced node the filter removed reports -inf and that bit)
    assert torch.equal(out_a, acts)
    _assert_state(env_name, st, want["state"])
    have = unpack_bits(kept, n).cpu()
    wrong = (have != keep) & judged & ex[:, :, None]
    assert not bool(wrong.any()), wrong.nonzero()[:8].tolist()
    # the forced node's log-prob: renormalised over the kept set, -inf if removed (steps judged in every entry)
    zk = z.masked_fill(~keep, float("-inf"))
    lp_k = (zk - torch.logsumexp(zk, -1, keepdim=True)).gather(2, acts[:, :, None])[:, :, 0]
    full = ex & judged.all(-1)
    removed = full & torch.isinf(lp_k)
    assert bool(removed.any()) and bool((err & _lib.EBIT_NEG_INF_LOGP) != 0)
    assert bool((lps[removed] == float("-inf")).all())
    dev = float((lps.double() - lp_k)[full & ~removed].abs().max())
    print(f"    kept log-probs: kernel {dev:.3e}, ratio {dev / tol:.3f}")
    assert dev <= tol


# ---- through the policy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("env_name", ["sdvrp", "mtsp"])
def test_policy_log_likelihood_against_float64_beyond_the_records(K, monkeypatch, env_name, dtype):
    """n = 129, B = 6, the variant the library chooses, on the cache the policy itself built (captured at the kernel binding,
    not refolded)."""
    from rl4co_amd.envs import get_env
    from rl4co_amd.policy import AttentionModelPolicy
    from rl4co_amd.tensordict import TensorDict
    from tests.helpers import WEIGHT_SEED

    n, b = 129, 6
    st0, acts = _instance((env_name, n, b, None))
    g = torch.Generator().manual_seed(7)
    if env_name == "sdvrp":
        data = {"locs": torch.rand(b, n - 1, 2, generator=g), "depot": torch.rand(b, 2, generator=g),
                "demand": st0["demand_with_depot"][:, 1:].clone()}
    else:
        data = {"locs": st0["locs"].clone(), "num_agents": st0["num_agents"].clone()}
    env = get_env(env_name, generator_params=dict(num_loc=n - 1 if env_name == "sdvrp" else n, device="cuda"), device="cuda")
    td = env.reset(TensorDict({k: v.cuda() for k, v in data.items()}, batch_size=[b]))
    torch.manual_seed(WEIGHT_SEED)
    pol = AttentionModelPolicy(env_name, cache_dtype=dtype).cuda().eval()
    seen = []
    launch = K.am_decode

    def spy(cache, state, **kw):
        seen.append((cache.to("cpu"), kw["variant"]))
        return launch(cache, state, **kw)

    monkeypatch.setattr(K, "am_decode", spy)
    with torch.inference_mode():
        out = pol(td, env, phase="test", actions=acts.cuda(), return_sum_log_likelihood=False)
    assert len(seen) == 1 and seen[0][1] == "auto" and seen[0][0].kvl.dtype == dtype
    cache = seen[0][0]
    want, dev32, tol = _reference(cache, st0, acts, ("policy", env_name, dtype))
    got = out["log_likelihood"].cpu().double()  # (the policy returns the columns up to the longest row's own length)
    t_used = got.shape[1]
    assert t_used == int(mtsp_ref.row_lengths(acts).max()) and not bool(want["executed"][:, t_used:].any())
    ex = want["executed"][:, :t_used]
    dev = float((got - want["chosen"][:, :t_used])[ex].abs().max())
    print(f"policy {env_name}-n{n} {dtype}: dev32 {dev32:.3e}, kernel {dev:.3e}, bound {tol:.3e}, ratio {dev / tol:.3f}")
    assert dev <= tol
    assert bool((got[~ex] == 0).all())
