"""Split-delivery VRP on the fused decode kernels (MI355X): the state arithmetic against the torch-fp32 restatement, the
log-probs against the reference's recorded rollouts (tests/golden/reference/sdvrp_*.npz), the dynamic embedding, the
filter / graph / training surfaces and the refusals. Tolerances: tests/sdvrp_ref.py (STEP_TOL) and DESIGN §4.9."""
import warnings

import pytest
import torch

from tests import sdvrp_ref
from tests.helpers import SAMPLE_SEED, WEIGHT_SEED, ll_rtol

pytestmark = pytest.mark.gpu

RECORDS = list(sdvrp_ref.CASES)


@pytest.fixture(scope="module")
def K():
    from rl4co_amd import kernels

    return kernels


def _policy(env_name="sdvrp", seed=WEIGHT_SEED, **kw):
    from rl4co_amd.policy import AttentionModelPolicy

    torch.manual_seed(seed)
    return AttentionModelPolicy(env_name, **kw).cuda().eval()


def _env_td(rec, env_name="sdvrp", scale=1.0, **kw):
    from rl4co_amd.envs import get_env
    from rl4co_amd.tensordict import TensorDict

    b, num_loc = rec["in_locs"].shape[:2]
    env = get_env(env_name, generator_params=dict(num_loc=num_loc, device="cuda"), device="cuda", **kw)
    data = {k[3:]: v.cuda() for k, v in rec.items() if k.startswith("in_")}
    data["demand"] = data["demand"] * scale
    return env, env.reset(TensorDict(data, batch_size=[b]))


# ---- 4. state exactness ------------------------------------------------------------------------------------------------------
def _random_cache(b, n, dtype, seed=0):
    from rl4co_amd.cache import FoldedCache

    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return FoldedCache("sdvrp", (r(3, b, n, 128) * 0.5).to(dtype).cuda(), None, r(b, n, 128).cuda(), r(b, 128).cuda(), None,
                       r(128).cuda(), None, (r(3, 128) * 0.5).cuda())


def _forced_case(n, b=8):
    g = torch.Generator().manual_seed(n)
    demand = torch.randint(1, 10, (b, n - 1), generator=g).float() / 15.0  # 15 units per vehicle: split deliveries
    acts, final = sdvrp_ref.random_walk(demand, 6 * n, seed=n + 1)
    assert bool(final["done"].all())
    steps = int((acts != 0).nonzero()[:, 1].max()) + 3  # every trajectory done, two padding depot steps behind
    return demand, acts[:, :steps].contiguous()


@pytest.fixture(scope="module")
def forced():
    return {n: _forced_case(n) for n in (21, 65)}  # 65 crosses the 64-entry LDS pad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("n", [21, 65])
def test_state_is_the_restatements_bit_for_bit_in_every_variant(K, forced, n, dtype):
    from rl4co_amd import _lib

    demand, acts = forced[n]
    b, steps = acts.shape
    want = sdvrp_ref.initial_state(demand)
    for t in range(steps):
        sdvrp_ref.step_state(want, acts[:, t], freeze_done=True)
    assert int(((acts[:, :, None] == torch.arange(1, n)).sum(1) > 1).sum()) > 0  # customers visited more than once
    cache = _random_cache(b, n, dtype)
    results = {}
    for variant in ("stream", "lds", "wide"):
        st = {k: v.cuda() for k, v in sdvrp_ref.initial_state(demand).items()}
        out_a = torch.zeros(b, steps, dtype=torch.int64, device="cuda")
        lps = torch.zeros(b, steps, device="cuda")
        err = K.new_error_word("cuda")
        run = lambda: K.am_decode(cache, st, mode="evaluate", max_steps=steps, actions=out_a, logps=lps, err=err,  # noqa: E731
                                  forced_actions=acts.cuda(), variant=variant)
        if dtype == torch.float32 and variant != "stream":  # fp32 planes live in the one-wave kernel only
            with pytest.raises(_lib.Rl4coLibraryError):
                run()
            continue
        run()
        assert int(err.item()) == 0
        assert torch.equal(out_a.cpu(), acts)
        for key in ("demand_with_depot", "used_capacity", "action_mask", "done", "current_node"):
            assert torch.equal(st[key].cpu(), want[key]), (variant, key)
        assert bool(torch.isfinite(lps).all())
        results[variant] = lps.cpu()
    for variant, lps in results.items():
        assert torch.equal(lps, results["stream"]), variant  # one summation tree in all three (am_decode.hip header)


def test_step_entry_equals_the_restatement(K, forced):
    demand, acts = forced[21]
    want = sdvrp_ref.initial_state(demand)
    st = {k: v.cuda() for k, v in sdvrp_ref.initial_state(demand).items()}
    for t in range(acts.shape[1]):
        sdvrp_ref.step_state(want, acts[:, t])
        K.env_step("sdvrp", st, acts[:, t].cuda().contiguous())
        for key in want:
            assert torch.equal(st[key].cpu(), want[key]), (t, key)


# ---- 5. / 6. parity with the reference's records ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def policy():
    return _policy()


@pytest.mark.parametrize("case", RECORDS)
def test_teacher_forced_log_probs_equal_the_records(policy, case):
    rec = sdvrp_ref.record(case)
    env, td = _env_td(rec)
    with torch.inference_mode():
        out = policy(td, env, phase="test", actions=rec["actions"].cuda(), return_sum_log_likelihood=False)
    got, want = out["log_likelihood"].cpu(), rec["log_likelihood"]
    finite = torch.isfinite(want)
    dev = float((got - want)[finite].abs().max())
    print(f"{case}: largest per-step log-prob deviation {dev:.3e} over {int(finite.sum())} steps")
    assert dev <= sdvrp_ref.STEP_TOL
    torch.testing.assert_close(got.sum(1), want.sum(1), rtol=ll_rtol("cvrp", gpu=True), atol=0.0)
    assert torch.equal(out["reward"].cpu(), rec["reward"])


@pytest.mark.parametrize("case", RECORDS)
def test_free_running_rollout_reproduces_the_records(policy, case):
    rec = sdvrp_ref.record(case)
    env, td = _env_td(rec)
    b, n = td["action_mask"].shape
    greedy = case.endswith("greedy")
    kw = dict(decode_type="greedy") if greedy else dict(
        decode_type="sampling", exp_noise=sdvrp_ref.sample_noise(b, n, 6 * n, SAMPLE_SEED).cuda())
    with torch.inference_mode():
        out = policy(td, env, phase="test", return_all_logp=True, return_sum_log_likelihood=False, **kw)
    acts, ref = out["actions"].cpu(), rec["actions"]
    t_cmp = max(acts.shape[1], ref.shape[1])
    pad = lambda a: torch.cat((a, torch.zeros(b, t_cmp - a.shape[1], dtype=torch.int64)), 1)  # noqa: E731
    same = (pad(acts) == pad(ref)).all(1)
    fragile = rec["min_gap"] < 2 * sdvrp_ref.STEP_TOL if greedy else torch.ones(b, dtype=torch.bool)
    print(f"{case}: {int((~same).sum())} of {b} trajectories left the record")
    assert bool(same[~fragile].all())
    assert torch.equal(out["reward"].cpu()[same], rec["reward"][same])
    all_lp = out["all_logp"].cpu()
    for r in (~same).nonzero()[:, 0].tolist():  # a proven near-tie at the first divergent step
        t = int((pad(acts)[r] != pad(ref)[r]).nonzero()[0])
        own, other = int(acts[r, t]), int(ref[r, t])
        gap = all_lp[r, t, own] - all_lp[r, t, other]
        if not greedy:  # the sampler takes the largest exp(lp) / noise: compare the log keys
            nz = kw["exp_noise"][t, r].cpu()
            gap = gap - (torch.log(nz[own]) - torch.log(nz[other]))
        assert 0.0 <= float(gap) <= 2 * sdvrp_ref.STEP_TOL, (r, t, float(gap))


# ---- 7. the dynamic term is live ---------------------------------------------------------------------------------------------
def test_dynamic_term_is_live_and_vanishes_into_cvrp():
    rec = sdvrp_ref.record("sdvrp20_greedy")
    pol = _policy(cache_dtype=torch.float32)
    env, td = _env_td(rec)
    acts = rec["actions"].cuda()
    with torch.inference_mode():
        with_dyn = pol(td, env, phase="test", actions=acts)["log_likelihood"]
        pol.decoder.dynamic_embedding.projection.weight.zero_()  # (in place on the parameter: the packed weights follow)
        _, td = _env_td(rec)
        without = pol(td, env, phase="test", actions=acts)["log_likelihood"]
    assert float((with_dyn - without).abs().max()) > 1e-3
    # no customer ever split (an instance's whole demand fits one vehicle) and no dynamic term: CVRP's rollout, less its
    # closing depot visit (SDVRP is done when the last demand is served)
    cvrp = _policy("cvrp", cache_dtype=torch.float32)
    cvrp.load_state_dict({k: v for k, v in pol.state_dict().items() if "dynamic_embedding" not in k}, strict=True)
    env_s, td_s = _env_td(rec, scale=0.2)
    env_c, td_c = _env_td(rec, "cvrp", scale=0.2)
    assert float(td_s["demand"].sum(1).max()) < 1.0
    with torch.inference_mode():
        out_s = pol(td_s, env_s, phase="test", decode_type="greedy", return_sum_log_likelihood=False)
        out_c = cvrp(td_c, env_c, phase="test", decode_type="greedy", return_sum_log_likelihood=False)
    a_s, a_c = out_s["actions"], out_c["actions"]
    assert int(((a_s[:, :, None] == torch.arange(1, 21, device="cuda")).sum(1) > 1).sum()) == 0  # no split delivery
    t = max(a_s.shape[1], a_c.shape[1])  # (CVRP may add the closing depot visit: action 0 with log-prob 0, as the padding)
    pad = lambda x: torch.cat((x, torch.zeros(x.shape[0], t - x.shape[1], dtype=x.dtype, device="cuda")), 1)  # noqa: E731
    assert torch.equal(pad(a_c), pad(a_s))
    assert torch.equal(pad(out_c["log_likelihood"]), pad(out_s["log_likelihood"]))


# ---- 8. top-k / top-p and graph capture ----------------------------------------------------------------------------------------
def test_filter_and_graph_capture(policy):
    from rl4co_amd.graph import GraphedRollout

    rec = sdvrp_ref.record("sdvrp20_greedy")
    env, td = _env_td(rec)
    run = lambda **kw: policy(_env_td(rec)[1], env, phase="test", **kw)  # noqa: E731
    with torch.inference_mode():
        plain = run(decode_type="sampling", seed=7)
        inactive = run(decode_type="sampling", seed=7, top_k=21, top_p=1.0)
        greedy = run(decode_type="greedy")
        k1 = run(decode_type="sampling", seed=7, top_k=1)
    for key in ("actions", "log_likelihood", "reward"):
        assert torch.equal(plain[key], inactive[key]), key
    assert torch.equal(k1["actions"], greedy["actions"]) and torch.equal(k1["reward"], greedy["reward"])
    assert bool((k1["log_likelihood"] == 0).all())  # one node kept per step
    data = env.generator(batch_size=[64])
    g = GraphedRollout(policy, env, data, decode_type="greedy")
    torch.manual_seed(5)
    for d in (data, env.generator(batch_size=[64]), data):
        got = {k: v.clone() for k, v in g(d).items() if k in ("actions", "reward", "log_likelihood")}
        with torch.inference_mode():
            want = policy(env.reset(d), env, phase="test", decode_type="greedy")
        for key, v in got.items():
            assert torch.equal(v, want[key]), key


# ---- 9. training ---------------------------------------------------------------------------------------------------------------
def test_reinforce_gradients_equal_the_reference_decoders():
    from rl4co_amd import _lib
    from rl4co_amd.envs import get_env

    env = get_env("sdvrp", generator_params=dict(num_loc=20, device="cuda"), device="cuda")
    torch.manual_seed(3)
    data = env.generator(batch_size=[32])
    pol = _policy(seed=11).train()
    _lib._warned.clear()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = pol(env.reset(data), env, phase="train", decode_type="sampling", seed=5)
    ours = [x for x in w if issubclass(x.category, RuntimeWarning) and "rl4co_amd" in str(x.message)]
    assert len(ours) == 1 and "dynamic embedding" in str(ours[0].message), [str(x.message) for x in w]
    reward, ll, acts = out["reward"], out["log_likelihood"], out["actions"]
    adv = (reward - reward.mean()).detach()
    (adv * ll).mean().backward()
    got = {k: p.grad.clone() for k, p in pol.named_parameters() if p.grad is not None}
    assert "decoder.dynamic_embedding.projection.weight" in got
    pol.zero_grad()
    # the restatement: the same (torch) encoder, then the reference decoder's algebra step by step along the same actions
    td = env.reset(data)
    hidden, _ = pol.encoder(td)
    st0 = {k: v.to("cuda") for k, v in sdvrp_ref.initial_state(td["demand"].cpu()).items()}
    ll_ref = sdvrp_ref.decoder_step_logps(pol.decoder, hidden.float(), st0, acts).sum(1)
    torch.testing.assert_close(ll.detach(), ll_ref.detach(), rtol=1e-4, atol=1e-4)
    (adv * ll_ref).mean().backward()
    want = {k: p.grad for k, p in pol.named_parameters() if p.grad is not None}
    assert sorted(got) == sorted(want)
    # the measure of the fold=False training test (test_gpu_policy.py): relative Frobenius error of the whole gradient
    # vector; and per tensor wherever the gradient is not analytically zero (the biases in front of a training-mode batch
    # norm cancel in its mean: both sides hold rounding noise there, checked by size only, as DESIGN "Top-k / top-p (nucleus) sampling inside the decode kernels" does)
    flat = lambda g: torch.cat([g[k].flatten() for k in sorted(g)])  # noqa: E731
    total = float(flat(want).norm())
    rel = float((flat(got) - flat(want)).norm()) / total
    print(f"REINFORCE gradient, whole vector: relative error {rel:.3e}")
    assert rel <= 2e-3, rel
    for k in want:
        if k.endswith(("out_proj.bias", "lins.1.bias")):  # in front of a training-mode batch norm: analytically zero
            assert float(got[k].norm()) <= 1e-4 * total and float(want[k].norm()) <= 1e-4 * total, k
            continue
        rel_k = float((got[k] - want[k]).norm() / want[k].norm())
        assert rel_k <= 2e-3, (k, rel_k)
    k = "decoder.dynamic_embedding.projection.weight"
    assert float(want[k].norm()) > 1e-6 * total  # the dynamic embedding learns


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(K, forced):
    from rl4co_amd import _lib

    demand, acts = forced[21]
    b, steps = acts.shape
    cache = _random_cache(b, 21, torch.bfloat16)

    def run(variant="auto", max_steps=steps, mode="evaluate", **kw):
        st = {k: v.cuda() for k, v in sdvrp_ref.initial_state(demand).items()}
        out_a = torch.zeros(b, steps, dtype=torch.int64, device="cuda")
        lps = torch.zeros(b, steps, device="cuda")
        err = K.new_error_word("cuda")
        K.am_decode(cache, st, mode=mode, max_steps=max_steps, actions=out_a, logps=lps, err=err,
                    forced_actions=acts.cuda(), variant=variant, **kw)
        return int(err.item()), out_a, lps

    with pytest.raises(_lib.Rl4coLibraryError, match="variant >= 0"):  # as a pinned ms with an active filter
        run("ms")
    with pytest.raises(_lib.Rl4coLibraryError, match="variant >= 0"):
        K.am_decode(_random_cache(b, 21, torch.bfloat16), {k: v.cuda() for k, v in sdvrp_ref.initial_state(demand).items()},
                    mode="sampling", max_steps=4, actions=torch.zeros(b, 4, dtype=torch.int64, device="cuda"),
                    logps=torch.zeros(b, 4, device="cuda"), err=K.new_error_word("cuda"), variant="ms", top_k=3)
    assert K.decode_variant(21, torch.bfloat16, 126, 4096 * 8, 4096, env_name="sdvrp") != _lib.VARIANT_MS  # auto skips it
    with pytest.raises(ValueError, match="unfolded parity mode serves tsp / cvrp"):
        _policy(fold=False)(_env_td(sdvrp_ref.record("sdvrp20_greedy"))[1], phase="test", decode_type="greedy")
    # a horizon too short: the sticky bit, and nothing behind the columns it was given
    short = 5
    err, out_a, lps = run("stream", max_steps=short)
    assert err & _lib.EBIT_MAX_STEPS
    assert bool((out_a[:, short:] == 0).all()) and bool((lps[:, short:] == 0).all())
    with pytest.raises(AssertionError, match="Exceeded maximum number of steps"):
        _lib.raise_for_error_bits(err)
