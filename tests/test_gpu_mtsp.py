"""Multi-agent TSP (min-max) on the fused decode kernels (MI355X): the state arithmetic against the torch-fp32 restatement,
the log-probs and rewards against the reference's recorded rollouts (tests/golden/reference/mtsp_*.npz; the rewards carry the
reference's padding step), the four-scalar context, the filter and training surfaces and the refusals. Tolerances:
tests/mtsp_ref.py (STEP_TOL) and DESIGN §4.10."""
import warnings

import pytest
import torch

from tests import mtsp_ref
from tests.helpers import SAMPLE_SEED, WEIGHT_SEED, ll_rtol

pytestmark = pytest.mark.gpu

RECORDS = list(mtsp_ref.CASES)
STATE_KEYS = ("current_length", "max_subtour_length", "agent_idx", "action_mask", "done", "current_node")


@pytest.fixture(scope="module")
def K():
    from rl4co_amd import kernels

    return kernels


def _policy(seed=WEIGHT_SEED, **kw):
    from rl4co_amd.policy import AttentionModelPolicy

    torch.manual_seed(seed)
    return AttentionModelPolicy("mtsp", **kw).cuda().eval()


def _env_td(rec, **kw):
    from rl4co_amd.envs import get_env
    from rl4co_amd.tensordict import TensorDict

    b, num_loc = rec["in_locs"].shape[:2]
    env = get_env("mtsp", generator_params=dict(num_loc=num_loc, device="cuda"), device="cuda", **kw)
    data = {k[3:]: v.cuda() for k, v in rec.items() if k.startswith("in_")}
    return env, env.reset(TensorDict(data, batch_size=[b]))


# ---- 1. / 2. state exactness ---------------------------------------------------------------------------------------------------
def _random_cache(b, n, dtype, seed=0):
    from rl4co_amd.cache import FoldedCache

    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return FoldedCache("mtsp", (r(3, b, n, 128) * 0.5).to(dtype).cuda(), None, r(b, n, 128).cuda(), r(b, 128).cuda(), None,
                       None, None, None, (r(4, 128) * 0.5).cuda())


def _forced_case(n, b=8):
    g = torch.Generator().manual_seed(n)
    locs = torch.rand(b, n, 2, generator=g)
    # one agent (the depot is never offered), few, and more agents than customers
    num_agents = torch.tensor([1, 2, 5, n + 3, 1, 2, 5, n + 3])
    acts, final = mtsp_ref.random_walk(locs, num_agents, 2 * n, seed=n + 1)
    assert bool(final["done"].all())
    steps = int(mtsp_ref.row_lengths(acts).max()) + 2  # every trajectory done, two padding columns behind
    return locs, num_agents, acts[:, :steps].contiguous()


@pytest.fixture(scope="module")
def forced():
    return {n: _forced_case(n) for n in (21, 65)}  # 65 crosses the 64-entry LDS pad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("n", [21, 65])
def test_state_is_the_restatements_bit_for_bit_in_every_variant(K, forced, n, dtype):
    from rl4co_amd import _lib

    locs, num_agents, acts = forced[n]
    b, steps = acts.shape
    want = mtsp_ref.initial_state(locs, num_agents)
    for t in range(steps):
        mtsp_ref.step_state(want, acts[:, t], freeze_done=True)
    own = mtsp_ref.row_lengths(acts)
    depot_visits = torch.stack([(acts[r, : int(own[r])] == 0).sum() for r in range(b)])
    assert int(depot_visits[0]) == 0 and int(depot_visits[1]) == 1 and int(depot_visits.max()) >= 4  # 1, 2 and many agents
    cache = _random_cache(b, n, dtype)
    results = {}
    for variant in ("stream", "lds", "wide"):
        st = {k: v.cuda() for k, v in mtsp_ref.initial_state(locs, num_agents).items()}
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
        for key in STATE_KEYS:
            assert torch.equal(st[key].cpu(), want[key]), (variant, key)
        assert bool(torch.isfinite(lps).all())
        results[variant] = lps.cpu()
    for variant, lps in results.items():
        assert torch.equal(lps, results["stream"]), variant  # one summation tree in all three (am_decode.hip header)


def test_step_entry_equals_the_restatement(K, forced):
    locs, num_agents, acts = forced[21]
    want = mtsp_ref.initial_state(locs, num_agents)
    st = {k: v.cuda() for k, v in mtsp_ref.initial_state(locs, num_agents).items()}
    for t in range(acts.shape[1]):
        mtsp_ref.step_state(want, acts[:, t])
        K.env_step("mtsp", st, acts[:, t].cuda().contiguous())
        for key in STATE_KEYS:
            assert torch.equal(st[key].cpu(), want[key]), (t, key)


# ---- 3. / 4. parity with the reference's records ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def policy():
    return _policy()


@pytest.mark.parametrize("case", RECORDS)
def test_teacher_forced_log_probs_and_rewards_equal_the_records(policy, case):
    rec = mtsp_ref.record(case)
    env, td = _env_td(rec)
    with torch.inference_mode():
        out = policy(td, env, phase="test", actions=rec["actions"].cuda(), return_sum_log_likelihood=False)
    got, want = out["log_likelihood"].cpu(), rec["log_likelihood"]
    assert got.shape == want.shape
    finite = torch.isfinite(want)
    assert bool(finite.all())  # every row and step is compared
    dev = float((got - want).abs().max())
    print(f"{case}: largest per-step log-prob deviation {dev:.3e} over {int(finite.sum())} steps")
    assert dev <= mtsp_ref.STEP_TOL
    torch.testing.assert_close(got.sum(1), want.sum(1), rtol=ll_rtol("cvrp", gpu=True), atol=0.0)
    assert torch.equal(out["reward"].cpu(), rec["reward"])  # the padding rule on the GPU, bit for bit


@pytest.mark.parametrize("case", RECORDS)
def test_free_running_rollout_reproduces_the_records(policy, case):
    rec = mtsp_ref.record(case)
    env, td = _env_td(rec)
    b, n = td["action_mask"].shape
    greedy = case.endswith("greedy")
    kw = dict(decode_type="greedy") if greedy else dict(
        decode_type="sampling", exp_noise=mtsp_ref.sample_noise(b, n, 2 * n, SAMPLE_SEED).cuda())
    with torch.inference_mode():
        out = policy(td, env, phase="test", return_all_logp=True, return_sum_log_likelihood=False, **kw)
    acts, ref = out["actions"].cpu(), rec["actions"]
    t_cmp = max(acts.shape[1], ref.shape[1])
    pad = lambda a: torch.cat((a, torch.zeros(b, t_cmp - a.shape[1], dtype=torch.int64)), 1)  # noqa: E731
    same = (pad(acts) == pad(ref)).all(1)
    print(f"{case}: {int((~same).sum())} of {b} trajectories left the record")
    assert int((~same).sum()) * 4 <= b
    # a row's reward also depends on whether the batch outlived it (the padding step): comparable when both rollouts have
    # the same length, or the row is shorter than both
    own = mtsp_ref.row_lengths(pad(acts))
    comparable = same & ((acts.shape[1] == ref.shape[1]) | (own < min(acts.shape[1], ref.shape[1])))
    assert torch.equal(out["reward"].cpu()[comparable], rec["reward"][comparable])
    assert acts.shape[1] != ref.shape[1] or bool(comparable[same].all())
    all_lp = out["all_logp"].cpu()
    for r in (~same).nonzero()[:, 0].tolist():  # a proven near-tie at the first divergent step
        t = int((pad(acts)[r] != pad(ref)[r]).nonzero()[0])
        own_a, other = int(acts[r, t]), int(ref[r, t])
        gap = all_lp[r, t, own_a] - all_lp[r, t, other]
        if not greedy:  # the sampler takes the largest exp(lp) / noise: compare the log keys
            nz = kw["exp_noise"][t, r].cpu()
            gap = gap - (torch.log(nz[own_a]) - torch.log(nz[other]))
        assert 0.0 <= float(gap) <= 2 * mtsp_ref.STEP_TOL, (r, t, float(gap))


# ---- 5. the four context vectors are live --------------------------------------------------------------------------------------
def test_context_scalars_are_live():
    rec = mtsp_ref.record("mtsp20_greedy")
    pol = _policy(cache_dtype=torch.float32)
    env, td = _env_td(rec)
    acts = rec["actions"].cuda()
    with torch.inference_mode():
        with_feats = pol(td, env, phase="test", actions=acts, return_sum_log_likelihood=False)["log_likelihood"]
        pol.decoder.context_embedding.proj_dynamic_feats.weight.zero_()  # (in place on the parameter: the packed weights follow)
        without = pol(_env_td(rec)[1], env, phase="test", actions=acts, return_sum_log_likelihood=False)["log_likelihood"]
    assert float((with_feats - without).abs().max()) > 1e-3


@pytest.mark.parametrize("n", [20, 129])
def test_fused_encoders_serve_the_featureless_init_embedding(n):
    """MTSPInitEmbedding on the fused kernels' depot | customers mode with a zero feature column: the fused fp32 kernel
    (n <= 128) and the token-tile launches (n = 129) against the torch modules evaluated in float64. Bound: 3e-6 relative
    (Frobenius), what tests/test_gpu_encoder_f32.py grants the fp32 encoder kernels against float64 — three layers of
    fp32 GEMMs in another summation order."""
    import copy

    from rl4co_amd.envs import get_env

    pol = _policy()
    env = get_env("mtsp", generator_params=dict(num_loc=n, device="cuda"), device="cuda")
    torch.manual_seed(3)
    td = env.reset(env.generator(batch_size=[4]))
    pe = pol._packed_encoder()
    assert pe.supported(td, torch.float32)
    with torch.inference_mode():
        _, hidden = pe.encode(td, torch.float32, want_hidden=True, act_dtype=torch.float32)
        want, _ = copy.deepcopy(pol.encoder).double()({"locs": td["locs"].double()})
    rel = float((hidden.double() - want).norm() / want.norm())
    print(f"mTSP-{n} fused encoder against float64: {rel:.3e}")
    assert rel <= 3e-6
    # ... and inference never reaches the torch encoder
    pol.encoder.forward = lambda *a, **k: (_ for _ in ()).throw(AssertionError("torch encoder reached"))
    with torch.inference_mode():
        out = pol(td, env, phase="test", decode_type="greedy")
    assert bool(torch.isfinite(out["reward"]).all())


# ---- 6. top-k / top-p ---------------------------------------------------------------------------------------------------------
def test_filtered_rollouts(policy, K):
    rec = mtsp_ref.record("mtsp20_greedy")
    env, _ = _env_td(rec)
    run = lambda **kw: policy(_env_td(rec)[1], env, phase="test", **kw)  # noqa: E731
    with torch.inference_mode():
        plain = run(decode_type="sampling", seed=7)
        inactive = run(decode_type="sampling", seed=7, top_k=20, top_p=1.0)
        greedy = run(decode_type="greedy")
        k1 = run(decode_type="sampling", seed=7, top_k=1)
        hot = run(decode_type="sampling", seed=7, temperature=0.5)
    for key in ("actions", "log_likelihood", "reward"):
        assert torch.equal(plain[key], inactive[key]), key
    assert torch.equal(k1["actions"], greedy["actions"]) and torch.equal(k1["reward"], greedy["reward"])
    assert bool((k1["log_likelihood"] == 0).all())  # one node kept per step
    assert not torch.equal(hot["log_likelihood"], plain["log_likelihood"])
    # an active filter at the kernel surface: every chosen action lies inside its step's kept set
    with torch.inference_mode():
        hidden, _ = policy._encode(_env_td(rec)[1])
        cache = policy.decoder.precompute_cache(hidden.float(), torch.float32)
    td = _env_td(rec)[1]
    st = policy._initial_state(td, 0)
    b, n, steps = 64, 20, 40
    acts = torch.zeros(b, steps, dtype=torch.int64, device="cuda")
    lps = torch.zeros(b, steps, device="cuda")
    kept = torch.zeros(b, steps, 4, dtype=torch.int32, device="cuda")
    status = torch.zeros(6, dtype=torch.int32, device="cuda")
    K.am_decode(cache, st, mode="sampling", max_steps=steps, actions=acts, logps=lps, err=status[:1], philox_seed=3,
                steps_summary=status[2:6], top_k=3, top_p=0.8, kept_bits=kept)
    assert int(status[0]) == 0
    t_used = int(status[2])
    lengths = mtsp_ref.row_lengths(acts[:, :t_used].cpu())
    for r in range(b):
        for t in range(int(lengths[r])):
            a = int(acts[r, t])
            row = kept[r, t].cpu()
            assert (int(row[a // 32]) >> (a % 32)) & 1, (r, t, a)
            assert 1 <= sum(bin(int(w) & 0xFFFFFFFF).count("1") for w in row) <= 3, (r, t)


# ---- 7. training ---------------------------------------------------------------------------------------------------------------
def test_reinforce_gradients_equal_the_reference_decoders():
    from rl4co_amd import _lib
    from rl4co_amd.envs import get_env

    env = get_env("mtsp", generator_params=dict(num_loc=20, min_num_agents=1, max_num_agents=6, device="cuda"), device="cuda")
    torch.manual_seed(3)
    data = env.generator(batch_size=[32])
    pol = _policy(seed=11).train()
    _lib._warned.clear()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = pol(env.reset(data), env, phase="train", decode_type="sampling", seed=5)
    ours = [x for x in w if issubclass(x.category, RuntimeWarning) and "rl4co_amd" in str(x.message)]
    assert len(ours) == 1 and "four-scalar context" in str(ours[0].message), [str(x.message) for x in w]
    reward, ll, acts = out["reward"], out["log_likelihood"], out["actions"]
    adv = (reward - reward.mean()).detach()
    (adv * ll).mean().backward()
    got = {k: p.grad.clone() for k, p in pol.named_parameters() if p.grad is not None}
    k_feat = "decoder.context_embedding.proj_dynamic_feats.weight"
    assert k_feat in got and float(got[k_feat].norm()) > 0
    pol.zero_grad()
    # the restatement: the same (torch) encoder, then the reference decoder's algebra step by step along the same actions
    td = env.reset(data)
    hidden, _ = pol.encoder(td)
    st0 = {k: v.cuda() for k, v in mtsp_ref.initial_state(td["locs"].cpu(), td["num_agents"].cpu()).items()}
    ll_ref = mtsp_ref.decoder_step_logps(pol.decoder, hidden.float(), st0, acts).sum(1)
    torch.testing.assert_close(ll.detach(), ll_ref.detach(), rtol=1e-4, atol=1e-4)
    (adv * ll_ref).mean().backward()
    want = {k: p.grad for k, p in pol.named_parameters() if p.grad is not None}
    assert sorted(got) == sorted(want)
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
    assert float(want[k_feat].norm()) > 1e-6 * total  # the running scalars' layer learns


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(K, forced, policy):
    from rl4co_amd import _lib
    from rl4co_amd.envs import get_env
    from rl4co_amd.graph import GraphedRollout

    locs, num_agents, acts = forced[21]
    b, steps = acts.shape
    cache = _random_cache(b, 21, torch.bfloat16)

    def run(variant="auto", max_steps=steps, mode="evaluate", **kw):
        st = {k: v.cuda() for k, v in mtsp_ref.initial_state(locs, num_agents).items()}
        out_a = torch.zeros(b, steps, dtype=torch.int64, device="cuda")
        lps = torch.zeros(b, steps, device="cuda")
        err = K.new_error_word("cuda")
        K.am_decode(cache, st, mode=mode, max_steps=max_steps, actions=out_a, logps=lps, err=err,
                    forced_actions=acts.cuda(), variant=variant, **kw)
        return int(err.item()), out_a, lps

    with pytest.raises(_lib.Rl4coLibraryError, match="variant >= 0"):  # the multistart variant, pinned
        run("ms")
    assert K.decode_variant(21, torch.bfloat16, 42, 4096 * 8, 4096, env_name="mtsp") != _lib.VARIANT_MS  # auto skips it
    rec = mtsp_ref.record("mtsp20_greedy")
    env, td = _env_td(rec)
    with pytest.raises(NotImplementedError, match="multistart"):
        policy(td, env, phase="test", decode_type="multistart_greedy", num_starts=4)
    with pytest.raises(ValueError, match="unfolded parity mode serves tsp / cvrp"):
        _policy(fold=False)(_env_td(rec)[1], phase="test", decode_type="greedy")
    with pytest.raises(NotImplementedError, match="cost_type"):
        get_env("mtsp", cost_type="sum")
    with pytest.raises(NotImplementedError, match="captured-graph"):
        GraphedRollout(policy, env, env.generator(batch_size=[8]), decode_type="greedy")
    with pytest.raises(NotImplementedError, match="one-launch replay"):
        K.env_replay("mtsp", policy._initial_state(td, 0), rec["actions"].cuda(), None)
    from rl4co_amd import teacher

    assert not teacher.supports("mtsp", torch.bfloat16, 20)
    with pytest.raises(NotImplementedError, match="teacher-forced backward kernels serve"):
        teacher.teacher_forced_logps("mtsp", {}, None, rec["actions"].cuda(), torch.zeros(64, 24, device="cuda"), {})
    with pytest.raises(NotImplementedError, match="teacher-forced backward kernels serve"):
        teacher.run_backward(_random_cache(b, 21, torch.bfloat16), acts.cuda(), torch.zeros(b, steps, device="cuda"), {})
    # a horizon too short: the sticky bit, and nothing behind the columns it was given
    short = 5
    err, out_a, lps = run("stream", max_steps=short)
    assert err & _lib.EBIT_MAX_STEPS
    assert bool((out_a[:, short:] == 0).all()) and bool((lps[:, short:] == 0).all())
    with pytest.raises(AssertionError, match="Exceeded maximum number of steps"):
        _lib.raise_for_error_bits(err)
