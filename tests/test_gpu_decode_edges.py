"""GPU (`-m gpu`): OP, PCTSP, PDP and CVRPTW (and CVRP / TSP at three sizes) on the fused decode kernels at the sizes where the
kernels change shape — the 64-lane boundary (N = 63, 64, 65), two and more passes per wave (128, 129, 257), the pad-to-4 and
pad-to-64 roundings, the LDS-resident variant's last size and the first it must refuse (101, 102; PDP 101, 103), the MFMA
variant's N <= 128, and N >= 129 where only WIDE and STREAM remain. Until here these four ran at the golden records' 21, 51 and
101 nodes only, and their arithmetic was checked against ``oracle/rollout_ref.c`` alone — the kernels' own algebra.

 a. teacher-forced, every variant / plane-type pair against the float64 restatement of the decode step
    (tests/decode_f64_ref.py, pinned to the reference decoder and proven against the C oracle and five seeded mistakes by
    tests/test_decode_f64_cpu.py). Tolerance per case, never from a kernel's output: ``max(FLOOR, 4 x dev32)``
    (``decode_f64_ref.tolerance``). Every case asserts on the CPU side that its walk exercises what it is there for
    (``decode_f64_ref.walk_facts``).
 b. free-running (greedy, sampling on injected noise, the in-kernel Philox stream), bit for bit against the C oracle.
 c. the multistart MFMA variant, which has no bit-exact oracle: feasibility and final state through the C oracle's step
    entries, log-probs within ``MS_LOGP_TOL`` of ``step_f64`` on the kernel's own actions, and the float64 argmax wherever
    the float64 top-two gap exceeds ``2 * MS_LOGP_TOL``.

A pinned LDS-resident build beyond its last size is refused, and no other kernel runs in its place: those cases assert the
refusal. Every test prints ``dev32``, the kernel's deviation, the bound and their ratio.

Measured on the MI355X (kernel deviation / bound, the largest per environment): teacher-forced tsp 0.177,
cvrp 0.114, op 0.118, pctsp 0.176, pdp 0.144, cvrptw 0.174 (all on STREAM; at most 1.23e-6 against 6.91e-6); multistart MFMA
bf16 0.364 / 0.298 / 0.352 / 0.400 (op / pctsp / pdp / cvrptw; 2.00e-3 against 5e-3), f16 at most 0.048. Every free-running
case is bit for bit the C oracle's. Nothing here found a defect in a kernel or in the C oracle."""
import pytest
import torch

from tests import decode_f64_ref as D
from tests.helpers import apply_step, max_horizon
from tests.test_gpu_decode_f64 import VARIANTS, VIDS
from tests.test_gpu_decode_ms import MS_LOGP_TOL

pytestmark = pytest.mark.gpu

FOUR = ("op", "pctsp", "pdp", "cvrptw")


def _cid(case):
    return f"{case[0]}-n{case[1]}-b{case[2]}"


@pytest.fixture(scope="module")
def K():
    from rl4co_amd import kernels

    return kernels


_CASES, _REFS, _C_RUNS = {}, {}, {}


def _case(case):
    """(initial state, forced actions, walk facts) of an edge case, computed once."""
    if case not in _CASES:
        st0, acts = D.forced_case(*case)
        _CASES[case] = (st0, acts, D.walk_facts(case[0], st0, acts))
    return _CASES[case]


def _reference(cache, st0, acts, key):
    """The float64 rollout along ``acts`` and the case's tolerance from its float32 twin, computed once per ``key``."""
    if key not in _REFS:
        want = D.rollout(cache, st0, acts)
        dev32 = D.fp32_cost(want, D.rollout(cache, st0, acts, step=D.step_f32))
        _REFS[key] = (want, dev32, D.tolerance(cache.env_name, dev32))
    return _REFS[key]


def _buffers(st0, steps):
    b = st0["action_mask"].shape[0]
    return ({k: v.clone().cuda() for k, v in st0.items()}, torch.zeros(b, steps, dtype=torch.int64, device="cuda"),
            torch.zeros(b, steps, device="cuda"), torch.zeros(b, dtype=torch.int32, device="cuda"))


def _launch(K, cache, st0, steps, variant, mode, t0=0, first=None, **kw):
    """``steps`` columns of output, the decode from column ``t0`` (``first``: the multistart nodes, stepped on the GPU)."""
    st, out_a, lps, n_steps = _buffers(st0, steps)
    err = K.new_error_word("cuda")
    if first is not None:
        out_a[:, 0] = first.cuda()
        K.env_step(cache.env_name, st, first.cuda().contiguous(), err)
    kw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}
    K.am_decode(cache.to("cuda"), st, mode=mode, max_steps=steps - t0, t0=t0, actions=out_a, logps=lps, err=err,
                n_steps=n_steps, variant=variant, **kw)
    return {k: v.cpu() for k, v in st.items()}, out_a.cpu(), lps.cpu(), n_steps.cpu(), int(err.item())


def _refused(K, cache, st0, steps, variant, dtype, mode, **kw):
    """The LDS-resident build keeps a trajectory's three 16-bit planes and its scratch in half a CU's LDS: pinned beyond its
    last size (``decode_row_groups`` says which that is) the library must refuse, and no other kernel runs in its place —
    the outputs and the state stay as they were. True if this launch is such a one (and was refused)."""
    from rl4co_amd import _lib

    n = cache.num_nodes
    if variant != "lds":
        return False
    try:
        K.decode_row_groups(n, dtype, steps, "lds", st0["action_mask"].shape[0])
        assert n <= D.LDS_MAX_N
        return False
    except _lib.Rl4coLibraryError:
        assert n > D.LDS_MAX_N
    st, out_a, lps, n_steps = _buffers(st0, steps)
    err = K.new_error_word("cuda")
    kw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}
    with pytest.raises(_lib.Rl4coLibraryError, match="variant >= 0"):
        K.am_decode(cache.to("cuda"), st, mode=mode, max_steps=steps, actions=out_a, logps=lps, err=err, n_steps=n_steps,
                    variant=variant, **kw)
    torch.cuda.synchronize()
    assert int(err.item()) == 0 and not bool(lps.any()) and not bool(out_a.any()) and not bool(n_steps.any())
    for k, v in st0.items():
        assert torch.equal(st[k].cpu(), v), k
    return True


def test_lds_limit_is_the_librarys(K):
    """The case table's LDS sizes are the library's: the last size served, and the next one (PDP: the next odd one) refused."""
    from rl4co_amd import _lib

    for dtype in (torch.bfloat16, torch.float16):
        assert K.decode_row_groups(D.LDS_MAX_N, dtype, 2 * D.LDS_MAX_N, "lds", 6) == 16
        for n in (D.LDS_MAX_N + 1, D.LDS_MAX_N + 2):
            with pytest.raises(_lib.Rl4coLibraryError):
                K.decode_row_groups(n, dtype, 2 * n, "lds", 6)
    for env_name in FOUR:
        assert D.LDS_MAX_N in D.EDGE_SIZES[env_name] and D.LDS_MAX_N + (2 if env_name == "pdp" else 1) in D.EDGE_SIZES[env_name]


# ---- a. teacher-forced against float64 ----------------------------------------------------------------------------------------------
def _assert_exercised(case, facts):
    """What the case is there for, from the restatement's walk alone. The conditions on a row's course need room: from
    n = 63 (at n = 3 there are two customers; OP's n = 3 walk is still cut by its length limit)."""
    env_name, n, _ = case
    if n >= 65:
        assert facts["max_node"] >= 64
    if n >= 129:
        assert facts["max_node"] >= 128
    if env_name == "op":
        assert facts["length_cut"]
    if env_name == "pctsp":
        assert facts["home_early"] and facts["home_full"]
    if env_name == "cvrptw":
        assert facts["time_window_masked"]
    if env_name in ("cvrp", "cvrptw") and n >= 63:
        assert int(facts["depot_returns"].max()) >= 3


@pytest.mark.parametrize("variant,dtype", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("case", D.edge_cases(), ids=_cid)
def test_teacher_forced_log_probs_against_float64(K, case, variant, dtype):
    env_name, n, b = case
    st0, acts, facts = _case(case)
    steps = acts.shape[1]
    assert steps <= max_horizon(env_name, n)
    _assert_exercised(case, facts)
    cache = D.random_cache(env_name, b, n, dtype)
    if _refused(K, cache, st0, steps, variant, dtype, "evaluate", forced_actions=acts):
        return
    want, dev32, tol = _reference(cache, st0, acts, (case, dtype))
    st, out_a, lps, n_steps, err = _launch(K, cache, st0, steps, variant, "evaluate", forced_actions=acts)
    assert err == 0
    assert torch.equal(out_a, acts)
    for k, v in want["state"].items():
        assert torch.equal(st[k], v), k
    ex = want["executed"]
    assert bool(want["state"]["done"].all()) and bool(torch.isfinite(want["chosen"][ex]).all())
    dev = float((lps.double() - want["chosen"])[ex].abs().max())
    print(f"{_cid(case)} {variant}: dev32 {dev32:.3e}, kernel {dev:.3e}, bound {tol:.3e}, ratio {dev / tol:.3f} over "
          f"{int(ex.sum())} steps")
    assert dev <= tol
    assert bool((lps[~ex] == 0).all()) and bool((out_a[~ex] == 0).all())  # behind done: the padding action, log-prob 0


# ---- b. free-running, bit for bit against the C oracle ------------------------------------------------------------------------------
FREE_SIZES = {env_name: [3, 63 if env_name == "pdp" else 64, 65, 129] for env_name in FOUR}
FREE_CASES = [(env_name, n) for env_name in FOUR for n in FREE_SIZES[env_name]]
PHILOX = dict(philox_seed=0x1234ABCD5678, philox_offset=7)


def _noise(b, n, steps, seed):
    torch.manual_seed(seed)
    return torch.stack([torch.empty(b, n).exponential_(1) for _ in range(steps)], 0).contiguous()


def _free_running(K, env_name, n, mode, variant, dtype, **kw):
    b = 6
    st0 = D.six_state(env_name, n, b)
    cache = D.random_cache(env_name, b, n, dtype)
    steps = max_horizon(env_name, n)
    if mode == "noise":
        kw = dict(exp_noise=_noise(b, n, steps, 4321 + n))
    mode_name = "greedy" if mode == "greedy" else "sampling"
    if _refused(K, cache, st0, steps, variant, dtype, mode_name, **kw):
        return
    groups = K.decode_row_groups(n, dtype, steps, variant, b)
    key = (env_name, n, mode, dtype, groups)
    if key not in _C_RUNS:
        _C_RUNS[key] = D.c_decode(cache, st0, mode_name, steps, groups, **kw)
    ref = _C_RUNS[key]
    st, out_a, lps, n_steps, err = _launch(K, cache, st0, steps, variant, mode_name, **kw)
    assert err == ref["err"] == 0
    assert bool(ref["state"]["done"].all())
    assert torch.equal(n_steps, ref["n_steps"])
    assert torch.equal(out_a, ref["actions"]), f"{int((out_a != ref['actions']).any(1).sum())} trajectories differ from the C oracle"
    assert torch.equal(lps.view(torch.int32), ref["logps"].view(torch.int32)), "log-probabilities are not bit-identical"
    for k, v in ref["state"].items():
        assert torch.equal(st[k], v), f"final state {k} differs"


@pytest.mark.parametrize("variant,dtype", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("mode", ["greedy", "noise"])
@pytest.mark.parametrize("env_name,n", FREE_CASES, ids=[f"{e}-n{n}" for e, n in FREE_CASES])
def test_free_running_bit_exact_vs_c_oracle(K, env_name, n, mode, variant, dtype):
    _free_running(K, env_name, n, mode, variant, dtype)


@pytest.mark.parametrize("env_name,n", FREE_CASES, ids=[f"{e}-n{n}" for e, n in FREE_CASES])
def test_free_running_philox_bit_exact_vs_c_oracle(K, env_name, n):
    """The in-kernel Philox stream, which the C oracle also draws (stream-bf16)."""
    _free_running(K, env_name, n, "philox", "stream", torch.bfloat16, **PHILOX)


# ---- c. the multistart MFMA variant ------------------------------------------------------------------------------------------------
MS_CASES = [(env_name, n) for env_name in FOUR for n in (21, 65, 113, 127 if env_name == "pdp" else 128)]


def _start_nodes(st_inst, starts):
    """``starts`` nodes per instance, feasible under the reset mask, s-major over the instances."""
    mask = st_inst["action_mask"].bool()
    g = torch.Generator().manual_seed(starts)
    first = torch.multinomial(mask.float(), starts, replacement=True, generator=g)  # [B_inst, S]
    return first.t().reshape(-1).contiguous()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("starts", [5, 8])
@pytest.mark.parametrize("env_name,n", MS_CASES, ids=[f"{e}-n{n}" for e, n in MS_CASES])
def test_multistart_mfma_variant_against_float64(K, env_name, n, starts, dtype):
    from oracle import c_oracle

    b_inst = 3
    st_inst = D.six_state(env_name, n, b_inst)
    st0 = D.six_state(env_name, n, b_inst, num_starts=starts)
    b = starts * b_inst
    assert st0["action_mask"].shape == (b, n)
    first = _start_nodes(st_inst, starts)
    inst = torch.arange(b) % b_inst
    assert bool(st_inst["action_mask"].bool()[inst, first].all())  # feasible under the reset mask, every row
    # Planes at half the scale of the other tests' (0.25): this kernel rounds the query, the softmax numerators and the
    # glimpse to 16 bits (relative 2^-9 each), so its log-prob error grows with the logits, which are bilinear in the
    # planes. MS_LOGP_TOL was measured on encoder outputs (largest 2.1e-3); at scale 0.5 the project's own rounding model
    # (oracle_am_decode_ms, on the CPU) already leaves float64 by 4e-3 - 7e-3, so the bound would judge the number format,
    # not the kernel. At 0.25 the logits are 4 x smaller and the model stays under 2.1e-3, the figure the bound was set
    # from; 60 - 95 % of the steps still have a clear float64 argmax.
    cache = D.random_cache(env_name, b_inst, n, dtype, scale=0.25)
    tmax = max_horizon(env_name, n)
    st, out_a, lps, n_steps, err = _launch(K, cache, st0, tmax, "ms", "greedy", t0=1, first=first)
    assert err == 0
    assert torch.equal(out_a[:, 0], first)
    st1 = {k: v.clone() for k, v in st0.items()}
    apply_step(c_oracle, env_name, first, st1)
    t = int(n_steps.max())
    acts, lps = out_a[:, 1 : 1 + t].contiguous(), lps[:, 1 : 1 + t].double()
    assert bool((out_a[:, 1 + t :] == 0).all())
    want, dev32, _ = _reference(cache, st1, acts, (env_name, n, starts, dtype, acts.numpy().tobytes()))
    ex = want["executed"]
    assert torch.equal(ex.sum(1).to(torch.int32), n_steps)
    assert bool(want["masks"].gather(2, acts[:, :, None])[:, :, 0][ex].all())  # every action is feasible
    assert bool(want["state"]["done"].all())
    for k, v in want["state"].items():
        assert torch.equal(st[k], v), f"final state {k} differs"
    dev = float((lps - want["chosen"])[ex].abs().max())
    top2 = want["logps"].topk(2, -1)[0]
    gap = top2[..., 0] - top2[..., 1]  # (inf where one node is feasible)
    clear = ex & (gap > 2 * MS_LOGP_TOL)
    print(f"{env_name}-n{n} S={starts} {dtype}: dev32 {dev32:.3e}, kernel {dev:.3e}, bound {MS_LOGP_TOL:.3e}, ratio "
          f"{dev / MS_LOGP_TOL:.3f} over {int(ex.sum())} steps, {int(clear.sum())} of them with a clear float64 argmax")
    assert torch.equal(acts[clear], want["logps"].argmax(-1)[clear])
    assert dev <= MS_LOGP_TOL
    assert bool((lps[~ex] == 0).all()) and bool((acts[~ex] == 0).all())
