"""GPU (`-m gpu`): the streaming decode kernel with a step's scores held in registers (am_decode.hip, variant
"stream_reg" = RL4CO_VARIANT_STREAM_REG).

Only where a value waits between pass 1 and pass 2 differs from "stream" — registers instead of LDS — and the LDS that
frees goes to a larger row cache: the kernel equals the C specified-order oracle and "stream" bit for bit, and its row
counter (steps_summary words 2..3) equals the host's replay of the residency rule with the capacity of the new layout
(the replay is restated here; tests/test_gpu_decode_row_cache.py keeps the one for "stream")."""
import os

import pytest
import torch

from oracle import c_oracle
from tests.helpers import apply_step, fold_cache, make_instances, make_policy, max_horizon, rollout_state

pytestmark = pytest.mark.gpu

KNOB = "RL4CO_DECODE_ROW_CACHE"
HALF = [torch.bfloat16, torch.float16]
HALF_IDS = ["bf16", "f16"]


@pytest.fixture(scope="module")
def K():
    from rl4co_amd import kernels

    return kernels


@pytest.fixture
def knob():
    """Sets the row-cache knob for the launches a test makes; restores the environment afterwards."""
    old = os.environ.get(KNOB)

    def set_(v):
        if v is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = str(v)

    set_(None)
    yield set_
    set_(old)


_CASES = {}


def _case(env_name: str, num_loc: int, batch: int):
    key = (env_name, num_loc, batch)
    if key not in _CASES:
        env, data = make_instances(env_name, num_loc, batch)
        pol = make_policy(env_name)
        td0 = env.reset(data)
        with torch.inference_mode():
            h, _ = pol.encoder(td0)
        _CASES[key] = (pol, td0, h)
    return _CASES[key]


def _run(K, backend, env_name, num_loc, batch, mode, dtype, noise_seed=None, variant="stream_reg", split=None,
         want_all=False, **kw):
    """One whole rollout on ``backend`` in {"hip", "c"}; ``split``: two launches, the second from step ``split`` on
    (t0 / max_steps), the state carried between them. Returns a dict of outputs."""
    pol, td0, h = _case(env_name, num_loc, batch)
    dev = "cuda" if backend == "hip" else "cpu"
    cache = fold_cache(pol, env_name, h, dtype, device="cuda")
    if backend == "c":
        cache = cache.to("cpu")
    st = rollout_state(env_name, td0, device=dev)
    b, n = st["action_mask"].shape
    tmax = max_horizon(env_name, n)
    noise = None
    if noise_seed is not None:
        g = torch.Generator().manual_seed(noise_seed)
        noise = torch.empty(tmax, b, n).exponential_(1, generator=g).contiguous().to(dev)
    actions = torch.zeros(b, tmax, dtype=torch.int64, device=dev)
    logps = torch.zeros(b, tmax, device=dev)
    n_steps = torch.zeros(b, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    out = dict(actions=actions, logps=logps, n_steps=n_steps, state=st)
    if want_all:
        out["all_logps"] = kw["all_logps"] = torch.zeros(b, tmax, n, device=dev)
        out["entropy"] = kw["entropy"] = torch.zeros(b, device=dev)
    legs = [(0, tmax)] if split is None else [(0, split), (split, tmax - split)]
    rows = 0
    total_steps = torch.zeros(b, dtype=torch.int32, device=dev)
    for t0, steps in legs:
        leg = dict(kw, t0=t0)
        if noise is not None:
            leg["exp_noise"] = noise[t0:].contiguous()  # (the draws are indexed by the launch's own step)
        if backend == "hip":
            summary = torch.zeros(4, dtype=torch.int32, device=dev)
            K.am_decode(cache, st, mode=mode, max_steps=steps, actions=actions, logps=logps, err=err, n_steps=n_steps,
                        steps_summary=summary, variant=variant, **leg)
            torch.cuda.synchronize()
            lo, hi = summary[2:4].cpu().tolist()
            rows += (hi << 32) | (lo & 0xFFFFFFFF)
        else:
            groups = K.decode_row_groups(n, dtype, steps, variant, b)
            c_oracle.am_decode(cache, st, mode=mode, max_steps=steps, actions=actions, logps=logps, err=err,
                               n_steps=n_steps, row_groups=groups, **leg)
        total_steps += n_steps
    out["n_steps"] = total_steps
    out["rows"] = rows
    out["err"] = int(err.item())
    if split is not None:
        out["err"] &= ~16  # RL4CO_EBIT_MAX_STEPS: the first leg stops before the tours end, on both sides
    return {k: ({kk: vv.cpu() for kk, vv in v.items()} if isinstance(v, dict) else (v.cpu() if torch.is_tensor(v) else v))
            for k, v in out.items()}


def _assert_same(x, y):
    assert x["err"] == y["err"] == 0
    assert torch.equal(x["n_steps"], y["n_steps"])
    assert torch.equal(x["actions"], y["actions"]), f"{int((x['actions'] != y['actions']).any(1).sum())} tours differ"
    assert torch.equal(x["logps"].view(torch.int32), y["logps"].view(torch.int32)), "log-probs not bit-identical"
    for k in y["state"]:
        assert torch.equal(x["state"][k], y["state"][k]), f"final state {k} differs"
    for k in ("all_logps", "entropy"):
        if k in y:
            assert torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)), f"{k} not bit-identical"


def _capacity_slots(n: int) -> int:
    """Slots of the register-score layout (16-bit planes): scratch = lg | fl | mk | vis = 8 bytes per padded node; the
    most slots for which a CU still holds as many workgroups as that scratch alone lets it, at most 16, with 512 B or
    1280 B LDS granules; capped at N and 255."""
    pad = (n + 63) & ~63
    base = pad * 8

    def per_cu(b, g):
        return min(16, 160 * 1024 // ((b + g - 1) // g * g))

    s = 0
    while s < min(n, 255):
        b = base + (s + 1) * 3 * 128 * 2 + pad + s + 1
        if per_cu(b, 512) < per_cu(base, 512) or per_cu(b, 1280) < per_cu(base, 1280) or b > 160 * 1024:
            break
        s += 1
    return s


def _expected_rows(env_name, num_loc, batch, out, S, list_all=False):
    """HBM rows of the rollout `out`, replayed on the host: the feasible list of every step, the S highest-index
    candidates resident, a slot freed by a visited node handed to the highest candidate not resident, pending until
    the next step that lists it has read its rows from HBM."""
    _, td0, _ = _case(env_name, num_loc, batch)
    st = rollout_state(env_name, td0)
    b, n = st["action_mask"].shape
    steps = out["n_steps"].tolist()
    slot = [dict() for _ in range(b)]  # node -> pending flag
    total = 0
    for t in range(max(steps)):
        mask = st["action_mask"].clone()
        vis = st["visited"].clone() if env_name == "cvrp" else None

        def cand(r, j):
            return list_all or (bool(mask[r, j]) if env_name == "tsp" else (j == 0 or not bool(vis[r, j])))

        for r in range(b):
            if t >= steps[r]:
                continue
            res = slot[r]
            if t == 0 and S > 0:
                for j in [j for j in range(n - 1, -1, -1) if cand(r, j)][:S]:
                    res[j] = True
            lst = list(range(n)) if list_all else [j for j in range(n) if bool(mask[r, j])]
            f = len(lst)
            hend = max(f - S, 0)
            for c in range(max(f - S, 0), f):
                if lst[c] not in res or res[lst[c]]:
                    hend = c + 1
            total += hend
            for c in range(hend):
                if lst[c] in res:
                    res[lst[c]] = False
        a = out["actions"][:, t].clone()
        apply_step(c_oracle, env_name, a, st)
        mask = st["action_mask"]
        vis = st["visited"] if env_name == "cvrp" else None
        for r in range(b):
            if t >= steps[r]:
                continue
            j = int(a[r])
            if j in slot[r] and not cand(r, j):
                del slot[r][j]
                free = [k for k in range(n) if cand(r, k) and k not in slot[r]]
                if free:
                    slot[r][max(free)] = True
    return total


# ---- bit-exact against the C oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF, ids=HALF_IDS)
@pytest.mark.parametrize("mode", ["greedy", "sampling"])
@pytest.mark.parametrize("num_loc", [5, 17, 100, 112])
def test_tsp_bit_exact_vs_c_oracle(K, knob, num_loc, mode, dtype):
    """5: less than one load; 17: one row past a 16-entry batch; 112: the last register slot."""
    seed = 7 if mode == "sampling" else None
    _assert_same(_run(K, "hip", "tsp", num_loc, 64, mode, dtype, seed), _run(K, "c", "tsp", num_loc, 64, mode, dtype, seed))


@pytest.mark.parametrize("dtype", HALF, ids=HALF_IDS)
@pytest.mark.parametrize("mode", ["greedy", "sampling"])
@pytest.mark.parametrize("num_loc", [50, 100, 111])
def test_cvrp_bit_exact_vs_c_oracle(K, knob, num_loc, mode, dtype):
    """The depot comes back into the list, capacity-infeasible resident nodes drop out of it; 111: N = 112."""
    seed = 11 if mode == "sampling" else None
    _assert_same(_run(K, "hip", "cvrp", num_loc, 64, mode, dtype, seed), _run(K, "c", "cvrp", num_loc, 64, mode, dtype, seed))


@pytest.mark.parametrize("env_name", ["tsp", "cvrp"])
def test_mask_inner_off_bit_exact_vs_c_oracle(K, knob, env_name):
    _assert_same(_run(K, "hip", env_name, 20, 64, "greedy", torch.bfloat16, mask_inner=False),
                 _run(K, "c", env_name, 20, 64, "greedy", torch.bfloat16, mask_inner=False))


@pytest.mark.parametrize("env_name", ["tsp", "cvrp"])
def test_all_logps_and_entropy_bit_exact_vs_c_oracle(K, knob, env_name):
    _assert_same(_run(K, "hip", env_name, 20, 64, "sampling", torch.bfloat16, 3, want_all=True),
                 _run(K, "c", env_name, 20, 64, "sampling", torch.bfloat16, 3, want_all=True))


@pytest.mark.parametrize("env_name,num_loc,split", [("tsp", 100, 37), ("cvrp", 50, 20)])
def test_rollout_split_in_two_launches(K, knob, env_name, num_loc, split):
    """The second launch starts past step 0 with the state of the first (TSP: first node set, placeholder gone)."""
    two = _run(K, "hip", env_name, num_loc, 64, "sampling", torch.bfloat16, 5, split=split)
    _assert_same(two, _run(K, "c", env_name, num_loc, 64, "sampling", torch.bfloat16, 5, split=split))
    one = _run(K, "hip", env_name, num_loc, 64, "sampling", torch.bfloat16, 5)
    assert torch.equal(one["actions"], two["actions"]) and torch.equal(one["logps"].view(torch.int32), two["logps"].view(torch.int32))


def test_top_k_top_p_is_not_served(K, knob):
    """The filter's build of this kernel does not fit four waves per SIMD: an explicit request is refused, `auto` keeps
    "stream" for it (and is checked there by tests/test_gpu_topkp.py)."""
    from rl4co_amd import _lib

    with pytest.raises(_lib.Rl4coLibraryError):
        _run(K, "hip", "tsp", 20, 64, "sampling", torch.bfloat16, 3, top_k=5)
    with pytest.raises(_lib.Rl4coLibraryError):
        _run(K, "hip", "tsp", 20, 64, "sampling", torch.bfloat16, 3, top_p=0.9)


# ---- bit-identical to "stream" -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0, None], ids=["knob0", "default"])
@pytest.mark.parametrize("env_name", ["tsp", "cvrp"])
def test_equals_stream(K, knob, env_name, cap):
    knob(cap)
    reg = _run(K, "hip", env_name, 100, 64, "sampling", torch.bfloat16, 3)
    stream = _run(K, "hip", env_name, 100, 64, "sampling", torch.bfloat16, 3, variant="stream")
    _assert_same(reg, stream)
    if cap == 0:
        assert reg["rows"] == stream["rows"]
    else:
        assert reg["rows"] < stream["rows"]


# ---- row counter -----------------------------------------------------------------------------------------------------------
def test_capacity_is_11_slots_at_100_nodes():
    assert _capacity_slots(100) == 11 and _capacity_slots(101) == 11


@pytest.mark.parametrize("cap", [None, 0, 3, 255])
@pytest.mark.parametrize("env_name,num_loc,dtype", [("tsp", 100, torch.bfloat16), ("cvrp", 50, torch.float16),
                                                  ("tsp", 5, torch.bfloat16)])
def test_hbm_row_count_matches_host_replay(K, knob, env_name, num_loc, dtype, cap):
    knob(cap)
    out = _run(K, "hip", env_name, num_loc, 32, "sampling", dtype, 5)
    assert out["err"] == 0
    n = num_loc + (env_name == "cvrp")
    slots = _capacity_slots(n) if cap is None else min(cap, _capacity_slots(n))
    assert out["rows"] == _expected_rows(env_name, num_loc, 32, out, slots)
    if cap == 0:  # every listed row, every step
        assert out["rows"] == _expected_rows(env_name, num_loc, 32, out, 0)
        if env_name == "tsp":
            assert out["rows"] == 32 * n * (n + 1) // 2


def test_mask_off_row_count_matches_host_replay(K, knob):
    out = _run(K, "hip", "cvrp", 20, 32, "greedy", torch.bfloat16, mask_inner=False)
    assert out["err"] == 0
    assert out["rows"] == _expected_rows("cvrp", 20, 32, out, _capacity_slots(21), list_all=True)


# ---- selection (host queries, no launch) ---------------------------------------------------------------------------------
def test_selection(K):
    from rl4co_amd import _lib

    reg, stream = _lib.VARIANT_STREAM_REG, _lib.VARIANT_STREAM
    assert reg == 5 and K.VARIANT_IDS["stream_reg"] == 5
    assert K.decode_variant(100, torch.bfloat16, 99, 4096) == reg  # (the measured default)
    assert K.decode_variant(100, torch.float16, 99, 4096) == reg
    assert K.decode_variant(101, torch.bfloat16, 202, 4096, env_name="cvrp") == reg
    assert K.decode_variant(112, torch.bfloat16, 111, 4096) == reg
    assert K.decode_variant(100, torch.bfloat16, 3, 4096) == stream  # fewer than 4 steps
    assert K.decode_variant(113, torch.bfloat16, 112, 4096) == stream
    assert K.decode_variant(100, torch.float32, 99, 4096) == stream
    assert K.decode_variant(100, torch.bfloat16, 99, 4096, env_name="pctsp") == stream
    for n, dtype in ((113, torch.bfloat16), (100, torch.float32)):
        with pytest.raises(_lib.Rl4coLibraryError):
            K.decode_row_groups(n, dtype, 99, "stream_reg", 4096)
    assert K.decode_row_groups(100, torch.bfloat16, 99, "stream_reg", 4096) == 4
    assert K.decode_row_groups(100, torch.bfloat16, 99, "auto", 4096) == 4
