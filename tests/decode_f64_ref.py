"""A float64 restatement of ONE folded decode step of the two environments the C specified-order oracle does not know: the
split-delivery VRP (rank-one dynamic term ``d_j (x . u)`` from ``FoldedCache.dyn``) and the min-max multi-agent TSP (four
running scalars through ``FoldedCache.feat``). Pure torch, any device, no kernel: the algebra of the am_decode.hip header
and DESIGN §4.9 / §4.10 on the bytes the kernels read —

    q       = ctx_cur[cur] + q_bias + (cap - used) w_cap                         (SDVRP)
            = ctx_cur[cur] + q_bias + sum_k f_k feat[k]                          (mTSP; f = mtsp_ref.features)
    d_j     = remaining demand of node j, the depot's taken as 0 (SDVRP; 0 for mTSP)
    head h  : p = softmax over the feasible j of q_h . (K_j + d_j u_k)_h / sqrt(16) ;  o_h = sum_j p_j (V_j + d_j u_v)_h
    z_j     = 10 tanh(o . (L_j + d_j u_l') / sqrt(128)), -inf where infeasible, / temperature ;  logp = log_softmax(z)

The planes are widened exactly (``.double()`` on the stored 16-bit or fp32 values); the state scalars the kernels compute in
fp32 (``cap - used``, the four features) are taken in fp32 from the restatements' state and widened, so the only difference
between a kernel and ``step_f64`` is the fp32 rounding of the kernel's own sums, exp, tanh and log. ``step_f32`` is the same
function in float32: what fp32 arithmetic alone costs on the same inputs (the tests' tolerance is built from it, never from
a kernel's output). The state is stepped with ``sdvrp_ref`` / ``mtsp_ref`` (``freeze_done``: a rollout kernel stops a row at
its ``done``). Pinned to the reference decoder's algebra and to the reference's records by tests/test_decode_f64_cpu.py.

The six environments the C oracle does know (tsp, cvrp, op, pctsp, pdp, cvrptw) are restated here too, so that the kernels and
``oracle/rollout_ref.c`` — one author, one algebra — are both judged by a third statement. Only the query differs; it is read
off the environment's record (``rl4co_amd/envspec.py``: ``ctx_first``, ``Scalar``) and the fold (``rl4co_amd/cache.py``):

    q       = q_step0 + q_bias at step 0, else ctx_first[first] + ctx_cur[cur] + q_bias                      (ctx_first: TSP)
            = ctx_cur[cur] + q_bias                                                                          (no scalar: PDP)
            = ctx_cur[cur] + q_bias + s w_cap [+ clock w_time],  s = base - running [clamped at 0 from below]    (Scalar)

``s`` is computed in fp32 from the state and widened, like SDVRP's; ``base`` is a per-trajectory state tensor or column 0 of an
instance table (OP's ``max_length``). A cache of B_inst instances serves B = S x B_inst trajectory rows, s-major (row r reads
instance r % B_inst), as the multistart kernels lay them out. The state of these six is the flat state of
``tests.helpers.rollout_state``, stepped by ``oracle.c_oracle``'s step entries (``tests.helpers.apply_step``)."""
import math

import torch

from tests import mtsp_ref, sdvrp_ref

NUM_HEADS = 8
REFS = {"sdvrp": sdvrp_ref, "mtsp": mtsp_ref}
SIX = ("tsp", "cvrp", "op", "pctsp", "pdp", "cvrptw")  # the C oracle's environments: flat state, stepped by its entries
# The seeded mistakes of the six's query (tests/test_decode_f64_cpu.py): ``_step(..., mistake=name)`` evaluates the wrong formula.
MISTAKES = ("pctsp: scalar not clamped", "op: scalar from the current node's max_length column",
            "cvrptw: no w_time term", "tsp: ctx_first and ctx_cur swapped", "q_bias left out")
# The floor of ``tolerance`` for the six: 4 x the largest ``dev32`` (|step_f32 - step_f64| over every finite log-prob of
# every executed step) over all of ``edge_cases()`` and the three plane types, measured on the CPU from this restatement
# alone (``python -m tests.decode_f64_ref`` prints the table). Below the 2e-5 tests/mtsp_ref.py cites for this class.
MEASURED_DEV32 = 1.727e-6  # op, n = 102, b = 6, fp32 planes (1.7263e-06 rounded up); the other environments 1.1e-6 - 1.6e-6
FLOOR = 4 * MEASURED_DEV32  # 6.908e-6


# The largest N whose three 16-bit planes and scratch the LDS-resident variant holds for the six (no per-trajectory demands
# behind them, unlike SDVRP): what ``kernels.decode_row_groups(n, dtype, steps, "lds")`` serves, asserted by the tests.
LDS_MAX_N = 101
# N (the depot included), the sizes where the kernels change shape: the 64-lane boundary, two and more passes per wave, the
# pad-to-4 and pad-to-64 roundings, the LDS variant's last size and the first it refuses, the MFMA variant's limit, and
# N >= 129 where only WIDE and STREAM remain. PDP has an even number of customers: odd N only.
_EDGE_N = [3, 63, 64, 65, LDS_MAX_N, LDS_MAX_N + 1, 128, 129, 257]
EDGE_SIZES = {"op": _EDGE_N, "pctsp": _EDGE_N, "cvrptw": _EDGE_N, "pdp": [3, 63, 65, LDS_MAX_N, LDS_MAX_N + 2, 127, 129, 257],
              "cvrp": [64, 65, 129], "tsp": [64, 65, 129]}


# The walk's seed where n + 1 does not exercise what the case is there for (``walk_facts``, asserted by the GPU tests): an OP
# row visits a handful of customers, so its walks reach the last node (index >= 64 at n = 65, >= 128 at n = 129) or, at
# n = 3, are cut by the length limit only under some seeds. Found on the CPU from the restatement's walk alone.
WALK_SEEDS = {("op", 3): 6, ("op", 65): 68, ("op", 129): 132}


def edge_cases(envs=SIX) -> list:
    """(env, n, b) of every edge case: 6 rows, 4 at n = 257 (even and odd rows walk differently: both kinds in each)."""
    return [(env, n, 4 if n >= 257 else 6) for env in envs for n in EDGE_SIZES[env]]


def _query_six(cache, st: dict, w, inst, cur, mistake):
    """The six's query, from the environment's record (envspec) and the fold's tables (cache.py)."""
    from rl4co_amd.envspec import rem_base, spec

    sp = spec(cache.env_name)
    dev = cache.kvl.device
    b = cur.shape[0]
    ctx_cur = w(cache.ctx_cur)[inst, cur]
    if sp.ctx_first:
        first = st["first_node"].to(dev).view(-1)
        tables = (w(cache.ctx_first), w(cache.ctx_cur))
        if mistake == "tsp: ctx_first and ctx_cur swapped":
            tables = tables[::-1]
        q = tables[0][inst, first] + tables[1][inst, cur]
        step0 = (st["i"].to(dev).view(-1) == 0)[:, None]
        q = torch.where(step0, w(cache.q_step0)[None, :].expand(b, -1), q)
    else:
        q = ctx_cur
    if cache.q_bias is not None and mistake != "q_bias left out":
        q = q + w(cache.q_bias)[inst]
    if sp.scalar is not None:
        sc = sp.scalar
        base = rem_base(sp, st, b).to(dev).view(-1)
        if mistake == "op: scalar from the current node's max_length column":
            base = st[sc.base].to(dev)[inst, cur]
        s = base - st[sc.running].to(dev).view(-1)  # fp32, as the kernels' state holds it
        assert s.dtype == torch.float32
        if sc.clamp and mistake != "pctsp: scalar not clamped":
            s = s.clamp(min=0)
        q = q + w(s)[:, None] * w(cache.w_cap)
        if sc.clock is not None and mistake != "cvrptw: no w_time term":
            q = q + w(st[sc.clock].to(dev).view(-1))[:, None] * w(cache.w_time)
    return q


def _step(cache, st: dict, dtype, tanh_clipping: float = 10.0, temperature: float = 1.0, zero_depot: bool = True,
          mistake: str | None = None):
    """One decode step of every row of ``st`` (an ``initial_state``-style dict, any device) on ``cache`` in ``dtype``:
    (log-probs [B, N], processed logits z [B, N] (-inf = infeasible), mask [B, N]). ``zero_depot=False`` is a seeded
    mistake for the mutation test (the depot's stored demand enters the dynamic term); ``mistake``: one of ``MISTAKES``."""
    env = cache.env_name
    dev = cache.kvl.device
    w = lambda t: t.to(device=dev, dtype=dtype)  # noqa: E731  (exact for every stored value when dtype is float64)
    mask = st["action_mask"].to(dev).bool().clone()  # (the caller steps the state in place)
    b, n = mask.shape
    d_model = cache.kvl.shape[-1]
    dh = d_model // NUM_HEADS
    cur = st["current_node"].to(dev).view(-1)
    inst = torch.arange(b, device=dev) % cache.num_instances  # (s-major trajectory rows over the instances)
    key, val, lkey = (w(cache.kvl[i])[inst] for i in range(3))
    q = _query_six(cache, st, w, inst, cur, mistake) if env in SIX else w(cache.ctx_cur)[inst, cur] + w(cache.q_bias)
    if env in SIX:
        pass  # (the query is all that differs between them)
    elif env == "sdvrp":
        rem = st["vehicle_capacity"].view(-1) - st["used_capacity"].view(-1)  # fp32, as the kernels' state holds it
        q = q + w(rem)[:, None] * w(cache.w_cap)
        d = w(st["demand_with_depot"]).clone()
        if zero_depot:
            d[:, 0] = 0
        dyn = w(cache.dyn)
        key, val, lkey = (p + d[:, :, None] * u for p, u in zip((key, val, lkey), dyn))
    elif env == "mtsp":
        q = q + w(mtsp_ref.features(st)) @ w(cache.feat)  # (the features: fp32 state arithmetic, widened)
    else:
        raise ValueError(f"the float64 decode step serves sdvrp / mtsp, not {env}")
    scores = torch.einsum("bhd,bnhd->bhn", q.reshape(b, NUM_HEADS, dh), key.reshape(b, n, NUM_HEADS, dh)) / math.sqrt(dh)
    scores = scores.masked_fill(~mask[:, None, :], float("-inf"))
    p = torch.softmax(scores - scores.max(-1, keepdim=True)[0], -1)
    heads = torch.einsum("bhn,bnhd->bhd", p, val.reshape(b, n, NUM_HEADS, dh)).reshape(b, d_model)
    logits = torch.einsum("bd,bnd->bn", heads, lkey) / math.sqrt(d_model)
    z = torch.tanh(logits) * tanh_clipping if tanh_clipping > 0 else logits
    z = z.masked_fill(~mask, float("-inf")) / temperature
    logp = torch.log_softmax(z - z.max(-1, keepdim=True)[0], -1)
    return logp, z, mask


def step_f64(cache, st, **kw):
    return _step(cache, st, torch.float64, **kw)


def step_f32(cache, st, **kw):
    """The same step in float32: the cost of fp32 arithmetic alone on the same inputs."""
    return _step(cache, st, torch.float32, **kw)


def rollout(cache, st0: dict, actions, step=step_f64, **kw) -> dict:
    """``actions`` [B, T] forced through the restatement's state from ``st0`` (CPU, cloned): ``logps`` [B, T, N] of every
    step in the step function's dtype, ``z`` [B, T, N] the processed logits, ``masks`` [B, T, N], ``executed`` [B, T] (the
    row was not done before the step: a rollout kernel evaluates exactly these), ``chosen`` [B, T] the log-prob of the
    forced node, and the final ``state``."""
    st = {k: v.clone() for k, v in st0.items()}
    actions = actions.cpu()
    lps, zs, masks, executed = [], [], [], []
    for t in range(actions.shape[1]):
        executed.append(~st["done"].view(-1).bool().clone())
        lp, z, mask = step(cache, st, **kw)
        lps.append(lp.cpu()), zs.append(z.cpu()), masks.append(mask.cpu())
        step_state(cache.env_name, st, actions[:, t])
    out = {"logps": torch.stack(lps, 1), "z": torch.stack(zs, 1), "masks": torch.stack(masks, 1),
           "executed": torch.stack(executed, 1), "state": st}
    out["chosen"] = out["logps"].gather(2, actions[:, :, None])[:, :, 0]
    return out


def fp32_cost(got64: dict, got32: dict) -> float:
    """``dev32``: the largest |step_f32 - step_f64| over the finite log-probs of the executed steps of the same inputs."""
    a, b = got64["logps"], got32["logps"].double()
    ok = torch.isfinite(a) & torch.isfinite(b) & got64["executed"][:, :, None]
    assert torch.equal(torch.isfinite(a), torch.isfinite(b))
    return float((a - b)[ok].abs().max())


def tolerance(env_name: str, dev32: float) -> float:
    """The bound of a kernel log-prob against ``step_f64``: the records' own STEP_TOL (the six: ``FLOOR``), or 4 x the fp32
    restatement's deviation on the same inputs (the margin the project grants a different summation order)."""
    return max(REFS[env_name].STEP_TOL if env_name in REFS else FLOOR, 4 * dev32)


def step_state(env_name: str, st: dict, action) -> None:
    """One transition of the state in place; a done row is no longer stepped (a rollout kernel stops a row at its ``done``)."""
    if env_name in REFS:
        REFS[env_name].step_state(st, action, freeze_done=True)
        return
    from oracle import c_oracle
    from rl4co_amd.envspec import spec
    from tests.helpers import apply_step

    done = st["done"].view(-1).bool().clone()
    keep = {k: st[k][done].clone() for k in spec(env_name).keys("traj")}
    apply_step(c_oracle, env_name, torch.where(done, 0, action.cpu()).contiguous(), st)
    for k, v in keep.items():
        st[k][done] = v


# ---- the cases the CPU and GPU tests share (CPU tensors; the GPU tests move them) -------------------------------------------
def random_cache(env_name: str, b: int, n: int, dtype, seed: int = 0, scale: float = 0.5):
    """The random caches of tests/test_gpu_sdvrp.py / test_gpu_mtsp.py (``_random_cache``: planes and the batch-shared table
    scaled 0.5), on the CPU. ``scale``: the six's planes (the multistart variant's test takes smaller ones)."""
    from rl4co_amd.cache import FoldedCache

    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    if env_name in SIX:
        # Random planes and every vector the environment's record uses — not an untrained policy's encoder output, whose
        # near-uniform logits never reach the tanh clip. Drawn in one order whatever the environment.
        from oracle import reference_torch as R
        from rl4co_amd.envspec import spec

        sp = spec(env_name)
        kvl, ctx_first, ctx_cur, q_bias = (r(3, b, n, 128) * scale).to(dtype), r(b, n, 128), r(b, n, 128), r(b, 128)
        q_step0, w_cap, w_time = r(128), r(128), r(128)
        clock = sp.scalar is not None and sp.scalar.clock is not None
        # the clock runs to the generator's max_time (480, unnormalised): its vector is scaled by 1 / max_time so that its term
        # has the order of the other terms of the query and the glimpse softmax does not saturate
        w_time = w_time / R.get_env(env_name, n - 1).max_time if clock else None
        return FoldedCache(env_name, kvl, ctx_first if sp.ctx_first else None, ctx_cur, q_bias,
                           q_step0 if sp.ctx_first else None, w_cap if sp.scalar is not None else None, w_time)
    if env_name == "sdvrp":
        return FoldedCache("sdvrp", (r(3, b, n, 128) * 0.5).to(dtype), None, r(b, n, 128), r(b, 128), None, r(128), None,
                           r(3, 128) * 0.5)
    return FoldedCache("mtsp", (r(3, b, n, 128) * 0.5).to(dtype), None, r(b, n, 128), r(b, 128), None, None, None, None,
                       r(4, 128) * 0.5)


def sdvrp_instances(n: int, b: int, seed: int | None = None):
    """Demands as ``_forced_case`` of tests/test_gpu_sdvrp.py: integers 1..9 over 15 units per vehicle."""
    g = torch.Generator().manual_seed(n if seed is None else seed)
    return torch.randint(1, 10, (b, n - 1), generator=g).float() / 15.0


def mtsp_instances(n: int, b: int, num_agents: int | None = None, seed: int | None = None):
    """Coordinates and agents as ``_forced_case`` of tests/test_gpu_mtsp.py: one agent, few, and more than customers, in
    turn over the rows — or ``num_agents`` for every row."""
    g = torch.Generator().manual_seed(n if seed is None else seed)
    locs = torch.rand(b, n, 2, generator=g)
    agents = torch.tensor([1, 2, 5, n + 3] * ((b + 3) // 4))[:b] if num_agents is None else torch.full((b,), num_agents)
    return locs, agents


def initial_state(env_name: str, inst) -> dict:
    if env_name in SIX:  # (``forced_case`` hands the six's reset state out as their instance)
        return {k: v.clone() for k, v in inst.items()}
    return sdvrp_ref.initial_state(inst) if env_name == "sdvrp" else mtsp_ref.initial_state(*inst)


def six_instances(env_name: str, n: int, b: int, seed: int | None = None):
    """(the restated reference environment, its reset state) of ``b`` generated instances of ``n`` nodes, the depot included
    where the environment has one (``tests.helpers.make_instances``: its generators take any size)."""
    from tests.helpers import DATA_SEED, make_instances

    env, data = make_instances(env_name, n - (env_name != "tsp"), b, seed=DATA_SEED + n if seed is None else seed)
    return env, env.reset(data)


def six_state(env_name: str, n: int, b: int, seed: int | None = None, num_starts: int = 0) -> dict:
    """The flat reset state (``tests.helpers.rollout_state``) of ``six_instances``."""
    from tests.helpers import rollout_state

    st = rollout_state(env_name, six_instances(env_name, n, b, seed)[1], num_starts=num_starts)
    assert st["action_mask"].shape[1] == n, (env_name, n, tuple(st["action_mask"].shape))
    return st


def row_steps(executed) -> torch.Tensor:
    """A row's own length from ``executed`` [B, T]: the steps taken before its ``done``."""
    return executed.sum(1)


def _six_walk(env_name: str, st0: dict, seed: int):
    """A random feasible walk of the six until every row is done. Even rows prefer customers and take the depot only when
    nothing else is feasible (an OP or PCTSP row may go home early: uniform walks end those rows after a few steps); odd
    rows pick uniformly over the mask. (actions [B, T], executed [B, T])."""
    from tests.helpers import max_horizon

    st = {k: v.clone() for k, v in st0.items()}
    b, n = st["action_mask"].shape
    g = torch.Generator().manual_seed(seed)
    even = torch.arange(b) % 2 == 0
    acts, executed = [], []
    for _ in range(max_horizon(env_name, n)):
        done = st["done"].view(-1).bool().clone()
        if bool(done.all()):
            break
        wgt = st["action_mask"].bool().float()
        assert bool((wgt.sum(1) > 0)[~done].all())
        customers = wgt[:, 1:].sum(1) > 0
        wgt[even & customers, 0] = 0
        wgt[done] = 0
        wgt[done, 0] = 1  # (the padding action)
        a = torch.multinomial(wgt, 1, generator=g)[:, 0]
        acts.append(a), executed.append(~done)
        step_state(env_name, st, a)
    assert bool(st["done"].all()), f"{env_name}: the walk did not finish inside the horizon"
    return torch.stack(acts, 1), torch.stack(executed, 1)


def forced_case(env_name: str, n: int, b: int, num_agents: int | None = None, seed: int | None = None):
    """(instances, forced actions [B, steps]): a random feasible walk until every row is done, cut two padding steps behind
    the longest row's own length (as ``_forced_case`` does). The six: the instance is the flat reset state, and the walk
    with its padding stays within ``tests.helpers.max_horizon`` (a TSP, PDP or full PCTSP row leaves no room for padding)."""
    if env_name in SIX:
        from tests.helpers import max_horizon

        st0 = six_state(env_name, n, b, seed)
        acts, executed = _six_walk(env_name, st0, seed=WALK_SEEDS.get((env_name, n), n + 1) if seed is None else seed)
        steps = min(int(row_steps(executed).max()) + 2, max_horizon(env_name, n))
        out = torch.zeros(b, steps, dtype=torch.int64)
        out[:, : acts.shape[1]] = acts
        return st0, out.contiguous()
    if env_name == "sdvrp":
        inst = sdvrp_instances(n, b)
        acts, final = sdvrp_ref.random_walk(inst, 6 * n, seed=n + 1)
    else:
        inst = mtsp_instances(n, b, num_agents)
        acts, final = mtsp_ref.random_walk(*inst, 2 * n, seed=n + 1)
    assert bool(final["done"].all())
    steps = int(mtsp_ref.row_lengths(acts).max()) + 2  # (the action that finishes a row is a customer in both environments)
    return inst, acts[:, :steps].contiguous()


def c_decode(cache, st0: dict, mode: str, steps: int, row_groups, t0: int = 0, first=None, want_all: bool = False, **kw) -> dict:
    """``steps`` decode steps of the C specified-order oracle from ``st0`` (cloned) on ``cache`` (CPU): ``actions`` and
    ``logps`` [B, t0 + steps], ``n_steps`` [B], ``err``, the final ``state`` and, ``want_all``, ``all_logps`` [B, ., N].
    ``first`` [B]: the multistart nodes, applied as step 0 (``t0`` = 1)."""
    from oracle import c_oracle
    from tests.helpers import apply_step

    st = {k: v.clone() for k, v in st0.items()}
    b, n = st["action_mask"].shape
    out = {"actions": torch.zeros(b, t0 + steps, dtype=torch.int64), "logps": torch.zeros(b, t0 + steps),
           "n_steps": torch.zeros(b, dtype=torch.int32), "state": st}
    err = torch.zeros(1, dtype=torch.int32)
    if first is not None:
        out["actions"][:, 0] = first
        apply_step(c_oracle, cache.env_name, first.contiguous(), st)
    if want_all:
        out["all_logps"] = torch.zeros(b, t0 + steps, n)
    c_oracle.am_decode(cache, st, mode=mode, max_steps=steps, t0=t0, actions=out["actions"], logps=out["logps"], err=err,
                       n_steps=out["n_steps"], row_groups=row_groups, all_logps=out.get("all_logps"), **kw)
    out["err"] = int(err.item())
    return out


def walk_facts(env_name: str, st0: dict, acts) -> dict:
    """What a forced walk of the six exercises, from the restatement's state alone (the GPU cases assert these on the CPU
    side): ``max_node`` the largest node chosen at an executed step; ``depot_returns`` [B] the executed depot visits of a
    row; ``time_window_masked`` (CVRPTW) some unvisited customer whose demand fits is masked at an executed step;
    ``length_cut`` (OP) some row goes home from a customer-less mask with customers unvisited and the depot not visited
    before; ``home_early`` / ``home_full`` (OP, PCTSP) some row finishes with / without unvisited customers."""
    st = {k: v.clone() for k, v in st0.items()}
    b, n = st["action_mask"].shape
    facts = {"max_node": 0, "depot_returns": torch.zeros(b, dtype=torch.int64), "time_window_masked": False,
             "length_cut": False, "home_early": False, "home_full": False}
    for t in range(acts.shape[1]):
        ex = ~st["done"].view(-1).bool().clone()
        if not bool(ex.any()):
            break
        a = acts[:, t]
        mask = st["action_mask"].bool().clone()
        facts["max_node"] = max(facts["max_node"], int(a[ex].max()))
        facts["depot_returns"] += (ex & (a == 0)).long()
        if env_name == "cvrptw":
            inst = torch.arange(b) % st["demand"].shape[0]
            fits = st["demand"][inst] + st["used_capacity"].view(-1, 1) <= st["vehicle_capacity"].view(-1, 1)
            open_ = ~st["visited"][:, 1:].bool() & fits
            facts["time_window_masked"] |= bool((open_ & ~mask[:, 1:] & ex[:, None]).any())
        if env_name in ("op", "pctsp"):
            unvisited = ~st["visited"][:, 1:].bool()
            home = ex & (a == 0) & (st["i"].view(-1) > 0)
            facts["home_early"] |= bool((home & unvisited.any(1)).any())
            facts["home_full"] |= bool((home & ~unvisited.any(1)).any())
            if env_name == "op":
                cut = home & unvisited.any(1) & ~mask[:, 1:].any(1) & ~st["visited"][:, 0].bool()
                facts["length_cut"] |= bool(cut.any())
        step_state(env_name, st, a)
    return facts


if __name__ == "__main__":  # python -m tests.decode_f64_ref: the table MEASURED_DEV32 is taken from
    worst = (0.0, None)
    for case in edge_cases():
        st0_, acts_ = forced_case(*case)
        for dtype_ in (torch.float32, torch.bfloat16, torch.float16):
            cache_ = random_cache(case[0], case[2], case[1], dtype_)
            dev_ = fp32_cost(rollout(cache_, st0_, acts_), rollout(cache_, st0_, acts_, step=step_f32))
            worst = max(worst, (dev_, (case, dtype_)))
            print(f"{case[0]}-n{case[1]}-b{case[2]} {dtype_}: dev32 {dev_:.4e} over {acts_.shape[1]} steps", flush=True)
    print(f"largest dev32 {worst[0]:.4e} at {worst[1]}: FLOOR = {4 * worst[0]:.4e}")
