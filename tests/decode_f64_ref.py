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
its ``done``). Pinned to the reference decoder's algebra and to the reference's records by tests/test_decode_f64_cpu.py."""
import math

import torch

from tests import mtsp_ref, sdvrp_ref

NUM_HEADS = 8
REFS = {"sdvrp": sdvrp_ref, "mtsp": mtsp_ref}


def _step(cache, st: dict, dtype, tanh_clipping: float = 10.0, temperature: float = 1.0, zero_depot: bool = True):
    """One decode step of every row of ``st`` (an ``initial_state``-style dict, any device) on ``cache`` in ``dtype``:
    (log-probs [B, N], processed logits z [B, N] (-inf = infeasible), mask [B, N]). ``zero_depot=False`` is a seeded
    mistake for the mutation test (the depot's stored demand enters the dynamic term)."""
    env = cache.env_name
    dev = cache.kvl.device
    w = lambda t: t.to(device=dev, dtype=dtype)  # noqa: E731  (exact for every stored value when dtype is float64)
    mask = st["action_mask"].to(dev).bool().clone()  # (the caller steps the state in place)
    b, n = mask.shape
    d_model = cache.kvl.shape[-1]
    dh = d_model // NUM_HEADS
    cur = st["current_node"].to(dev).view(-1)
    q = w(cache.ctx_cur)[torch.arange(b, device=dev), cur] + w(cache.q_bias)
    key, val, lkey = w(cache.kvl[0]), w(cache.kvl[1]), w(cache.kvl[2])
    if env == "sdvrp":
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
    ref = REFS[cache.env_name]
    st = {k: v.clone() for k, v in st0.items()}
    actions = actions.cpu()
    lps, zs, masks, executed = [], [], [], []
    for t in range(actions.shape[1]):
        executed.append(~st["done"].view(-1).bool().clone())
        lp, z, mask = step(cache, st, **kw)
        lps.append(lp.cpu()), zs.append(z.cpu()), masks.append(mask.cpu())
        ref.step_state(st, actions[:, t], freeze_done=True)
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
    """The bound of a kernel log-prob against ``step_f64``: the records' own STEP_TOL, or 4 x the fp32 restatement's
    deviation on the same inputs (the margin the project grants a different summation order)."""
    return max(REFS[env_name].STEP_TOL, 4 * dev32)


# ---- the cases the CPU and GPU tests share (CPU tensors; the GPU tests move them) -------------------------------------------
def random_cache(env_name: str, b: int, n: int, dtype, seed: int = 0):
    """The random caches of tests/test_gpu_sdvrp.py / test_gpu_mtsp.py (``_random_cache``: planes and the batch-shared table
    scaled 0.5), on the CPU."""
    from rl4co_amd.cache import FoldedCache

    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
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
    return sdvrp_ref.initial_state(inst) if env_name == "sdvrp" else mtsp_ref.initial_state(*inst)


def forced_case(env_name: str, n: int, b: int, num_agents: int | None = None):
    """(instances, forced actions [B, steps]): a random feasible walk until every row is done, cut two padding steps behind
    the longest row's own length (as ``_forced_case`` does)."""
    if env_name == "sdvrp":
        inst = sdvrp_instances(n, b)
        acts, final = sdvrp_ref.random_walk(inst, 6 * n, seed=n + 1)
    else:
        inst = mtsp_instances(n, b, num_agents)
        acts, final = mtsp_ref.random_walk(*inst, 2 * n, seed=n + 1)
    assert bool(final["done"].all())
    steps = int(mtsp_ref.row_lengths(acts).max()) + 2  # (the action that finishes a row is a customer in both environments)
    return inst, acts[:, :steps].contiguous()
