"""Split-delivery VRP: a torch-fp32 restatement of the reference's transition (envs/routing/sdvrp/env.py:56-123) and
of its decoder with the dynamic embedding (zoo/am/decoder.py:142-152, env_embeddings/dynamic.py:60-78), and the recorder of
the reference's own rollouts (tests/golden/reference/sdvrp_*.npz). The restatement is pinned to the recorded reference
states by tests/test_sdvrp_cpu.py; the GPU tests compare the kernels with the restatement and the records."""
import math

import torch

CASES = {"sdvrp20_greedy": (20, 64, "greedy"), "sdvrp50_greedy": (50, 64, "greedy"),
         "sdvrp20_sampling": (20, 64, "sampling"), "sdvrp50_sampling": (50, 64, "sampling")}
STATE_ROWS = 16  # instances whose per-step remaining demands a greedy record keeps
# Per-step tolerance of a kernel log-prob against the recorded reference (fp32 both sides, different operation order: folded
# cache, specified-order reductions): 4 x the largest deviation measured on the MI355X over the four records, 1.192e-6 (at
# SDVRP-50 greedy; 7.7e-7 - 9.5e-7 on the others) — DESIGN §4.9. The headroom covers fold GEMMs whose summation order
# differs between library versions; far below the 2e-5 the top-k record test grants this class of comparison.
STEP_TOL = 4 * 1.192e-6


# ---- the transition, op for op in IEEE fp32 -----------------------------------------------------------------------------
def mask_of(demand_with_depot, used_capacity, vehicle_capacity, current_node):
    """sdvrp/env.py:117-123; [B, N], [B], [B], [B] -> [B, N] bool."""
    mask_loc = (demand_with_depot[:, 1:] == 0) | (used_capacity >= vehicle_capacity)[:, None]
    mask_depot = (current_node == 0) & ((mask_loc == 0).int().sum(-1) > 0)
    return ~torch.cat((mask_depot[:, None], mask_loc), -1)


def step(action, demand_with_depot, used_capacity, vehicle_capacity, current_node, action_mask, done, err=None):
    """In-place stand-in of ``kernels.sdvrp_step`` on CPU tensors (the test plays the device); action=None: mask only."""
    used, cap = used_capacity.view(-1), vehicle_capacity.view(-1)
    cur = current_node.view(-1)
    if action is not None:
        a = action.view(-1, 1)
        selected = demand_with_depot.gather(1, a)[:, 0]
        delivered = torch.min(selected, cap - used)
        used.copy_((used + delivered) * (a[:, 0] != 0).float())
        demand_with_depot.scatter_add_(1, a, -delivered[:, None])
        done.view(-1).copy_(~(demand_with_depot > 0).any(-1))
        cur.copy_(a[:, 0])
    action_mask.copy_(mask_of(demand_with_depot, used, cap, cur))


def initial_state(demand, capacity: float = 1.0):
    """The flat state of ``envspec`` for fresh instances: demand [B, N - 1] -> dict of [B, ...] tensors."""
    b = demand.shape[0]
    st = {"demand_with_depot": torch.cat((torch.zeros(b, 1), demand), 1).contiguous(),
          "used_capacity": torch.zeros(b), "vehicle_capacity": torch.full((b,), capacity),
          "current_node": torch.zeros(b, dtype=torch.int64), "done": torch.zeros(b, dtype=torch.bool)}
    st["action_mask"] = mask_of(st["demand_with_depot"], st["used_capacity"], st["vehicle_capacity"], st["current_node"])
    return st


def step_state(st: dict, action, freeze_done: bool = False) -> None:
    """``freeze_done``: a finished trajectory keeps its state, as in a rollout kernel (its loop ends at ``done``)."""
    before = {k: v.clone() for k, v in st.items()} if freeze_done else None
    step(action, st["demand_with_depot"], st["used_capacity"], st["vehicle_capacity"], st["current_node"], st["action_mask"],
         st["done"])
    if freeze_done:
        rows = before["done"].view(-1).bool()
        for k, v in st.items():
            v[rows] = before[k][rows]


def random_walk(demand, steps: int, seed: int = 0, capacity: float = 1.0):
    """Forced action sequences [B, steps] (a uniformly drawn feasible node per step, the depot once done) and the state
    after them."""
    g = torch.Generator().manual_seed(seed)
    st = initial_state(demand, capacity)
    acts = torch.zeros(demand.shape[0], steps, dtype=torch.int64)
    for t in range(steps):
        w = st["action_mask"].float()
        a = torch.multinomial(w, 1, generator=g)[:, 0]
        a = torch.where(st["done"], torch.zeros_like(a), a)
        acts[:, t] = a
        step_state(st, a)
    return acts, st


# ---- the reference decoder along given actions (autograd) -----------------------------------------------------------------
def decoder_step_logps(dec, hidden, st0: dict, actions, tanh_clipping=10.0, temperature=1.0, all_logps=False):
    """Per-step log-probs [B, T] of ``actions`` under the reference's AttentionModelDecoder algebra with the SDVRP dynamic
    embedding, step by step as the reference's loop evaluates them. ``dec``: a decoder with the reference's attribute names
    (``project_node_embeddings``, ``project_fixed_context``, ``context_embedding.project_context``,
    ``dynamic_embedding.projection``, ``pointer.project_out``); ``st0``: ``initial_state``-style dict (cloned)."""
    b, n, d = hidden.shape
    nh = 8
    st = {k: v.clone() for k, v in st0.items()}
    k_g, v_g, k_l = dec.project_node_embeddings(hidden).chunk(3, dim=-1)
    graph = dec.project_fixed_context(hidden.mean(1))
    out, full = [], []
    for t in range(actions.shape[1]):
        cur = st["current_node"].view(-1).clone()  # (the state is stepped in place below: autograd keeps these)
        h_cur = hidden.gather(1, cur[:, None, None].expand(b, 1, d))[:, 0]
        rem = (st["vehicle_capacity"].view(-1) - st["used_capacity"].view(-1))[:, None]
        q = dec.context_embedding.project_context(torch.cat((h_cur, rem.to(hidden.dtype)), -1)) + graph
        dem = st["demand_with_depot"].to(hidden.dtype, copy=True)  # (the decoder may be evaluated in float64)
        dem[:, 0] = 0
        dk, dv, dl = dec.dynamic_embedding.projection(dem[..., None]).chunk(3, dim=-1)
        mask = st["action_mask"].bool().clone()
        split = lambda x: x.view(b, -1, nh, d // nh).transpose(1, 2)  # noqa: E731
        heads = torch.nn.functional.scaled_dot_product_attention(split(q[:, None]), split(k_g + dk), split(v_g + dv),
                                                                 attn_mask=mask[:, None, None, :])
        glimpse = dec.pointer.project_out(heads.transpose(1, 2).reshape(b, 1, d))
        logits = (torch.bmm(glimpse, (k_l + dl).transpose(1, 2)) / math.sqrt(d))[:, 0]
        logits = torch.tanh(logits) * tanh_clipping
        logp = torch.log_softmax(logits.masked_fill(~mask, float("-inf")) / temperature, -1)
        out.append(logp.gather(1, actions[:, t : t + 1])[:, 0])
        full.append(logp)
        step_state(st, actions[:, t])
    return (torch.stack(out, 1), torch.stack(full, 1)) if all_logps else torch.stack(out, 1)


def sample_noise(batch: int, n: int, steps: int, seed: int):
    """The Exp(1) draws of the reference's torch.multinomial stream (one [B, N] draw per step after manual_seed)."""
    torch.manual_seed(seed)
    return torch.stack([torch.empty(batch, n).exponential_(1) for _ in range(steps)], 0).contiguous()


# ---- the recorder (needs the reference checkout) ---------------------------------------------------------------------------
def reference_rollout(case: str) -> dict:
    """The reference's own AttentionModelPolicy("sdvrp") and SDVRPEnv on CPU in fp32, seeded as oracle/gen_golden.py."""
    import importlib

    from oracle import ref_import
    from tests.helpers import DATA_SEED, SAMPLE_SEED, WEIGHT_SEED

    ref = ref_import.load()
    num_loc, batch, decode_type = CASES[case]
    env_cls = importlib.import_module("rl4co.envs.routing.sdvrp.env").SDVRPEnv
    base = importlib.import_module("rl4co.models.common.constructive.base")
    ref_env = env_cls(generator_params=dict(num_loc=num_loc), seed=0)
    torch.manual_seed(WEIGHT_SEED)
    pol = ref.AttentionModelPolicy(env_name="sdvrp").eval()
    torch.manual_seed(DATA_SEED)
    data = ref_env.generator(batch_size=[batch])
    td0 = ref_env.reset(data.clone())
    seen = {}
    orig_ll, orig_reward = base.get_log_likelihood, ref_env.get_reward

    def grab_ll(logprobs, actions, mask, return_sum):
        seen["logprobs"] = logprobs
        return orig_ll(logprobs, actions, mask, return_sum)

    def grab_reward(td, actions):
        seen["td"] = td
        return orig_reward(td, actions)

    base.get_log_likelihood, ref_env.get_reward = grab_ll, grab_reward
    try:
        torch.manual_seed(SAMPLE_SEED)
        with torch.inference_mode():
            out = pol(td0.clone(), ref_env, phase="test", decode_type=decode_type, return_sum_log_likelihood=False,
                      store_all_logp=True)
    finally:
        base.get_log_likelihood = orig_ll
    rec = {"actions": out["actions"], "log_likelihood": out["log_likelihood"], "reward": out["reward"],
           "demand_with_depot": seen["td"]["demand_with_depot"], "used_capacity": seen["td"]["used_capacity"].reshape(-1)}
    rec.update({f"in_{k}": v for k, v in data.items()})
    if decode_type == "greedy":
        lp = seen["logprobs"]  # [B, T, N]
        top2 = lp.topk(2, dim=-1)[0]
        gap = top2[..., 0] - top2[..., 1]  # inf where one node is feasible
        rec["min_gap"] = gap.min(1)[0]
        # the states the reference's environment went through, before each step (all rows: mask bits, used capacity, done;
        # the first STATE_ROWS rows: the remaining demands)
        td = ref_env.reset(data.clone())
        masks, used, done, dem = [], [], [], []
        for t in range(out["actions"].shape[1]):
            masks.append(td["action_mask"].clone()), used.append(td["used_capacity"].reshape(-1).clone())
            done.append(td["done"].reshape(-1).clone()), dem.append(td["demand_with_depot"][:STATE_ROWS].clone())
            td.set("action", out["actions"][:, t])
            td = ref_env.step(td)["next"]
        masks.append(td["action_mask"].clone()), used.append(td["used_capacity"].reshape(-1).clone())
        done.append(td["done"].reshape(-1).clone()), dem.append(td["demand_with_depot"][:STATE_ROWS].clone())
        rec["states_mask"] = torch.stack(masks, 1).to(torch.uint8)
        rec["states_used"] = torch.stack(used, 1)
        rec["states_done"] = torch.stack(done, 1).to(torch.uint8)
        rec["states_demand"] = torch.stack(dem, 1)
    return rec


def record(case: str) -> dict:
    from tests.helpers import reference_record

    return reference_record(f"sdvrp_{case}", lambda: reference_rollout(case))


if __name__ == "__main__":  # RL4CO_RECORD_REFERENCE=1 python -m tests.sdvrp_ref
    for name in CASES:
        r = record(name)
        print(name, {k: tuple(v.shape) for k, v in r.items()})
