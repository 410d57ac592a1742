"""Multi-agent TSP (min-max): a torch-fp32 restatement of the reference's transition (envs/routing/mtsp/env.py:63-131) and of
its decoder step with the four-scalar context (env_embeddings/context.py:246-280), the closed form of the reference's padding
quirk, and the recorder of the reference's own rollouts (tests/golden/reference/mtsp_*.npz). The restatement is pinned to the
recorded reference states by tests/test_mtsp_cpu.py; the GPU tests compare the kernels with the restatement and the records."""
import math

import torch

# case -> (num_loc incl. the depot, batch, decode type, min_num_agents, max_num_agents, data seed)
CASES = {"mtsp20_greedy": (20, 64, "greedy", 1, 6, 1234), "mtsp50_greedy": (50, 64, "greedy", 2, 8, 1234),
         "mtsp20_sampling": (20, 64, "sampling", 1, 6, 1234), "mtsp50_sampling": (50, 64, "sampling", 2, 8, 1234)}
# Per-step tolerance of a kernel log-prob against the recorded reference (fp32 both sides, different operation order: folded
# cache and context, specified-order reductions): 4 x the largest deviation measured on the MI355X over the four records
# (MEASURED_STEP_DEV). The headroom covers fold GEMMs whose summation order differs between library versions;
# it has to stay at or below the 2e-5 the top-k record test grants this class of comparison.
MEASURED_STEP_DEV = 1.431e-6  # mTSP-50, greedy and sampling; mTSP-20: 1.192e-6 greedy, 9.54e-7 sampling
STEP_TOL = 4 * MEASURED_STEP_DEV
STATE_ROWS = 24  # instances whose per-step lengths a greedy record keeps (masks, agents, nodes, done: all rows)
RESET_DTYPES = [torch.bool, torch.int64, torch.float32]
STATE_KEYS = ("agent_idx", "current_length", "max_subtour_length", "current_node", "action_mask", "done")


def dist(x, y):
    """get_distance (utils/ops.py): the fp32 2-norm of a size-2 dim — sqrt(fma(dy, dy, dx * dx)) in torch's CPU kernel."""
    return (x - y).norm(p=2, dim=-1)


# ---- the transition, op for op in IEEE fp32 -----------------------------------------------------------------------------
def step(action, locs, num_agents, agent_idx, current_length, max_subtour_length, current_node, action_mask, done, err=None):
    """In-place stand-in of ``kernels.mtsp_step`` on CPU tensors (the test plays the device). mtsp/env.py:63-131."""
    b = action_mask.shape[0]
    rows = torch.arange(b)
    a = action.view(-1)
    cur_loc, prev_loc, depot = locs[rows, a], locs[rows, current_node.view(-1)], locs[:, 0]
    avail = action_mask.bool().clone()
    avail[rows, a] = False
    avail[:, 0] = (a != 0) & (agent_idx < num_agents - 1)
    fin = avail[:, 1:].sum(-1) == 0
    avail[:, 0] = fin | avail[:, 0]
    length = current_length + dist(cur_loc, prev_loc)
    length = torch.where(fin, length + dist(cur_loc, depot), length)
    max_subtour_length.copy_(torch.where(length > max_subtour_length, length, max_subtour_length))
    new_agent = agent_idx + (a == 0).long()
    current_length.copy_(length * (new_agent == agent_idx).float())
    agent_idx.copy_(new_agent)
    current_node.view(-1).copy_(a)
    action_mask.copy_(avail.to(action_mask.dtype))
    done.view(-1).copy_(fin.to(done.dtype))


def initial_state(locs, num_agents):
    """The flat state of ``envspec`` for fresh instances."""
    b, n = locs.shape[:2]
    mask = torch.ones(b, n, dtype=torch.bool)
    mask[:, 0] = False
    return {"locs": locs.contiguous(), "num_agents": num_agents.to(torch.int64).contiguous(),
            "agent_idx": torch.zeros(b, dtype=torch.int64), "current_length": torch.zeros(b),
            "max_subtour_length": torch.zeros(b), "current_node": torch.zeros(b, dtype=torch.int64), "action_mask": mask,
            "done": torch.zeros(b, dtype=torch.bool)}


def step_state(st: dict, action, freeze_done: bool = False) -> None:
    """``freeze_done``: a finished trajectory keeps its state, as in a rollout kernel (its loop ends at ``done``)."""
    before = {k: st[k].clone() for k in STATE_KEYS} if freeze_done else None
    step(action, st["locs"], st["num_agents"], st["agent_idx"], st["current_length"], st["max_subtour_length"],
         st["current_node"], st["action_mask"], st["done"])
    if freeze_done:
        rows = before["done"].view(-1).bool()
        for k in STATE_KEYS:
            st[k][rows] = before[k][rows]


def random_walk(locs, num_agents, steps: int, seed: int = 0):
    """Forced action sequences [B, steps] (a uniformly drawn feasible node per step, the depot once done) and the state of
    a rollout kernel after them (every row frozen at its ``done``)."""
    g = torch.Generator().manual_seed(seed)
    st = initial_state(locs, num_agents)
    acts = torch.zeros(locs.shape[0], steps, dtype=torch.int64)
    for t in range(steps):
        a = torch.multinomial(st["action_mask"].float(), 1, generator=g)[:, 0]
        a = torch.where(st["done"], torch.zeros_like(a), a)
        acts[:, t] = a
        step_state(st, a, freeze_done=True)
    return acts, st


def row_lengths(actions):
    """A row's own length: 1 + the index of its last non-zero action (the action that finishes a row is a customer)."""
    t = actions.shape[1]
    return t - (actions != 0).flip(1).to(torch.int8).argmax(1)


def padded_reward(locs, actions, max_at_done, length_at_done):
    """The reference keeps stepping finished rows with action 0 until the batch is done; the first such step adds the
    return leg a second time before ``max_subtour_length`` is taken (mtsp/env.py:97-112). Closed form of the reward the
    reference reports, from a row's state AT its done: rows finished before the batch's last step get
    max(max, length_at_done + dist(depot, last customer))."""
    b, t = actions.shape
    n_own = row_lengths(actions)
    last = actions[torch.arange(b), n_own - 1]
    leg = dist(locs[:, 0], locs[torch.arange(b), last])
    again = length_at_done + leg
    padded = torch.where(again > max_at_done, again, max_at_done)
    return -torch.where(n_own < t, padded, max_at_done)


# ---- the reference decoder along given actions (autograd) -----------------------------------------------------------------
def features(st):
    """context.py:265-280: (num_agents - agent_idx, current_length, max_subtour_length, |loc_cur - loc_0|), [B, 4]."""
    b = st["locs"].shape[0]
    here = st["locs"][torch.arange(b, device=st["locs"].device), st["current_node"].view(-1)]
    return torch.stack(((st["num_agents"] - st["agent_idx"]).float(), st["current_length"], st["max_subtour_length"],
                        torch.norm(here - st["locs"][:, 0], dim=-1)), -1)


def _step_any_device(st, a):
    """``step`` without in-place aliasing problems under autograd, on the state's device."""
    new = {k: v.clone() for k, v in st.items()}
    dev = st["locs"].device
    cpu = {k: v.cpu() for k, v in new.items()}
    step(a.cpu(), cpu["locs"], cpu["num_agents"], cpu["agent_idx"], cpu["current_length"], cpu["max_subtour_length"],
         cpu["current_node"], cpu["action_mask"], cpu["done"])
    return {k: v.to(dev) for k, v in cpu.items()}


def decoder_step_logps(dec, hidden, st0: dict, actions, tanh_clipping=10.0, temperature=1.0, all_logps=False):
    """Per-step log-probs [B, T] of ``actions`` under the reference's AttentionModelDecoder algebra with MTSPContext, step by
    step as the reference's loop evaluates them (finished rows are stepped with the padding action, log-prob 0). ``dec``: a
    decoder with the reference's attribute names (``project_node_embeddings``, ``project_fixed_context``,
    ``context_embedding.project_context`` / ``.proj_dynamic_feats``, ``pointer.project_out``)."""
    b, n, d = hidden.shape
    nh = 8
    st = {k: v.clone() for k, v in st0.items()}
    k_g, v_g, k_l = dec.project_node_embeddings(hidden).chunk(3, dim=-1)
    graph = dec.project_fixed_context(hidden.mean(1))
    split = lambda x: x.view(b, -1, nh, d // nh).transpose(1, 2)  # noqa: E731
    out, full = [], []
    for t in range(actions.shape[1]):
        cur = st["current_node"].view(-1)
        h_cur = hidden.gather(1, cur[:, None, None].expand(b, 1, d))[:, 0]
        q = dec.context_embedding.project_context(
            torch.cat((h_cur, dec.context_embedding.proj_dynamic_feats(features(st).to(hidden.dtype))), -1)) + graph
        mask = st["action_mask"].bool()
        heads = torch.nn.functional.scaled_dot_product_attention(split(q[:, None]), split(k_g), split(v_g),
                                                                 attn_mask=mask[:, None, None, :])
        glimpse = dec.pointer.project_out(heads.transpose(1, 2).reshape(b, 1, d))
        logits = (torch.bmm(glimpse, k_l.transpose(1, 2)) / math.sqrt(d))[:, 0]
        logits = torch.tanh(logits) * tanh_clipping
        logp = torch.log_softmax(logits.masked_fill(~mask, float("-inf")) / temperature, -1)
        out.append(logp.gather(1, actions[:, t : t + 1])[:, 0])
        full.append(logp)
        st = _step_any_device(st, actions[:, t])
    return (torch.stack(out, 1), torch.stack(full, 1)) if all_logps else torch.stack(out, 1)


def pack_mask(mask):
    """[..., N] bool -> [..., ceil(N / 8)] uint8, bit j % 8 of byte j // 8 = node j (the records keep the masks as bits)."""
    n = mask.shape[-1]
    m = torch.nn.functional.pad(mask.to(torch.int32), (0, (-n) % 8)).view(*mask.shape[:-1], -1, 8)
    return (m << torch.arange(8, dtype=torch.int32)).sum(-1).to(torch.uint8)


def sample_noise(batch: int, n: int, steps: int, seed: int):
    """The Exp(1) draws of the reference's torch.multinomial stream (one [B, N] draw per step after manual_seed)."""
    torch.manual_seed(seed)
    return torch.stack([torch.empty(batch, n).exponential_(1) for _ in range(steps)], 0).contiguous()


# ---- the recorder (needs the reference checkout) ---------------------------------------------------------------------------
def reference_rollout(case: str) -> dict:
    """The reference's own AttentionModelPolicy("mtsp") and MTSPEnv on CPU in fp32, seeded as oracle/gen_golden.py. Everything
    is recorded AFTER the batch's padding (the reference's loop runs until every row is done)."""
    import importlib

    from oracle import ref_import
    from tests.helpers import SAMPLE_SEED, WEIGHT_SEED

    ref = ref_import.load()
    num_loc, batch, decode_type, lo, hi, data_seed = CASES[case]
    env_cls = importlib.import_module("rl4co.envs.routing.mtsp.env").MTSPEnv
    base = importlib.import_module("rl4co.models.common.constructive.base")
    ref_env = env_cls(generator_params=dict(num_loc=num_loc, min_num_agents=lo, max_num_agents=hi), seed=0)
    torch.manual_seed(WEIGHT_SEED)
    pol = ref.AttentionModelPolicy(env_name="mtsp").eval()
    torch.manual_seed(data_seed)
    data = ref_env.generator(batch_size=[batch])
    td0 = ref_env.reset(data.clone())
    seen = {}
    orig_ll = base.get_log_likelihood

    def grab_ll(logprobs, actions, mask, return_sum):
        seen["logprobs"] = logprobs
        return orig_ll(logprobs, actions, mask, return_sum)

    base.get_log_likelihood = grab_ll
    try:
        torch.manual_seed(SAMPLE_SEED)
        with torch.inference_mode():
            out = pol(td0.clone(), ref_env, phase="test", decode_type=decode_type, return_sum_log_likelihood=False,
                      store_all_logp=True)
    finally:
        base.get_log_likelihood = orig_ll
    rec = {"actions": out["actions"], "log_likelihood": out["log_likelihood"], "reward": out["reward"]}
    rec.update({f"in_{k}": v for k, v in data.items()})
    if decode_type == "greedy":
        lp = seen["logprobs"]  # [B, T, N]
        top2 = lp.topk(2, dim=-1)[0]
        rec["min_gap"] = (top2[..., 0] - top2[..., 1]).min(1)[0]  # inf where one node is feasible
        # the states the reference's environment went through, before each step and after the last
        td = ref_env.reset(data.clone())
        rec.update({f"reset_{k}": (v.to(torch.uint8) if v.dtype == torch.bool else v) for k, v in td.items()
                    if k not in ("locs", "num_agents")})
        # (npz keeps no bool / key list: the dtypes of the reset keys, sorted by name, as codes — RESET_DTYPES)
        rec["reset_dtype_codes"] = torch.tensor([RESET_DTYPES.index(td[k].dtype) for k in sorted(td.keys())])
        keys = ("agent_idx", "current_length", "max_subtour_length", "current_node", "done")
        tab = {k: [] for k in keys + ("action_mask",)}
        for t in range(out["actions"].shape[1] + 1):
            for k in keys:
                tab[k].append(td[k].reshape(-1).clone())
            tab["action_mask"].append(td["action_mask"].clone())
            if t < out["actions"].shape[1]:
                td.set("action", out["actions"][:, t])
                td = ref_env.step(td)["next"]
        rec["states_mask_bits"] = pack_mask(torch.stack(tab["action_mask"], 1))
        rec["states_done"] = torch.stack(tab["done"], 1).to(torch.uint8)
        rec["states_agent"] = torch.stack(tab["agent_idx"], 1).to(torch.uint8)  # (< 2 n)
        rec["states_node"] = torch.stack(tab["current_node"], 1).to(torch.uint8)
        rec["states_length"] = torch.stack(tab["current_length"], 1)[:STATE_ROWS]
        rec["states_max"] = torch.stack(tab["max_subtour_length"], 1)[:STATE_ROWS]
    return rec


def record(case: str) -> dict:
    from tests.helpers import reference_record

    return reference_record(f"mtsp_{case}", lambda: reference_rollout(case))


if __name__ == "__main__":  # RL4CO_RECORD_REFERENCE=1 python -m tests.mtsp_ref
    for name in CASES:
        r = record(name)
        print(name, {k: tuple(v.shape) for k, v in r.items()})
