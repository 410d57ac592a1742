"""Shared builders for the parity tests: golden fixtures, seeded instances, oracle policies, state."""
from __future__ import annotations

import hashlib
import json
from pathlib import Path

import numpy as np
import torch

from oracle import reference_torch as R

ROOT = Path(__file__).resolve().parents[1]
GOLDEN_DIR = ROOT / "tests" / "golden"
WEIGHT_SEED = 0
DATA_SEED = 1234
SAMPLE_SEED = 4321


def manifest() -> dict:
    return {c["name"]: c for c in json.loads((GOLDEN_DIR / "MANIFEST.json").read_text())["cases"]}


def state_hash(sd: dict) -> str:
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def make_policy(env_name: str, pomo: bool = False, seed: int = WEIGHT_SEED, **kw):
    torch.manual_seed(seed)
    pol = R.pomo_policy(env_name, **kw) if pomo else R.AttentionModelPolicy(env_name, **kw)
    return pol.eval()


def make_instances(env_name: str, num_loc: int, batch: int, seed: int = DATA_SEED, check_solution=True):
    env = R.get_env(env_name, num_loc, check_solution=check_solution)
    torch.manual_seed(seed)
    data = env.generate(batch)
    return env, data


class GoldenCase:
    """One fixture of tests/golden: the REAL reference's outputs (oracle/gen_golden.py) plus the
    seeded policy/inputs rebuilt through the restatement and verified against the stored hashes."""

    def __init__(self, name: str):
        self.meta = manifest()[name]
        z = np.load(GOLDEN_DIR / f"{name}.npz")
        self.actions = torch.from_numpy(z["actions"].astype(np.int64))
        self.reward = torch.from_numpy(z["reward"])
        self.log_likelihood = torch.from_numpy(z["log_likelihood"])
        self.entropy = torch.from_numpy(z["entropy"]) if "entropy" in z.files else None
        m = self.meta
        from rl4co_amd.cache import canonical_env

        # env_label: the reference's environment name; env_name: the environment whose kernels serve it
        self.env_label, self.num_loc, self.batch = m["env"], m["num_loc"], m["batch"]
        self.env_name = canonical_env(self.env_label)
        self.env = R.get_env(self.env_label, self.num_loc)
        torch.manual_seed(m["data_seed"])
        self.data = self.env.generate(self.batch)
        stored = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in_")}
        for k, v in stored.items():
            assert torch.equal(v, self.data[k]), f"seeded {k} differs from the stored fixture input"
        assert state_hash(self.data) == m["inputs_sha256"], "seeded inputs differ from the golden run"
        torch.manual_seed(m["weight_seed"])
        self.policy = R.AttentionModelPolicy(env_name=self.env_label, **m["policy_kwargs"]).eval()
        assert state_hash(self.policy.state_dict()) == m["weights_sha256"], "seeded weights differ from the golden run"

    def reset(self) -> dict:
        return self.env.reset(clone_td(self.data))

    @property
    def rollout_rows(self) -> int:
        """Trajectories the decode loop advances: instances x starts (multistart) or x samples (multisample)."""
        reps = self.num_starts or int(self.meta["forward_kwargs"].get("num_samples", 0) or 0)
        return self.batch * max(reps, 1)

    def start_nodes(self, td0: dict, num_starts: int) -> torch.Tensor:
        """The multistart nodes of the golden run. For OP the reference may RESAMPLE them (ops.py:150-160,
        torch.multinomial on the global generator, the first draw after the run's manual_seed(sample_seed))."""
        torch.manual_seed(self.meta["sample_seed"])
        return self.env.select_start_nodes(td0, num_starts)

    @property
    def num_starts(self) -> int:
        if "multistart" not in self.meta["decode_type"]:
            return 0
        default = self.num_loc // 2 if self.env_name == "pdp" else self.num_loc  # pdp/env.py:225-227: pickups only
        return self.meta["forward_kwargs"].get("num_starts", default)


def decode_level(name: str) -> bool:
    """Fixtures the decode-level tests (kernel / C oracle driven directly) can replay: the policy-only ones exercise
    arguments of ConstructivePolicy.forward (select_best, multisample, temperature ...) through the policy surface."""
    return not manifest()[name].get("policy_only", False)


def clone_td(td: dict) -> dict:
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in td.items()}


def decoder_weights(pol) -> dict:
    dec = pol.decoder
    w = dict(
        w_node=dec.project_node_embeddings.weight.detach(),
        w_out=dec.pointer.project_out.weight.detach(),
        w_ctx=dec.context_embedding.project_context.weight.detach(),
        w_fixed=dec.project_fixed_context.weight.detach() if dec.use_graph_context else None,
        w_placeholder=getattr(dec.context_embedding, "W_placeholder", None),
    )
    # SDVRP's dynamic embedding and mTSP's running scalars' layer, where the decoder has them (cache.fold_constants)
    dyn = getattr(getattr(dec, "dynamic_embedding", None), "projection", None)
    feat = getattr(dec.context_embedding, "proj_dynamic_feats", None)
    if dyn is not None:
        w["w_dyn"] = dyn.weight.detach()
    if feat is not None:
        w["w_feat"] = feat.weight.detach()
    return w


def fold_cache(pol, env_name: str, h: torch.Tensor, dtype=torch.float32, device="cpu", fold=True):
    """fold=False: the reference-association parity cache (raw logit key, per-step context / output GEMVs)."""
    from rl4co_amd.cache import build_folded_cache

    w = {k: (v.detach().to(device) if v is not None else None) for k, v in decoder_weights(pol).items()}
    return build_folded_cache(env_name, h.to(device), cache_dtype=dtype, fold=fold, **w)


def rollout_state(env_name: str, td: dict, device="cpu", num_starts: int = 0) -> dict:
    """Copy an oracle reset state into the flat layout the kernels / C oracle update in place
    (s-major batchify of the trajectory rows when ``num_starts`` > 0; instance data stays [B,...])."""
    s = max(num_starts, 1)

    def rep(x):
        x = x.to(device)
        return x.unsqueeze(0).expand(s, *x.shape).reshape(s * x.shape[0], *x.shape[1:]).contiguous().clone()

    st = {
        "action_mask": rep(td["action_mask"]),
        "current_node": rep(td["current_node"].reshape(-1)),
        "done": rep(td["done"].reshape(-1)),
    }
    if env_name == "tsp":
        st["first_node"] = rep(td["first_node"].reshape(-1))
        st["i"] = rep(td["i"].reshape(-1))
    elif env_name == "pdp":
        st["available"] = rep(td["available"].to(torch.uint8))
        st["to_deliver"] = rep(td["to_deliver"].to(torch.uint8))
        st["i"] = rep(td["i"].reshape(-1))
    elif env_name == "pctsp":
        st["real_prize"] = td["real_prize"].to(device).contiguous()
        st["cur_total_prize"] = rep(td["cur_total_prize"].reshape(-1))
        st["prize_required"] = rep(td["prize_required"].reshape(-1))
        st["i"] = rep(td["i"].reshape(-1))
        st["visited"] = rep(td["visited"].to(torch.uint8))
    elif env_name == "op":
        st["locs"] = td["locs"].to(device).contiguous()
        st["max_length"] = td["max_length"].to(device).contiguous()
        st["tour_length"] = rep(td["tour_length"].reshape(-1))
        st["i"] = rep(td["i"].reshape(-1))
        st["visited"] = rep(td["visited"].to(torch.uint8))
    else:
        st["demand"] = td["demand"].to(device).contiguous()
        st["used_capacity"] = rep(td["used_capacity"].reshape(-1))
        st["vehicle_capacity"] = rep(td["vehicle_capacity"].reshape(-1))
        st["visited"] = rep(td["visited"])
        if env_name == "cvrptw":
            st["locs"] = td["locs"].to(device).contiguous()
            st["time_windows"] = td["time_windows"].to(device).float().contiguous()
            st["durations"] = td["durations"].to(device).float().contiguous()
            st["current_time"] = rep(td["current_time"].reshape(-1))
    return st


device_state = rollout_state  # name used by the GPU tests


def apply_step(mod, env_name: str, action: torch.Tensor, st: dict) -> None:
    """One environment transition on the flat state through `mod` (rl4co_amd.kernels or oracle.c_oracle)."""
    if env_name == "tsp":
        mod.tsp_step(action, st["action_mask"], st["first_node"], st["current_node"], st["i"], st["done"])
    elif env_name == "cvrp":
        mod.cvrp_step(action, st["demand"], st["used_capacity"], st["vehicle_capacity"], st["visited"],
                      st["current_node"], st["action_mask"], st["done"])
    elif env_name == "op":
        mod.op_step(action, st["locs"], st["max_length"], st["tour_length"], st["visited"], st["current_node"], st["i"],
                    st["action_mask"], st["done"])
    elif env_name == "pctsp":
        mod.pctsp_step(action, st["real_prize"], st["cur_total_prize"], st["visited"], st["current_node"], st["i"],
                       st["action_mask"], st["done"])
    elif env_name == "cvrptw":
        mod.cvrptw_step(action, st["demand"], st["locs"], st["time_windows"], st["durations"], st["used_capacity"],
                        st["vehicle_capacity"], st["current_time"], st["visited"], st["current_node"], st["action_mask"],
                        st["done"])
    elif env_name == "pdp":
        mod.pdp_step(action, st["available"], st["to_deliver"], st["current_node"], st["i"], st["action_mask"], st["done"])
    else:
        raise ValueError(env_name)


def max_horizon(env_name: str, n: int) -> int:
    return n if env_name in ("tsp", "pctsp", "pdp") else (n + 2 if env_name == "op" else 2 * n)


def oracle_reward(env_name: str, td0: dict, actions: torch.Tensor) -> torch.Tensor:
    """The environment's reward of `actions` through the C oracle (tour length, or gathered prizes for OP)."""
    from oracle import c_oracle

    if env_name == "op":
        return c_oracle.gather_sum(td0["prize"].contiguous(), actions.contiguous())
    if env_name == "pctsp":  # pctsp/env.py:150-173: three sums in the reference's order
        pen = td0["penalty"].contiguous()
        n = pen.shape[-1]
        every = torch.arange(1, n).expand(actions.shape[0], n - 1).contiguous()
        length = c_oracle.tour_length(td0["locs"], actions.contiguous(), prepend_depot=True, negate=False)
        return c_oracle.gather_sum(pen, actions.contiguous()) - (length + c_oracle.gather_sum(pen, every))
    return c_oracle.tour_length(td0["locs"], actions, prepend_depot=(env_name in ("cvrp", "pdp", "cvrptw")), negate=True)


def kernel_reward(K, env_name: str, td0: dict, actions: torch.Tensor) -> torch.Tensor:
    """Same through the HIP kernels (inputs are moved to the GPU)."""
    if env_name == "op":
        return K.gather_sum(td0["prize"].cuda().contiguous(), actions.cuda().contiguous())
    if env_name == "pctsp":
        pen, acts = td0["penalty"].cuda().contiguous(), actions.cuda().contiguous()
        n = pen.shape[-1]
        every = torch.arange(1, n, device="cuda").expand(acts.shape[0], n - 1).contiguous()
        length = K.tour_length(td0["locs"].cuda(), acts, prepend_depot=True, negate=False)
        return K.gather_sum(pen, acts) - (length + K.gather_sum(pen, every))
    return K.tour_length(td0["locs"].cuda(), actions.cuda().contiguous(), prepend_depot=(env_name in ("cvrp", "pdp", "cvrptw")),
                         negate=True)


def ll_rtol(env_name: str, gpu: bool = False) -> float:
    """Relative tolerance of a rollout's summed log-likelihood against the reference (fp32 both sides, different
    operation order: folded cache, specified-order reductions). 1e-5 for the normalised environments. CVRPTW feeds
    unnormalised coordinates / times (up to 150 / 480) through the same fp32 arithmetic: queries and scores are
    hundreds of times larger, so is their rounding noise (CPU fold, measured 2e-5 on one trajectory of cvrptw100:
    bound 5e-5; cache folded by the GPU's GEMMs, whose summation order differs from oneDNN's, measured 7e-4 on one
    trajectory of cvrptw20: bound 2e-3). Rewards of identical trajectories stay bit-identical everywhere."""
    if env_name == "cvrptw":
        return 2e-3 if gpu else 5e-5
    return 1e-5


def flip_budget(env_name: str, rows: int, gpu: bool = False) -> int:
    """Trajectories that may leave the reference's at an fp32 near-tie: 1 % (2 % against the GPU-side encoder);
    5 % for CVRPTW on the GPU (see ll_rtol: measured 2 of 64)."""
    if env_name == "cvrptw" and gpu:
        return max(1, rows // 20)
    return max(1, rows // (50 if gpu else 100))


REFERENCE_RECORDS = GOLDEN_DIR / "reference"


def reference_record(key: str, compute) -> dict:
    """The reference's side of a comparison, as recorded: ``tests/golden/reference/<key>.npz`` holds the dict of arrays
    ``compute()`` returned when it ran the reference's own code (its checkout, through oracle/ref_import.py). The tests
    compare against the record and need no checkout; ``RL4CO_RECORD_REFERENCE=1`` (checkout present) runs ``compute``
    and rewrites the record — ``python -m oracle.gen_reference_records`` does that for every recorded test."""
    import os

    path = REFERENCE_RECORDS / f"{key}.npz"
    if os.environ.get("RL4CO_RECORD_REFERENCE") == "1":
        arrays = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in compute().items()}
        path.parent.mkdir(parents=True, exist_ok=True)
        np.savez_compressed(path, **arrays)
    with np.load(path) as z:
        return {k: torch.from_numpy(z[k].copy()) for k in z.files}
