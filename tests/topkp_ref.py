"""Float64 checker of the top-k / top-p (nucleus) filter of utils/decoding.py:109-188, for the tests of the fused decode
kernels' filter (am_decode.hip header, csrc/topkp.h). Pinned to the reference's own process_logits by
tests/test_topkp_cpu.py."""
import torch


def filter_f64(z: torch.Tensor, top_k: int = 0, top_p: float = 0.0) -> torch.Tensor:
    """Kept set [..., N] (bool) of processed logits ``z`` (-inf = masked): top-k (ties at the k-th value kept), then
    top-p over the survivors (stable ascending order, remove cumulative mass <= 1 - p)."""
    z = z.double()
    n = z.shape[-1]
    if top_k > 0:
        tau = torch.topk(z, min(top_k, n), dim=-1)[0][..., -1:]
        z = z.masked_fill(z < tau, float("-inf"))
    if 0.0 < top_p < 1.0:
        zs, idx = torch.sort(z, dim=-1, stable=True)
        cum = zs.softmax(-1).cumsum(-1)
        rm = torch.zeros_like(cum, dtype=torch.bool).scatter(-1, idx, cum <= 1 - top_p)
        z = z.masked_fill(rm, float("-inf"))
    return z > float("-inf")


def top_p_margin(z: torch.Tensor, top_k: int, top_p: float) -> torch.Tensor:
    """Per row: the smallest |A_c - (1 - p) Z| / Z over the top-k survivors (how close the row's top-p cut is to a tie)."""
    z = z.double()
    if top_k > 0:
        tau = torch.topk(z, min(top_k, z.shape[-1]), dim=-1)[0][..., -1:]
        z = z.masked_fill(z < tau, float("-inf"))
    if not (0.0 < top_p < 1.0):
        return torch.full(z.shape[:-1], float("inf"), dtype=torch.float64)
    zs, _ = torch.sort(z, dim=-1, stable=True)
    cum = zs.softmax(-1).cumsum(-1)
    d = (cum - (1 - top_p)).abs().masked_fill(zs == float("-inf"), float("inf"))
    return d.min(-1)[0]


def top_p_entry_margins(z: torch.Tensor, top_k: int, top_p: float) -> torch.Tensor:
    """Per entry [..., N]: |A_c - (1 - p) Z| / Z of the top-k survivors, in node order (inf elsewhere or without top-p) —
    how close entry c sits to the top-p cut."""
    z = z.double()
    if top_k > 0:
        tau = torch.topk(z, min(top_k, z.shape[-1]), dim=-1)[0][..., -1:]
        z = z.masked_fill(z < tau, float("-inf"))
    if not (0.0 < top_p < 1.0):
        return torch.full(z.shape, float("inf"), dtype=torch.float64)
    zs, idx = torch.sort(z, dim=-1, stable=True)
    cum = zs.softmax(-1).cumsum(-1)
    d = (cum - (1 - top_p)).abs().masked_fill(zs == float("-inf"), float("inf"))
    return torch.empty_like(d).scatter(-1, idx, d)


def process_logits_f64(logits, mask, temperature=1.0, top_p=0.0, top_k=0, tanh_clipping=0.0, mask_logits=True):
    """decoding.py:138-188 in float64: clip, mask, temperature, top-k, top-p, log_softmax."""
    z = logits.double()
    if tanh_clipping > 0:
        z = torch.tanh(z) * tanh_clipping
    if mask_logits:
        z = z.masked_fill(~mask, float("-inf"))
    z = z / temperature
    if top_p > 0:
        assert top_p <= 1.0, "top-p should be in (0, 1]."
    kept = filter_f64(z, top_k, top_p)
    return torch.log_softmax(z.masked_fill(~kept, float("-inf")), dim=-1)


def unpack_bits(bits: torch.Tensor, n: int) -> torch.Tensor:
    """[..., W] int32 words -> [..., n] bool (bit j % 32 of word j / 32)."""
    j = torch.arange(n, device=bits.device)
    return ((bits[..., j // 32] >> (j % 32)) & 1) != 0


# ---- recorded reference rollouts with a filter (tests/golden/reference/topkp_rollout_*.npz) ---------------------------
ROLLOUT_CASES = {
    "k5": dict(decode_type="sampling", top_k=5),
    "p0.9": dict(decode_type="sampling", top_p=0.9),
    "k10_p0.8_t0.7": dict(decode_type="sampling", top_k=10, top_p=0.8, temperature=0.7),
    "greedy_p0.5": dict(decode_type="greedy", top_p=0.5),
    "sampling_eval": dict(decode_type="sampling", num_starts=4, multisample=True, select_best=True, top_p=0.9, top_k=10,
                          starts_fn=True),
}


def start_nodes_fn(td, env, num_starts):
    """A deterministic ``select_start_nodes_fn`` (decoding.py:308-311): the environment's own first start nodes."""
    return env.select_start_nodes(td, num_starts=num_starts)


def reference_rollout(env_name: str, num_loc: int, batch: int, case: str) -> dict:
    """The reference's own AttentionModelPolicy on CPU in fp32 with the filter, seeded as oracle/gen_golden.py (weights,
    data, sampling stream); needs the reference checkout (only run when recording)."""
    from oracle import ref_import
    from tests.helpers import DATA_SEED, SAMPLE_SEED, WEIGHT_SEED

    ref = ref_import.load()
    env_cls = {"tsp": ref.TSPEnv, "cvrp": ref.CVRPEnv}[env_name]
    ref_env = env_cls(generator_params=dict(num_loc=num_loc), seed=0)
    torch.manual_seed(WEIGHT_SEED)
    pol = ref.AttentionModelPolicy(env_name=env_name).eval()
    torch.manual_seed(DATA_SEED)
    data = ref_env.generator(batch_size=[batch])
    td0 = ref_env.reset(data.clone())
    kw = dict(ROLLOUT_CASES[case])
    starts = []
    if kw.pop("starts_fn", False):
        def fn(td, env, n):
            s = start_nodes_fn(td, env, n)
            starts.append(s.clone())
            return s
        kw["select_start_nodes_fn"] = fn
    torch.manual_seed(SAMPLE_SEED)
    with torch.inference_mode():
        out = pol(td0.clone(), ref_env, phase="test", **kw)
    rec = {"actions": out["actions"], "log_likelihood": out["log_likelihood"], "reward": out["reward"]}
    if starts:
        rec["start_nodes"] = starts[0]
    rec.update({f"in_{k}": v for k, v in data.items()})
    return rec


def rollout_record(env_name: str, num_loc: int, batch: int, case: str) -> dict:
    from tests.helpers import reference_record

    return reference_record(f"topkp_rollout_{env_name}{num_loc}_b{batch}_{case}",
                            lambda: reference_rollout(env_name, num_loc, batch, case))
