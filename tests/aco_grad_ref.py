"""DeepACO's training path for TSP (the ants' log-likelihood and its gradient with respect to the heatmap): a plain-torch
restatement of the constructive rollout under ``NonAutoregressiveDecoder`` (gather the current node's heatmap row, mask the
visited nodes, divide by the temperature, ``log_softmax``, gather the action, sum), evaluable in float32 and float64 with
autograd, and the recorder of the reference's own train path (``NonAutoregressivePolicy`` with a stand-in encoder whose
output is a free parameter; tests/golden/reference/aco_grad_*.npz). tests/test_aco_grad_cpu.py pins the restatement to the
records; the GPU tests compare the kernels with the records and the float64 restatement.
Rows are ant-major everywhere: row ``j * B + b`` is ant ``j`` of instance ``b``."""
import torch

from tests.aco_ref import STEP_TOL, tour_reward  # noqa: F401  (the per-step log-prob tolerance and the CPU reward)

# case -> (N, ants, B, temperature, seed)
CASES = {"tsp12_a5": (12, 5, 4, 1.0, 4321), "tsp20_a20_t07": (20, 20, 4, 0.7, 4322)}
# The gradient's tolerance against the recorded float64 gradient: 4 x the largest deviation of the reference's OWN fp32
# autograd gradient from the float64 one over the records (the key "grad_noise_floor" of each record, measured by the
# recorder on the CPU, |grad_ll| <= 1) — the rule aco_ref.STEP_TOL uses.
MEASURED_GRAD_NOISE_FLOOR = 5.252e-07  # tsp20_a20_t07 (5.2516e-07 rounded up); tsp12_a5 2.221e-07
GRAD_TOL = 4 * MEASURED_GRAD_NOISE_FLOOR


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def rollout_logps(heatmap, actions, temperature=1.0):
    """heatmap [B, N, N] (float32 or float64, may require grad), actions [rows, N] -> per-step log-probs [rows, N], column
    0 (the start node) 0."""
    b, n, _ = heatmap.shape
    rows = actions.shape[0]
    idx = torch.arange(rows, device=heatmap.device)
    visited = torch.zeros(rows, n, dtype=torch.bool, device=heatmap.device)
    visited[idx, actions[:, 0]] = True
    cols = [torch.zeros(rows, dtype=heatmap.dtype, device=heatmap.device)]
    for t in range(1, n):
        z = heatmap[idx % b, actions[:, t - 1]].masked_fill(visited, float("-inf"))
        if temperature != 1.0:
            z = z / temperature
        cols.append(torch.log_softmax(z, -1)[idx, actions[:, t]])
        visited = visited.clone()
        visited[idx, actions[:, t]] = True
    return torch.stack(cols, 1)


def logp_grad(heatmap, actions, grad_ll, grad_steps=None, temperature=1.0, dtype=torch.float64):
    """(logps [rows, N], d sum_r(grad_ll[r] * ll[r] + sum_t grad_steps[r, t] * logps[r, t]) / d heatmap) in ``dtype``."""
    h = heatmap.detach().to(dtype).requires_grad_(True)
    logps = rollout_logps(h, actions, temperature)
    total = (grad_ll.to(dtype) * logps.sum(1)).sum()
    if grad_steps is not None:
        total = total + (grad_steps.to(dtype)[:, 1:] * logps[:, 1:]).sum()
    (grad,) = torch.autograd.grad(total, h)
    return logps.detach(), grad


def random_tours(rows, n, generator):
    return torch.stack([torch.randperm(n, generator=generator) for _ in range(rows)], 0)


def sample_tours(heatmap, start_nodes, temperature, generator):
    """The rollout itself in torch on the CPU (multinomial from the masked softmax): tours for the learning test's
    rehearsal. heatmap [B, N, N], start_nodes [rows] -> actions [rows, N]."""
    b, n, _ = heatmap.shape
    rows = start_nodes.shape[0]
    idx = torch.arange(rows)
    visited = torch.zeros(rows, n, dtype=torch.bool)
    visited[idx, start_nodes] = True
    tour = [start_nodes]
    for _ in range(1, n):
        z = heatmap[idx % b, tour[-1]].masked_fill(visited, float("-inf")) / temperature
        nxt = torch.multinomial(torch.softmax(z, -1), 1, generator=generator)[:, 0]
        visited[idx, nxt] = True
        tour.append(nxt)
    return torch.stack(tour, 1)


# ---- the recorder (needs the reference checkout) ------------------------------------------------------------------------------
def reference_policy_class():
    """The reference's NonAutoregressivePolicy, its files executed verbatim; two more empty package shells keep the package
    ``__init__`` files (and the autoregressive models they import) out."""
    import importlib
    import sys

    from oracle import ref_import

    ref_import.install()
    for pkg in ("rl4co.models.common.constructive", "rl4co.models.common.constructive.nonautoregressive"):
        if pkg not in sys.modules:
            mod = ref_import._Shell(pkg)
            mod.__path__ = [str(ref_import.REFERENCE_ROOT / pkg.replace(".", "/"))]
            mod.__package__ = pkg
            sys.modules[pkg] = mod
            setattr(sys.modules[pkg.rpartition(".")[0]], pkg.rpartition(".")[2], mod)
    return importlib.import_module("rl4co.models.common.constructive.nonautoregressive.policy").NonAutoregressivePolicy


class _FreeHeatmap(torch.nn.Module):
    """The stand-in encoder: its output is a free parameter, so the parameter's gradient is the heatmap's."""

    def __init__(self, heatmap):
        super().__init__()
        self.heatmap = torch.nn.Parameter(heatmap.clone())

    def forward(self, td):
        return self.heatmap, None


def reference_run(case: str) -> dict:
    """The reference's own train path (ConstructivePolicy.forward, multistart sampling, its Sampling strategy and TSPEnv) on
    the CPU in fp32, then the same tours in float64 through its own process_logits."""
    from oracle import ref_import

    ref = ref_import.load()
    policy_cls = reference_policy_class()
    n, ants, b, temperature, seed = CASES[case]
    rows = ants * b
    torch.manual_seed(seed)
    env = ref.TSPEnv(generator_params=dict(num_loc=n))
    td0 = env.reset(env.generator(batch_size=[b]))
    locs = td0["locs"].clone()
    gen = torch.Generator().manual_seed(seed + 1)
    heatmap = 2.0 * torch.randn(b, n, n, generator=gen)
    grad_ll = torch.rand(rows, generator=gen) * 2 - 1  # |grad_ll| <= 1
    starts = []

    def pick(td, env_, num_starts):
        s = torch.randint(0, n, (num_starts * b,), generator=gen)
        starts.append(s.clone())
        return s

    enc = _FreeHeatmap(heatmap)
    policy = policy_cls(enc, env_name="tsp", train_decode_type="multistart_sampling")
    out = policy(td0.clone(), env, phase="train", num_starts=ants, select_start_nodes_fn=pick, temperature=temperature,
                 return_actions=True, return_sum_log_likelihood=False)
    logps, actions, reward = out["log_likelihood"], out["actions"], out["reward"]  # [rows, N] per step, [rows, N], [rows]
    assert len(starts) == 1 and torch.equal(actions[:, 0], starts[0]) and logps.shape == (rows, n)
    ll = logps.sum(1)  # decoding.py get_log_likelihood(return_sum=True)
    (grad_ll * ll).sum().backward()
    grad32 = enc.heatmap.grad.clone()
    # the same steps in float64, through the reference's own process_logits
    h64 = heatmap.double().requires_grad_(True)
    idx = torch.arange(rows)
    mask = torch.ones(rows, n, dtype=torch.bool)
    mask[idx, actions[:, 0]] = False
    cols = [torch.zeros(rows, dtype=torch.float64)]
    for t in range(1, n):
        lp = ref.decoding.process_logits(h64[idx % b, actions[:, t - 1]], mask, temperature=temperature)
        cols.append(lp[idx, actions[:, t]])
        mask = mask.clone()
        mask[idx, actions[:, t]] = False
    logps64 = torch.stack(cols, 1)
    (grad64,) = torch.autograd.grad((grad_ll.double() * logps64.sum(1)).sum(), h64)
    return {"locs": locs, "heatmap": heatmap, "start_nodes": starts[0], "actions": actions, "logps": logps.detach(),
            "logps64": logps64.detach(), "log_likelihood": ll.detach(), "reward": reward.detach(), "grad_ll": grad_ll,
            "grad32": grad32, "grad64": grad64, "temperature": torch.tensor(temperature, dtype=torch.float64),
            "grad_noise_floor": (grad32.double() - grad64).abs().max()}


def record(case: str) -> dict:
    from tests.helpers import reference_record

    return reference_record(f"aco_grad_{case}", lambda: reference_run(case))


if __name__ == "__main__":  # RL4CO_RECORD_REFERENCE=1 python -m tests.aco_grad_ref
    for name in CASES:
        r = record(name)
        print(name, float(r["grad_noise_floor"]), float((r["logps"].double() - r["logps64"]).abs().max()),
              {k: tuple(v.shape) for k, v in r.items()})
