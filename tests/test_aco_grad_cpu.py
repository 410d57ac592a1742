"""DeepACO's training path without a GPU: the restatement (tests/aco_grad_ref.py) against the records of the reference's
own train path, the recorder itself, the C boundary of ``rl4co_aco_tsp_logp_grad``, ``deepaco_loss`` against the reference's
formula, and every refusal of ``heatmap_rollout``, of ``DeepACOPolicy.forward(phase="train")`` and of the binding."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from tests import aco_grad_ref as G

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "rl4co_amd.h").read_text()


# ---- 1. the restatement against the records -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(G.CASES))
def test_restatement_matches_the_recorded_reference(case):
    rec = G.record(case)
    n, ants, b, temperature, _ = G.CASES[case]
    rows = ants * b
    actions, grad_ll = rec["actions"], rec["grad_ll"]
    assert float(rec["temperature"]) == temperature and actions.shape == (rows, n)
    assert torch.equal(actions[:, 0], rec["start_nodes"])
    assert torch.equal(actions.sort(1).values, torch.arange(n).expand(rows, n))
    assert torch.equal(G.tour_reward(rec["locs"], actions), rec["reward"])
    assert float(grad_ll.abs().max()) <= 1.0
    # the floors the tolerances rest on are the recorded ones
    floor = float(rec["grad_noise_floor"])
    assert floor == float((rec["grad32"].double() - rec["grad64"]).abs().max()) and 0 < floor <= G.MEASURED_GRAD_NOISE_FLOOR
    assert float((rec["logps"].double() - rec["logps64"]).abs().max()) <= G.STEP_TOL
    # float64 against float64, float32 within the tolerances
    lp64, g64 = G.logp_grad(rec["heatmap"], actions, grad_ll, temperature=temperature, dtype=torch.float64)
    assert float((lp64 - rec["logps64"]).abs().max()) <= 1e-12 and float((g64 - rec["grad64"]).abs().max()) <= 1e-12
    lp32, g32 = G.logp_grad(rec["heatmap"], actions, grad_ll, temperature=temperature, dtype=torch.float32)
    step_err, grad_err = float((lp32 - rec["logps"]).abs().max()), float((g32.double() - rec["grad64"]).abs().max())
    print(f"{case}: restatement fp32 log-prob error {step_err:.3e} (tol {G.STEP_TOL:.3e}), gradient error {grad_err:.3e} "
          f"(floor {floor:.3e}, tol {G.GRAD_TOL:.3e})")
    assert step_err <= G.STEP_TOL and grad_err <= G.GRAD_TOL
    assert torch.allclose(lp32.sum(1), rec["log_likelihood"], rtol=0, atol=n * G.STEP_TOL)
    assert torch.equal(lp32[:, 0], torch.zeros(rows)) and float(g32.diagonal(dim1=1, dim2=2).abs().max()) == 0.0


def test_restatement_takes_per_step_gradients():
    gen = torch.Generator().manual_seed(3)
    heat, acts = torch.randn(2, 7, 7, generator=gen), G.random_tours(6, 7, gen)
    grad_ll, steps = torch.rand(6, generator=gen), torch.rand(6, 7, generator=gen)
    _, both = G.logp_grad(heat, acts, grad_ll, grad_steps=steps)
    _, only_ll = G.logp_grad(heat, acts, grad_ll)
    _, only_steps = G.logp_grad(heat, acts, torch.zeros(6), grad_steps=steps)
    assert torch.allclose(both, only_ll + only_steps, rtol=0, atol=1e-12)
    steps0 = steps.clone()
    steps0[:, 0] = 99.0  # column 0 is ignored
    assert torch.equal(G.logp_grad(heat, acts, grad_ll, grad_steps=steps0)[1], both)


def test_recorder_reproduces_a_record():
    from oracle import ref_import

    if not ref_import.available():
        pytest.skip("the reference checkout is not here")
    rec, again = G.record("tsp12_a5"), G.reference_run("tsp12_a5")
    for key in ("locs", "heatmap", "start_nodes", "actions", "logps", "reward", "grad_ll", "grad32", "grad64"):
        assert torch.equal(rec[key], torch.as_tensor(again[key])), key


# ---- 2. the C boundary --------------------------------------------------------------------------------------------------------
def test_header_ctypes_and_symbols_agree():
    from rl4co_amd import _lib

    assert int(re.search(r"#define RL4CO_ABI_VERSION (\d+)", HEADER).group(1)) >= 24 and _lib.ABI_VERSION >= 24
    body = re.search(r"typedef struct rl4co_aco_tsp_grad_args \{(.*?)\} rl4co_aco_tsp_grad_args;", HEADER, re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.AcoTspGradArgs._fields_]
    assert ctypes.sizeof(_lib.AcoTspGradArgs) == 6 * 4 + 7 * 8
    handle = _lib.lib()
    assert handle.rl4co_abi_version() == _lib.ABI_VERSION
    assert handle.rl4co_aco_tsp_grad_lds_entries() == 16384
    # arguments are checked on the host before any launch
    args = _lib.AcoTspGradArgs()
    assert handle.rl4co_aco_tsp_logp_grad(ctypes.byref(args), None) == 1 and b"requirement failed" in handle.rl4co_last_error()
    args.B, args.N, args.n_ants, args.row_split, args.temperature = 1, 1025, 1, 1, 1.0
    assert handle.rl4co_aco_tsp_logp_grad(ctypes.byref(args), None) == 1 and b"a.N >= 2" in handle.rl4co_last_error()
    args.N, args.row_split = 12, 13
    assert handle.rl4co_aco_tsp_logp_grad(ctypes.byref(args), None) == 1 and b"a.row_split" in handle.rl4co_last_error()


def test_the_pheromone_term_of_the_forward_is_exactly_zero(tmp_path):
    """heatmap_rollout samples through rl4co_aco_tsp with a pheromone of ones and alpha = beta = 1: its logits are
    1 * rl4co_logf(1) + 1 * heatmap, the heatmap itself only if rl4co_logf(1.0f) is exactly +0 (host build of the header
    the kernels compile; tests/test_math.py pins the device evaluation to the host's bit for bit)."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "log1.c"
    src.write_text('#include <stdio.h>\n#include "rl4co_math.h"\nint main(void) {\n  volatile float one = 1.0f;\n'
                   '  printf("%08x\\n", (unsigned)rl4co_float_to_bits(rl4co_logf(one)));\n  return 0;\n}\n')
    exe = tmp_path / "log1"
    subprocess.run([gcc, "-O2", "-ffp-contract=off", f"-I{ROOT / 'rl4co_amd' / 'csrc'}", str(src), "-o", str(exe), "-lm"], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip() == "00000000"


# ---- 3. the loss ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ls", [False, True])
def test_deepaco_loss_is_the_reference_s_formula(with_ls):
    from rl4co_amd.aco import deepaco_loss

    gen = torch.Generator().manual_seed(11)
    reward, ls_reward = -torch.rand(6, 9, generator=gen) * 5, -torch.rand(6, 9, generator=gen) * 4
    ll = (-torch.rand(6, 9, generator=gen) * 30).requires_grad_(True)
    out = {"reward": reward, "log_likelihood": ll, "ls_reward": ls_reward}
    w = 0.8
    # deepaco/model.py:79-91
    advantage = reward - reward.mean(dim=1, keepdim=True)
    if with_ls:
        ls_advantage = ls_reward - ls_reward.mean(dim=1, keepdim=True)
        weighted = advantage * (1 - w) + ls_advantage * w
    else:
        weighted = advantage
    want = -(weighted * ll).mean()
    got = deepaco_loss(out, train_with_local_search=with_ls, ls_reward_aug_W=w)
    assert torch.equal(got, want)
    (grad,), (grad_want,) = torch.autograd.grad(got, ll), torch.autograd.grad(want, ll)
    assert torch.equal(grad, grad_want) and torch.allclose(grad, -weighted / ll.numel(), rtol=1e-6, atol=0)
    if with_ls:  # the default weight is the reference's 0.95
        assert torch.equal(deepaco_loss(out, True), -((advantage * (1 - 0.95) + ls_advantage * 0.95) * ll).mean())
    else:
        assert torch.equal(deepaco_loss({"reward": reward, "log_likelihood": ll}), want)


# ---- 4. the refusals ------------------------------------------------------------------------------------------------------------
class _PairwiseEncoder(torch.nn.Module):
    """A tiny differentiable stand-in: an MLP on pairwise distances -> (heatmap [B, N, N], None)."""

    def __init__(self):
        super().__init__()
        self.mlp = torch.nn.Sequential(torch.nn.Linear(1, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1))

    def forward(self, td):
        locs = td["locs"]
        d = (locs[:, :, None, :] - locs[:, None, :, :]).norm(p=2, dim=-1)
        return self.mlp(d[..., None])[..., 0], None


def _td(n=12, b=2):
    return {"locs": torch.rand(b, n, 2), "action_mask": torch.ones(b, n, dtype=torch.bool)}


def test_heatmap_rollout_refuses_cpu_tensors_and_bad_shapes():
    from rl4co_amd.aco import heatmap_rollout

    with pytest.raises(NotImplementedError, match="MI355X kernel \\(rl4co_aco_tsp\\) only: heatmap on cpu"):
        heatmap_rollout(torch.randn(2, 6, 6), torch.rand(2, 6, 2), n_ants=3)
    with pytest.raises(NotImplementedError, match="heatmap on cpu"):
        heatmap_rollout(torch.randn(2, 6, 6, requires_grad=True), torch.rand(2, 6, 2), n_ants=3,
                        actions=G.random_tours(6, 6, torch.Generator().manual_seed(0)))


def test_policy_train_refusals():
    from rl4co_amd import DeepACOPolicy

    td = _td()
    # the policy's own kernel encoder carries no gradient: refused, and the message says why
    with pytest.raises(NotImplementedError, match="phase='train'.*inference-only"):
        DeepACOPolicy(num_layers_graph_encoder=1)(td, None, phase="train")
    enc = _PairwiseEncoder()
    with pytest.raises(NotImplementedError, match="env_name='tsp' only"):
        DeepACOPolicy(encoder=enc, env_name="cvrp")(td, None, phase="train")
    pol = DeepACOPolicy(encoder=enc, n_ants=4)
    tours = G.random_tours(8, 12, torch.Generator().manual_seed(0))
    with pytest.raises(NotImplementedError, match="actions="):
        pol(td, None, phase="train", actions=tours)
    with pytest.raises(NotImplementedError, match="return_entropy"):
        pol(td, None, phase="train", return_entropy=True)
    with pytest.raises(NotImplementedError, match="return_sum_log_likelihood"):
        pol(td, None, phase="train", return_sum_log_likelihood=False)
    for key, value in (("top_k", 5), ("top_p", 0.9), ("multisample", True), ("tanh_clipping", 10.0)):
        with pytest.raises(NotImplementedError, match=f"decoding_kwargs\\['{key}'\\] is not served"):
            pol(td, None, phase="train", **{key: value})
    # CPU tensors: the encoder runs, the search refuses
    with pytest.raises(NotImplementedError, match="MI355X kernel \\(rl4co_aco_tsp\\) only: log_heuristic on cpu"):
        pol(td, None, phase="train")
    with pytest.raises(NotImplementedError, match="on cpu"):
        pol(td)  # phase="train" is the default
    # every refusal above came before the encoder ran
    calls = []
    enc.register_forward_hook(lambda *a: calls.append(1))
    for kw in (dict(top_k=5), dict(return_entropy=True), {}):
        with pytest.raises(NotImplementedError):
            pol(td, None, phase="train", **kw)
    assert not calls
    # val / test are untouched by a custom encoder: the search refuses the CPU heatmap
    with pytest.raises(NotImplementedError, match="on cpu"):
        pol.eval()(td, "tsp", phase="test")


def test_binding_argument_checks():
    from rl4co_amd import _lib
    from rl4co_amd import kernels as K

    gen = torch.Generator().manual_seed(5)
    heat, acts, gll = torch.randn(2, 6, 6), G.random_tours(6, 6, gen), torch.rand(6)

    with pytest.raises(TypeError, match="heatmap must be torch.float32"):
        K.aco_tsp_logp_grad(heat.double(), acts, gll)
    with pytest.raises(TypeError, match="actions must be torch.int64"):
        K.aco_tsp_logp_grad(heat, acts.int(), gll)
    with pytest.raises(TypeError, match="grad_ll must be torch.float32"):
        K.aco_tsp_logp_grad(heat, acts, gll.double())
    with pytest.raises(TypeError, match="grad_steps must be torch.float32"):
        K.aco_tsp_logp_grad(heat, acts, gll, grad_steps=torch.rand(6, 6).double())
    with pytest.raises(ValueError, match="heatmap must be \\[B, N, N\\]"):
        K.aco_tsp_logp_grad(torch.randn(2, 6, 5), acts, gll)
    with pytest.raises(ValueError, match="actions must be"):
        K.aco_tsp_logp_grad(heat, acts[:5], gll[:5])  # rows % B
    with pytest.raises(ValueError, match="actions must be"):
        K.aco_tsp_logp_grad(heat, acts[:, :5].contiguous(), gll)
    with pytest.raises(ValueError, match="grad_ll must be"):
        K.aco_tsp_logp_grad(heat, acts, gll[:4])
    with pytest.raises(ValueError, match="grad_steps must be"):
        K.aco_tsp_logp_grad(heat, acts, gll, grad_steps=torch.rand(6, 5))
    with pytest.raises(ValueError, match="temperature"):
        K.aco_tsp_logp_grad(heat, acts, gll, temperature=0.0)
    with pytest.raises(ValueError, match="row_split"):
        K.aco_tsp_logp_grad(heat, acts, gll, row_split=7)
    with pytest.raises(NotImplementedError, match="2..1024 nodes"):
        K.aco_tsp_logp_grad(torch.randn(1, 1025, 1025), torch.zeros(1, 1025, dtype=torch.int64), torch.rand(1))
    with pytest.raises(_lib.Rl4coLibraryError, match="no CPU fallback"):
        K.aco_tsp_logp_grad(heat, acts, gll)
    # about two workgroups per CU, never fewer than sixteen rows per workgroup
    assert K.aco_grad_row_split(8, 100, 256) == 6 and K.aco_grad_row_split(1024, 100, 256) == 1
    assert K.aco_grad_row_split(1, 20, 256) == 1 and K.aco_grad_row_split(64, 1024, 256) == 8
    assert all(n // K.aco_grad_row_split(1, n, 256) >= 16 for n in (16, 31, 32, 100, 1024))
