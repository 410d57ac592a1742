"""DeepACO's training path on the depot graphs without a GPU: the restatement (tests/aco_depot_grad_ref.py) against the
records of the reference's own train path, the C boundary of ``rl4co_aco_depot_logp_grad``, and the host-side refusals of
``heatmap_rollout``, of ``NonAutoregressivePolicy`` and of the binding."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from tests import aco_depot_grad_ref as G

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "rl4co_amd.h").read_text()
RECORDS = [(env, case) for env in G.ENVS for case in G.CASES]


# ---- 1. the restatement against the records -------------------------------------------------------------------------------
@pytest.mark.parametrize("env,case", RECORDS)
def test_restatement_matches_the_recorded_reference(env, case):
    rec = G.record(env, case)
    c, ants, b, temperature, _ = G.CASES[case]
    n, rows = c + 1, ants * b
    w = G.width(env, n)
    actions, grad_ll, data = rec["actions"], rec["grad_ll"], G.record_data(env, rec)
    assert float(rec["temperature"]) == temperature and actions.shape == (rows, w) and rec["heatmap"].shape == (b, n, n)
    assert float(grad_ll.abs().max()) <= 1.0
    # the floors the tolerances rest on are the recorded ones
    floor = float(rec["grad_noise_floor"])
    assert floor == float((rec["grad32"].double() - rec["grad64"]).abs().max())
    assert 0 < floor <= G.GRAD_NOISE_FLOORS[f"{env}_{case}"] <= G.MEASURED_GRAD_NOISE_FLOOR and G.GRAD_TOL == 4 * G.MEASURED_GRAD_NOISE_FLOOR
    assert float((rec["logps"].double() - rec["logps64"]).abs().max()) <= G.STEP_TOL[env]
    # the fp32 restatement of the sampling kernel follows the recorded rows: its lengths, its per-step log-probs, its masks
    acts, lengths, logps, _, masks = G.replay(env, rec["heatmap"], data, actions=actions, temperature=temperature)
    assert torch.equal(acts, actions) and torch.equal(lengths, rec["lengths"])
    assert float((logps - rec["logps"]).abs().max()) <= G.STEP_TOL[env]
    taken = masks.gather(2, actions[:, :, None]).squeeze(2)
    assert not bool(taken.any())  # every recorded action is feasible under the restatement's masks
    worst = float(G.PZ.ulps(G.reward_w(env, data, actions), rec["reward"], G.reward_scale(env, data, actions)).max())
    assert worst <= G.REWARD_ULPS[env]
    # float64 against float64, float32 within the tolerances
    lp64, g64 = G.logp_grad(rec["heatmap"], actions, lengths, masks, grad_ll, temperature=temperature, dtype=torch.float64)
    assert float((lp64 - rec["logps64"]).abs().max()) <= 1e-12 and float((g64 - rec["grad64"]).abs().max()) <= 1e-12
    lp32, g32 = G.logp_grad(rec["heatmap"], actions, lengths, masks, grad_ll, temperature=temperature, dtype=torch.float32)
    step_err, grad_err = float((lp32 - rec["logps"]).abs().max()), float((g32.double() - rec["grad64"]).abs().max())
    print(f"{env}_{case}: restatement fp32 log-prob error {step_err:.3e} (tol {G.STEP_TOL[env]:.3e}), gradient error "
          f"{grad_err:.3e} (floor {floor:.3e}, tol {G.GRAD_TOL:.3e})")
    assert step_err <= G.STEP_TOL[env] and grad_err <= G.GRAD_TOL
    # the depot row is left at step 0 by every ant; a row never left is zero
    assert float(g64[:, 0].abs().max()) > 0
    left = torch.zeros(b, n, dtype=torch.bool)
    live = torch.arange(w)[None, :] < (lengths[:, None].long() - 1)
    left[(torch.arange(rows) % b)[:, None].expand(rows, w)[live], actions[live]] = True
    left[:, 0] = True
    assert float(g64[~left].abs().max() if bool((~left).any()) else 0.0) == 0.0


def test_restatement_takes_per_step_gradients_and_ignores_padding():
    env, b, n, ants = "cvrp", 2, 8, 3
    data = G.random_data(env, b, n, 5)
    gen = torch.Generator().manual_seed(3)
    heat = torch.randn(b, n, n, generator=gen)
    acts, lengths, _, _, masks = G.sample_rows(env, heat, data, ants, 6)
    rows, w = acts.shape
    grad_ll, steps = torch.rand(rows, generator=gen), torch.rand(rows, w, generator=gen)
    _, both = G.logp_grad(heat, acts, lengths, masks, grad_ll, grad_steps=steps)
    _, only_ll = G.logp_grad(heat, acts, lengths, masks, grad_ll)
    _, only_steps = G.logp_grad(heat, acts, lengths, masks, torch.zeros(rows), grad_steps=steps)
    assert torch.allclose(both, only_ll + only_steps, rtol=0, atol=1e-12)
    padded = steps.clone()
    padded[torch.arange(w)[None, :] >= lengths[:, None]] = 99.0  # the steps after a row's length are ignored
    assert int(lengths.min()) < w and torch.equal(G.logp_grad(heat, acts, lengths, masks, grad_ll, grad_steps=padded)[1], both)


# ---- 2. the C boundary --------------------------------------------------------------------------------------------------------
def test_header_ctypes_and_symbols_agree():
    from rl4co_amd import _lib

    assert int(re.search(r"#define RL4CO_ABI_VERSION (\d+)", HEADER).group(1)) >= 25 and _lib.ABI_VERSION >= 25
    assert re.search(r"\n \*  25: rl4co_aco_depot_logp_grad", HEADER)
    body = re.search(r"typedef struct rl4co_aco_depot_grad_args \{(.*?)\} rl4co_aco_depot_grad_args;", HEADER, re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.AcoDepotGradArgs._fields_]
    assert ctypes.sizeof(_lib.AcoDepotGradArgs) == 8 * 4 + 12 * 8
    handle = _lib.lib()
    assert handle.rl4co_abi_version() == _lib.ABI_VERSION
    entries = handle.rl4co_aco_depot_grad_lds_entries()
    assert entries == 8192
    assert handle.rl4co_aco_depot_grad_scratch_bytes(30, 101) == (6 * 30 * 101 + 4 * 30 + 15) // 16 * 16
    assert handle.rl4co_aco_depot_grad_scratch_bytes(1, 1025) == -1
    # arguments are checked on the host before any launch
    call = handle.rl4co_aco_depot_logp_grad
    args = _lib.AcoDepotGradArgs()
    assert call(ctypes.byref(args), None) == 1 and b"a.env ==" in handle.rl4co_last_error()  # 0 is TSP
    args.env, args.B, args.N, args.n_ants, args.row_split, args.temperature = _lib.ENV_OP, 1, 1025, 1, 1, 1.0
    assert call(ctypes.byref(args), None) == 1 and b"a.N >= 2" in handle.rl4co_last_error()
    args.N, args.row_split = 12, 13
    assert call(ctypes.byref(args), None) == 1 and b"a.row_split" in handle.rl4co_last_error()
    args.row_split, args.multistart = 1, 1
    assert call(ctypes.byref(args), None) == 1 and b"a.multistart" in handle.rl4co_last_error()
    args.multistart, args.temperature = 0, 0.0
    assert call(ctypes.byref(args), None) == 1 and b"a.temperature" in handle.rl4co_last_error()


def test_the_rules_are_one_text():
    """The sampling kernels and the backward call ant_rules.h; none restates a rule."""
    csrc = ROOT / "rl4co_amd" / "csrc"
    rules = (csrc / "ant_rules.h").read_text()
    for name in ("cvrp_threshold", "cvrp_fits", "cvrp_advance", "cvrp_depot_ok", "op_dist", "op_advance", "op_within",
                 "pctsp_advance", "pctsp_depot_ok"):
        assert f" {name}(" in rules
    for source, names in (("aco_cvrp.hip", ("cvrp_threshold", "cvrp_fits", "cvrp_advance", "cvrp_depot_ok")),
                          ("aco_prize.hip", ("op_dist", "op_advance", "op_within", "pctsp_advance", "pctsp_depot_ok")),
                          ("aco_depot_grad.hip", ("cvrp_threshold", "cvrp_fits", "cvrp_advance", "cvrp_depot_ok", "op_dist",
                                                  "op_advance", "op_within", "pctsp_advance", "pctsp_depot_ok"))):
        text = (csrc / source).read_text()
        code = "\n".join(line.split("//")[0] for line in text.splitlines())
        assert '#include "ant_rules.h"' in text
        for name in names:
            assert f"{name}(" in code, (source, name)
        assert "1e-5f" not in code and "sqrtf(" not in code and "< 1.0f" not in code, source


# ---- 3. the refusals ------------------------------------------------------------------------------------------------------------
class _FreeHeatmap(torch.nn.Module):
    def __init__(self, b, n):
        super().__init__()
        self.heatmap = torch.nn.Parameter(torch.zeros(b, n, n))
        self.calls = 0

    def forward(self, td):
        self.calls += 1
        return self.heatmap, None


def test_heatmap_rollout_refusals():
    from rl4co_amd.aco import heatmap_rollout

    heat, locs = torch.randn(2, 6, 6), torch.rand(2, 6, 2)
    for env in ("cvrp", "op", "pctsp", "spctsp"):
        with pytest.raises(NotImplementedError, match="MI355X"):
            heatmap_rollout(heat, locs, n_ants=3, env_name=env, td={})
    with pytest.raises(NotImplementedError, match="MI355X"):
        heatmap_rollout(heat, locs, n_ants=3)  # the TSP call is what it was


def test_binding_refusals():
    from rl4co_amd import _lib
    from rl4co_amd import kernels as K

    b, n, ants = 2, 6, 3
    heat, gll = torch.randn(b, n, n), torch.rand(ants * b)
    acts = torch.zeros(ants * b, n, dtype=torch.int64)
    prize = torch.rand(b, n)
    with pytest.raises(NotImplementedError, match="serves"):
        K.aco_depot_logp_grad(heat, acts, gll, env="tsp")
    with pytest.raises(TypeError, match="heatmap"):
        K.aco_depot_logp_grad(heat.double(), acts, gll, env="pctsp", prize=prize)
    with pytest.raises(TypeError, match="actions"):
        K.aco_depot_logp_grad(heat, acts.int(), gll, env="pctsp", prize=prize)
    with pytest.raises(ValueError, match="actions must be"):
        K.aco_depot_logp_grad(heat, acts, gll, env="cvrp", demand=torch.rand(b, n - 1), vehicle_capacity=torch.ones(b))  # W = 9
    with pytest.raises(ValueError, match="grad_ll"):
        K.aco_depot_logp_grad(heat, acts, gll[:4], env="pctsp", prize=prize)
    with pytest.raises(ValueError, match="grad_steps"):
        K.aco_depot_logp_grad(heat, acts, gll, env="pctsp", prize=prize, grad_steps=torch.rand(ants * b, n - 1))
    with pytest.raises(ValueError, match="takes prize"):
        K.aco_depot_logp_grad(heat, acts, gll, env="pctsp")
    with pytest.raises(ValueError, match="takes max_length"):
        K.aco_depot_logp_grad(heat, acts, gll, env="op", locs=torch.rand(b, n, 2))
    with pytest.raises(ValueError, match="takes demand"):
        K.aco_depot_logp_grad(heat, torch.zeros(ants * b, 9, dtype=torch.int64), gll, env="cvrp", vehicle_capacity=torch.ones(b))
    with pytest.raises(NotImplementedError, match="multistart"):
        K.aco_depot_logp_grad(heat, acts, gll, env="op", locs=torch.rand(b, n, 2), max_length=torch.rand(b, n), multistart=True)
    with pytest.raises(ValueError, match="temperature"):
        K.aco_depot_logp_grad(heat, acts, gll, env="pctsp", prize=prize, temperature=0.0)
    with pytest.raises(ValueError, match="row_split"):
        K.aco_depot_logp_grad(heat, acts, gll, env="pctsp", prize=prize, row_split=7)
    with pytest.raises(NotImplementedError, match="2..1024"):
        K.aco_depot_logp_grad(torch.randn(1, 1025, 1025), torch.zeros(1, 1025, dtype=torch.int64), torch.rand(1), env="pctsp",
                              prize=torch.rand(1, 1025))
    with pytest.raises(_lib.Rl4coLibraryError, match="no CPU fallback"):
        K.aco_depot_logp_grad(heat, acts, gll, env="pctsp", prize=prize)
    assert K.aco_depot_width("cvrp", 11) == 19 and K.aco_depot_width("op", 11) == K.aco_depot_width("spctsp", 11) == 11


def test_policy_refusals_come_before_the_encoder():
    import rl4co_amd
    from rl4co_amd import NonAutoregressivePolicy

    assert "NonAutoregressivePolicy" in rl4co_amd.__all__
    b, n = 2, 6
    td = {"locs": torch.rand(b, n, 2)}
    enc = _FreeHeatmap(b, n)
    pol = NonAutoregressivePolicy(enc, env_name="cvrp", temperature=0.9)
    ok = dict(multisample=True, num_samples=3)
    for kw, match in ((dict(phase="val", **ok), "DeepACOPolicy"), (dict(phase="test", **ok), "DeepACOPolicy"),
                      (dict(actions=torch.zeros(6, 9, dtype=torch.int64), **ok), "actions="),
                      (dict(return_entropy=True, **ok), "return_entropy"),
                      (dict(return_sum_log_likelihood=False, **ok), "return_sum_log_likelihood"),
                      (dict(top_k=3, **ok), "top_k"), (dict(top_p=0.9, **ok), "top_p"), (dict(tanh_clipping=10.0, **ok), "tanh_clipping"),
                      (dict(mask_logits=False, **ok), "mask_logits"), (dict(select_best=True, **ok), "select_best"),
                      (dict(decode_type="greedy", **ok), "decode types"), (dict(beam_width=3, **ok), "beam_width"),
                      (dict(), "exactly one"), (dict(multisample=True), "num_samples"),
                      (ok, "MI355X")):  # the last: CPU tensors
        with pytest.raises(NotImplementedError, match=match):
            pol(td, None, **kw)
    with pytest.raises(NotImplementedError, match="multistart for tsp and cvrp"):
        NonAutoregressivePolicy(enc, env_name="op", train_decode_type="multistart_sampling")(td, None, num_starts=3)
    with pytest.raises(NotImplementedError, match="tsp with multistart"):
        NonAutoregressivePolicy(enc, env_name="tsp")(td, None, **ok)
    with pytest.raises(NotImplementedError, match="serves env_name"):
        NonAutoregressivePolicy(enc, env_name="pdp")
    with pytest.raises(NotImplementedError, match="decoder"):
        NonAutoregressivePolicy(enc, decoder=object())
    assert enc.calls == 0
