"""DeepACO's training path on the MI355X (csrc/aco_tsp_grad.hip, rl4co_amd/aco.py, DeepACOPolicy phase="train"): the
backward kernel against the records of the reference's own train path and against the float64 restatement
(tests/aco_grad_ref.py) on the shapes where it can go wrong, its exact properties (run-to-run and split-to-split identical
bits, zeros where nothing contributes), the refusals, the autograd seam, the policy and a short training run.

Tolerance. Against a record and against the float64 restatement alike the gradient stays within GRAD_TOL = 4 x the
reference's own fp32-vs-float64 deviation of its autograd gradient (tests/aco_grad_ref.py), for every shape here."""
from functools import lru_cache

import pytest
import torch

from rl4co_amd import _lib
from tests import aco_grad_ref as G

pytestmark = pytest.mark.gpu
NEG_INF = float("-inf")


def _K():
    from rl4co_amd import kernels as K

    return K


# ---- 1. against the records -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(G.CASES))
def test_forward_and_gradient_against_the_record(case):
    from rl4co_amd.aco import heatmap_rollout

    rec = G.record(case)
    n, ants, b, temperature, _ = G.CASES[case]
    heat = rec["heatmap"].cuda().requires_grad_(True)
    out = heatmap_rollout(heat, rec["locs"].cuda(), n_ants=ants, actions=rec["actions"].cuda(), temperature=temperature)
    assert torch.equal(out["actions"].cpu(), rec["actions"]) and torch.equal(out["reward"].cpu(), rec["reward"])
    step_err = float((out["logps"].detach().cpu() - rec["logps"]).abs().max())
    (out["log_likelihood"] * rec["grad_ll"].cuda()).sum().backward()
    grad_err = float((heat.grad.cpu().double() - rec["grad64"]).abs().max())
    print(f"{case}: log-prob error {step_err:.3e} (tol {G.STEP_TOL:.3e}), gradient error {grad_err:.3e} "
          f"(floor {float(rec['grad_noise_floor']):.3e}, tol {G.GRAD_TOL:.3e})")
    assert step_err <= G.STEP_TOL
    assert torch.equal(out["logps"][:, 0].cpu(), torch.zeros(ants * b))
    assert grad_err <= G.GRAD_TOL
    direct = _K().aco_tsp_logp_grad(rec["heatmap"].cuda(), rec["actions"].cuda(), rec["grad_ll"].cuda(), temperature=temperature)
    assert torch.equal(direct, heat.grad)


# ---- 2. against the float64 restatement ---------------------------------------------------------------------------------------
# name -> (N, ants, B, temperature, grad_steps given, -inf entries, binding keywords)
RANDOM = {
    "n5_a1_b1": (5, 1, 1, 1.0, False, False, {}),
    "n5_a5_b3": (5, 5, 3, 1.0, False, False, {}),
    "n64_a5_b3": (64, 5, 3, 1.0, False, False, {}),
    "n65_a33_b1": (65, 33, 1, 1.0, False, False, {}),
    "n130_a5_b3": (130, 5, 3, 1.0, False, False, {}),
    "n64_a33_b3_t05": (64, 33, 3, 0.5, False, False, {}),
    "n65_a1_b3_steps": (65, 1, 3, 1.0, True, False, {}),
    "n130_a127_b1_scratch": (130, 127, 1, 1.0, False, False, {}),  # 16 510 entries: the table leaves LDS (16 384)
    "n20_a5_b3_scratch_forced": (20, 5, 3, 1.0, False, False, dict(pos_in_scratch=True, row_split=2)),
    "n20_a5_b3_split3": (20, 5, 3, 1.0, True, False, dict(row_split=3)),
    "n1024_a2_b1": (1024, 2, 1, 1.0, False, False, {}),
    "n64_a5_b3_neg_inf": (64, 5, 3, 1.0, False, True, {}),
}


@lru_cache(maxsize=None)
def _random_case(name):
    n, ants, b, temperature, with_steps, neg_inf, _ = RANDOM[name]
    gen = torch.Generator().manual_seed(1000 + sorted(RANDOM).index(name))
    rows = ants * b
    heat = 2.0 * torch.randn(b, n, n, generator=gen)
    acts = G.random_tours(rows, n, gen)
    grad_ll = torch.rand(rows, generator=gen) * 2 - 1
    steps = (torch.rand(rows, n, generator=gen) * 2 - 1) if with_steps else None
    if neg_inf:  # -inf on a third of the off-diagonal entries, never on an edge an ant takes: every step stays feasible
        drop = torch.rand(b, n, n, generator=gen) < 1 / 3
        inst = (torch.arange(rows) % b)[:, None].expand(rows, n - 1)
        drop[inst, acts[:, :-1], acts[:, 1:]] = False
        drop |= torch.eye(n, dtype=torch.bool)
        heat = heat.masked_fill(drop, NEG_INF)
    _, want = G.logp_grad(heat, acts, grad_ll, grad_steps=steps, temperature=temperature, dtype=torch.float64)
    assert bool(torch.isfinite(want).all())
    return heat, acts, grad_ll, steps, want


@pytest.mark.parametrize("name", list(RANDOM))
def test_gradient_against_the_float64_restatement(name):
    n, ants, b, temperature, with_steps, _, kw = RANDOM[name]
    heat, acts, grad_ll, steps, want = _random_case(name)
    K = _K()
    if "scratch" in name and not kw:
        assert ants * n > K.aco_grad_lds_entries()
    got = K.aco_tsp_logp_grad(heat.cuda(), acts.cuda(), grad_ll.cuda(), grad_steps=None if steps is None else steps.cuda(),
                              temperature=temperature, **kw)
    assert got.shape == (b, n, n) and bool(torch.isfinite(got).all())
    err = float((got.cpu().double() - want).abs().max())
    print(f"{name}: gradient error {err:.3e} (tol {G.GRAD_TOL:.3e}, largest entry {float(want.abs().max()):.3e})")
    assert err <= G.GRAD_TOL
    assert float(got.diagonal(dim1=1, dim2=2).abs().max()) == 0.0


# ---- 3. exact properties ------------------------------------------------------------------------------------------------------
def test_launches_and_splits_give_identical_bits():
    K = _K()
    for name in ("n64_a33_b3_t05", "n130_a5_b3", "n65_a1_b3_steps"):
        heat, acts, grad_ll, steps, _ = (None if t is None else t.cuda() for t in _random_case(name))
        kw = dict(grad_steps=steps, temperature=RANDOM[name][3])
        one = K.aco_tsp_logp_grad(heat, acts, grad_ll, row_split=1, **kw)
        assert torch.equal(one, K.aco_tsp_logp_grad(heat, acts, grad_ll, row_split=1, **kw))
        for split in (2, 5, RANDOM[name][0]):
            assert torch.equal(one, K.aco_tsp_logp_grad(heat, acts, grad_ll, row_split=split, **kw)), (name, split)
        assert torch.equal(one, K.aco_tsp_logp_grad(heat, acts, grad_ll, **kw))  # the binding's own choice
        assert torch.equal(one, K.aco_tsp_logp_grad(heat, acts, grad_ll, pos_in_scratch=True, row_split=3, **kw))


def test_zeros_where_nothing_contributes():
    K = _K()
    heat, acts, grad_ll, _, _ = _random_case("n64_a5_b3")
    n, ants, b = 64, 5, 3
    g = grad_ll.clone()
    g.view(ants, b)[:, 1] = 0.0  # instance 1: every upstream gradient is zero
    got = K.aco_tsp_logp_grad(heat.cuda(), acts.cuda(), g.cuda()).cpu()
    assert float(got[1].abs().max()) == 0.0 and float(got[0].abs().max()) > 0 and float(got[2].abs().max()) > 0
    # one ant: the row of its last node gets nothing, the row of every other node does
    one = K.aco_tsp_logp_grad(heat[:1].cuda(), acts[:1].cuda(), torch.ones(1).cuda()).cpu()[0]
    last = int(acts[0, -1])
    assert float(one[last].abs().max()) == 0.0
    assert all(float(one[i].abs().max()) > 0 for i in acts[0, :-2].tolist())
    # ... and the row of the node before the last one holds (1 - p) = 0 on its single feasible node
    assert float(one[int(acts[0, -2])].abs().max()) == 0.0
    # visited nodes get nothing: row a_t is zero on a_0 .. a_t
    for t in (0, 1, 30, 62):
        assert float(one[int(acts[0, t]), acts[0, : t + 1]].abs().max()) == 0.0


# ---- 4. errors --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["above_range", "negative", "repeated"])
def test_bad_tours_are_refused_per_instance(kind):
    K = _K()
    heat, acts, grad_ll, _, _ = _random_case("n64_a5_b3")
    n, ants, b = 64, 5, 3
    clean = K.aco_tsp_logp_grad(heat.cuda(), acts.cuda(), grad_ll.cuda())
    bad = acts.clone()
    row = 2 * b + 1  # ant 2 of instance 1
    if kind == "repeated":
        bad[row, 40] = bad[row, 3]
    else:
        bad[row, 40] = n if kind == "above_range" else -1
    bit, message = ((_lib.EBIT_INVALID_TOUR, "Invalid tour") if kind == "repeated"
                    else (_lib.EBIT_TOUR_INDEX, "tour index out of range"))
    for kw in ({}, dict(row_split=4), dict(pos_in_scratch=True)):
        err = K.new_error_word("cuda")
        got = K.aco_tsp_logp_grad(heat.cuda(), bad.cuda(), grad_ll.cuda(), err=err, **kw)
        assert int(err.item()) == bit
        assert float(got[1].abs().max()) == 0.0
        assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])
    with pytest.raises(AssertionError, match=message):
        K.aco_tsp_logp_grad(heat.cuda(), bad.cuda(), grad_ll.cuda())


# ---- 5. the autograd seam ---------------------------------------------------------------------------------------------------------
def test_heatmap_rollout_backward_is_the_kernel():
    from rl4co_amd.aco import heatmap_rollout

    K = _K()
    gen = torch.Generator().manual_seed(21)
    b, n, ants = 3, 21, 7
    locs = torch.rand(b, n, 2, generator=gen).cuda()
    heat = (2.0 * torch.randn(b, n, n, generator=gen)).cuda().requires_grad_(True)
    w = (torch.rand(ants * b, generator=gen) * 2 - 1).cuda()
    out = heatmap_rollout(heat, locs, n_ants=ants, temperature=0.8, seed=7)
    acts = out["actions"]
    assert acts.shape == (ants * b, n) and torch.equal(acts.sort(1).values.cpu(), torch.arange(n).expand(ants * b, n))
    assert torch.equal(acts[:, 0].cpu(), (torch.arange(ants) % n).repeat_interleave(b))
    assert torch.equal(out["logps"][:, 0], torch.zeros(ants * b, device="cuda"))
    assert torch.equal(out["log_likelihood"], out["logps"].sum(1))
    assert torch.equal(out["reward"], K.tour_length(locs, acts, negate=True))
    assert out["log_likelihood"].requires_grad and out["logps"].requires_grad
    assert not out["actions"].requires_grad and not out["reward"].requires_grad
    (w * out["log_likelihood"]).sum().backward()
    assert torch.equal(heat.grad, K.aco_tsp_logp_grad(heat.detach(), acts, w, temperature=0.8))
    # the per-step log-probs carry the gradient too, and both add up
    ws = (torch.rand(ants * b, n, generator=gen) * 2 - 1).cuda()
    again = heatmap_rollout(heat, locs, n_ants=ants, temperature=0.8, seed=7)
    assert torch.equal(again["actions"], acts) and torch.equal(again["logps"], out["logps"])  # the same seed, the same ants
    (grad,) = torch.autograd.grad((ws * again["logps"]).sum() + (w * again["log_likelihood"]).sum(), heat)
    assert torch.equal(grad, K.aco_tsp_logp_grad(heat.detach(), acts, w, grad_steps=ws, temperature=0.8))
    assert not torch.equal(heatmap_rollout(heat, locs, n_ants=ants, temperature=0.8, seed=8)["actions"], acts)
    # evaluation of given tours: the forced forward reports the sampled run's log-probs
    forced = heatmap_rollout(heat, locs, n_ants=ants, temperature=0.8, actions=acts)
    assert torch.equal(forced["logps"], out["logps"]) and torch.equal(forced["reward"], out["reward"])
    # no double backward
    fresh = heatmap_rollout(heat, locs, n_ants=ants, seed=7)
    with pytest.raises(RuntimeError, match="no double backward"):
        torch.autograd.grad(fresh["log_likelihood"].sum(), heat, create_graph=True)
    # a heatmap that needs no gradient: nothing is recorded, nothing is saved
    plain = heatmap_rollout(heat.detach(), locs, n_ants=ants, temperature=0.8, seed=7)
    assert plain["log_likelihood"].grad_fn is None and not plain["log_likelihood"].requires_grad
    assert plain["logps"].grad_fn is None and torch.equal(plain["logps"], out["logps"])
    # the caller's error word: nothing raises, the bit is there
    err = K.new_error_word("cuda")
    heatmap_rollout(heat.detach(), locs, n_ants=ants, start_nodes=torch.full((ants * b,), n), err=err)
    assert int(err.item()) == _lib.EBIT_TOUR_INDEX


def test_a_refusal_of_the_backward_launch_comes_through_the_seam():
    """The forward accepts its tours; the saved tours are then spoiled behind autograd's back (``.data`` leaves the version
    counter alone), so only the backward launch can refuse: with ``err=None`` it reads its own word and raises, with the
    caller's word it sets the bit there and raises nothing."""
    from rl4co_amd.aco import heatmap_rollout

    gen = torch.Generator().manual_seed(22)
    b, n, ants = 2, 9, 3
    locs = torch.rand(b, n, 2, generator=gen).cuda()
    heat = torch.randn(b, n, n, generator=gen).cuda().requires_grad_(True)
    out = heatmap_rollout(heat, locs, n_ants=ants, seed=1)
    out["actions"].data[1 * b + 1, 4] = out["actions"].data[1 * b + 1, 2]  # ant 1 of instance 1 repeats a node
    with pytest.raises(AssertionError, match="Invalid tour"):
        out["log_likelihood"].sum().backward()
    err = _K().new_error_word("cuda")
    out = heatmap_rollout(heat, locs, n_ants=ants, seed=1, err=err)
    assert int(err.item()) == 0
    out["actions"].data[1 * b + 1, 4] = out["actions"].data[1 * b + 1, 2]
    heat.grad = None
    out["log_likelihood"].sum().backward()
    assert int(err.item()) == _lib.EBIT_INVALID_TOUR
    assert float(heat.grad[1].abs().max()) == 0.0 and float(heat.grad[0].abs().max()) > 0


# ---- 6. the policy ------------------------------------------------------------------------------------------------------------------
class _PairwiseEncoder(torch.nn.Module):
    """A tiny differentiable encoder: an MLP on pairwise distances -> (heatmap [B, N, N], None)."""

    def __init__(self):
        super().__init__()
        self.mlp = torch.nn.Sequential(torch.nn.Linear(1, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1))

    def forward(self, td):
        locs = td["locs"]
        d = (locs[:, :, None, :] - locs[:, None, :, :]).norm(p=2, dim=-1)
        return self.mlp(d[..., None])[..., 0], None


def _td(b, n, seed):
    locs = torch.rand(b, n, 2, generator=torch.Generator().manual_seed(seed)).cuda()
    return {"locs": locs, "action_mask": torch.ones(b, n, dtype=torch.bool, device="cuda")}


@pytest.mark.parametrize("use_nls", [False, True])
def test_policy_trains_an_encoder_through_the_kernels(use_nls):
    from rl4co_amd import DeepACOPolicy
    from rl4co_amd.aco import deepaco_loss

    torch.manual_seed(3)
    b, n, ants = 4, 20, 6
    enc = _PairwiseEncoder().cuda()
    pol = DeepACOPolicy(encoder=enc, n_ants=ants, temperature=0.9, train_with_local_search=True,
                        aco_kwargs=dict(use_local_search=True, use_nls=use_nls))
    out = pol(_td(b, n, 5), None, phase="train")
    assert out["reward"].shape == out["log_likelihood"].shape == out["ls_reward"].shape == (b, ants)
    assert out["actions"].shape == (ants * b, n) and out["hidden"].shape == (b, n, n) and out["hidden"].requires_grad
    assert bool((out["ls_reward"] >= out["reward"]).all()) and bool((out["ls_reward"] > out["reward"]).any())
    assert bool((out["reward"] < 0).all()) and bool((out["log_likelihood"] < 0).all())
    loss = deepaco_loss(out, train_with_local_search=True)
    loss.backward()
    for p in enc.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    # the keywords of the reference's call; without local search nothing of it is returned
    plain = DeepACOPolicy(encoder=enc, n_ants=ants)(_td(b, n, 5), "tsp", phase="train", return_actions=False, return_hidden=False)
    assert sorted(plain) == ["log_likelihood", "reward"]


# ---- 7. learning ----------------------------------------------------------------------------------------------------------------------
def test_a_free_heatmap_learns_shorter_tours():
    """B = 8, N = 20, 16 ants, Adam(lr = 0.2), 40 steps: on the CPU restatement (torch multinomial, autograd) the mean tour
    length falls from 10.0 over the first five steps to 6.2 - 6.6 over the last five (three seeds); here only the direction."""
    from rl4co_amd.aco import deepaco_loss, heatmap_rollout

    torch.manual_seed(0)
    b, n, ants = 8, 20, 16
    locs = _td(b, n, 9)["locs"]
    heat = torch.nn.Parameter(torch.zeros(b, n, n, device="cuda"))
    opt = torch.optim.Adam([heat], lr=0.2)
    lengths = []
    for step in range(40):
        out = heatmap_rollout(heat, locs, n_ants=ants, seed=100 + step)
        loss = deepaco_loss({"reward": out["reward"].view(ants, b).t(), "log_likelihood": out["log_likelihood"].view(ants, b).t()})
        opt.zero_grad()
        loss.backward()
        opt.step()
        lengths.append(-out["reward"].mean())
    lengths = torch.stack(lengths).cpu()
    first, last = float(lengths[:5].mean()), float(lengths[-5:].mean())
    print(f"mean tour length: first five steps {first:.3f}, last five {last:.3f}")
    assert last < first
