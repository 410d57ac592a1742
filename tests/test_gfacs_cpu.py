"""GFACS without a GPU: the two encoders' keys, strict load and refusals, the restated head against the records of the
reference's own ``GFACSEncoder`` (which settle the pooling rule), ``log_pb_uniform`` against the reference's numpy / scipy
lines, ``gfacs_loss`` against a float64 line-by-line restatement, and the two schedules.

``log_pb_uniform`` for cvrp is float64 and uses ``torch.lgamma`` where the reference uses ``scipy.special.gammaln``. Measured on
the CPU for n = 0 .. 2048 (``lgamma(n + 1)``): the worst relative gap between the two is 3.4e-16 (exactly 0 where the value is
0, n = 0 and 1). The test measures it again and allows four times that, and never less than 2^-50 = 8.9e-16, relative to the
reference's value."""
import math

import numpy as np
import pytest
import torch

from tests import gfacs_ref as G
from tests import nargnn_depot_train_ref as TD
from tests import nargnn_train_ref as T

ENVS = ("tsp", "cvrp", "op", "pctsp")


def _encoder(env, **kw):
    from rl4co_amd import GFACSDepotEncoder, GFACSEncoder

    return (GFACSEncoder if env == "tsp" else GFACSDepotEncoder)(env_name=env, **kw)


# ---- the encoders -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ENVS)
def test_state_dict_keys_are_the_reference_class_s(env):
    keys = G.recorded_keys()[env]
    assert keys[-4:] == list(G.Z_KEYS)
    assert list(_encoder(env, z_out_dim=2).state_dict().keys()) == keys


@pytest.mark.parametrize("case", list(G.CASES))
def test_a_gfacs_state_dict_loads_strictly(case):
    env, _, z, layers, mlp_layers = G.CASES[case][:5]
    sd = G.case_state_dict(case)
    enc = _encoder(env, z_out_dim=z, num_layers_graph_encoder=layers, num_layers_heatmap_generator=mlp_layers)
    enc.load_state_dict(sd, strict=True)
    assert all(torch.equal(enc.state_dict()[key], value) for key, value in sd.items())
    assert enc.z_out_dim == z and enc.pooling == "reference"
    # the parents cannot take it: Z_net's keys are unexpected there
    from rl4co_amd import TrainableNARGNNDepotEncoder, TrainableNARGNNEncoder

    parent = (TrainableNARGNNEncoder if env == "tsp" else TrainableNARGNNDepotEncoder)(
        env_name=env, num_layers_graph_encoder=layers, num_layers_heatmap_generator=mlp_layers)
    with pytest.raises(RuntimeError, match="Z_net"):
        parent.load_state_dict(sd, strict=True)


@pytest.mark.parametrize("env", ("tsp", "cvrp"))
def test_eval_returns_none_for_logz(env, monkeypatch):
    from rl4co_amd import nargnn

    heat, embed = torch.zeros(2, 5, 5), torch.zeros(2, 5, 64)
    parent = nargnn.NARGNNEncoder if env == "tsp" else nargnn.NARGNNDepotEncoder
    monkeypatch.setattr(parent, "forward", lambda self, td: (heat, embed))  # (the fused inference kernel's launch)
    out = _encoder(env, num_layers_graph_encoder=1).eval()({"locs": torch.zeros(2, 5, 2)})
    assert len(out) == 3 and out[0] is heat and out[1] is embed and out[2] is None


def test_refusals():
    from rl4co_amd import GFACSPolicy

    for env in ENVS:
        with pytest.raises(NotImplementedError, match="z_out_dim 1 or 2"):
            _encoder(env, z_out_dim=3)
        with pytest.raises(ValueError, match="pooling"):
            _encoder(env, pooling="mean")
    for env, why in (("cvrp", "HGS"), ("op", "destroy-and-repair"), ("pctsp", "destroy-and-repair")):
        with pytest.raises(NotImplementedError, match=why):  # the default: train_with_local_search=True
            GFACSPolicy(env_name=env, aco_kwargs={"use_local_search": True}, num_layers_graph_encoder=1)
        policy = GFACSPolicy(env_name=env, train_with_local_search=False, num_layers_graph_encoder=1)
        assert policy.encoder.z_out_dim == 1 and type(policy.encoder).__name__ == "GFACSDepotEncoder"
    with pytest.raises(AssertionError):  # local search in training needs the search's own switch, as in the reference
        GFACSPolicy(num_layers_graph_encoder=1)
    policy = GFACSPolicy(aco_kwargs={"use_local_search": True}, num_layers_graph_encoder=1)
    assert policy.encoder.z_out_dim == 2 and policy.train_with_local_search
    with pytest.raises(ValueError, match="z_out_dim=2"):
        GFACSPolicy(encoder=_encoder("tsp", z_out_dim=1, num_layers_graph_encoder=1), aco_kwargs={"use_local_search": True})
    # CPU tensors in train: the encoder and the policy (before the encoder runs)
    td = {"locs": torch.rand(2, 6, 2)}
    with pytest.raises(NotImplementedError, match="MI355X"):
        _encoder("tsp", num_layers_graph_encoder=1).train()(td)
    with pytest.raises(NotImplementedError, match="MI355X"):
        _encoder("cvrp", num_layers_graph_encoder=1).train()({**td, "demand": torch.rand(2, 5)})
    with pytest.raises(NotImplementedError, match="MI355X"):
        policy.train()(td, "tsp", phase="train")
    for kw in ({"actions": torch.zeros(2, 6, dtype=torch.int64)}, {"return_entropy": True}, {"return_sum_log_likelihood": False}):
        with pytest.raises(NotImplementedError, match="does not serve"):
            policy(td, "tsp", phase="train", **kw)
    with pytest.raises(NotImplementedError, match="top_k"):
        policy(td, "tsp", phase="train", top_k=3)


# ---- the head against the records -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(G.CASES))
def test_the_restated_head_reproduces_the_record_and_the_record_settles_the_pooling(case):
    rec = G.record(case)
    env, locs, feats, nbr = G.record_graph(case, rec)
    sd = G.case_state_dict(case)
    ref32, ref64 = rec["logZ32"], rec["logZ64"]
    assert ref64.shape == (G.BATCH, G.CASES[case][2])
    tol = G.bound(ref32, ref64)
    for dtype, ref in ((torch.float32, ref32), (torch.float64, ref64)):
        got = G.run(sd, env, locs, feats, nbr, dtype)  # pooling="reference": gfacs/encoder.py:62 read literally
        err = float((got["logZ"].double() - ref.double()).abs().max())
        print(f"{case} {dtype}: logZ is {err:.3e} from the record (bound {tol:.3e})")
        assert got["logZ"].dtype == dtype and err <= (tol if dtype == torch.float32 else 1e-12)
        for name, (r32, r64) in G.record_pairs(rec).items():  # and the rest of the encoder with it
            want = r32 if dtype == torch.float32 else r64
            if name.endswith("num_batches_tracked"):
                assert torch.equal(got[name], want)
            else:
                assert float((got[name].double() - want.double()).abs().max()) <= G.bound(r32, r64), name
    # the per-instance mean is another number: far outside the bound at B = 3
    other = G.run(sd, env, locs, feats, nbr, torch.float64, pooling="instance")["logZ"]
    assert float((other - ref64).abs().max()) > 1000 * tol


@pytest.mark.parametrize("case", list(G.CASES))
def test_without_the_head_the_restatement_is_the_trainable_encoder_s(case):
    rec = G.record(case)
    env, locs, feats, nbr = G.record_graph(case, rec)
    sd = G.case_state_dict(case)
    body = {k: v for k, v in sd.items() if not k.startswith("Z_net.")}
    mine = G.encode_train(sd, env, locs, feats, nbr, torch.float64)[0]
    if env == "tsp":
        theirs = T.encode_train(body, locs, dtype=torch.float64, neighbors=nbr)[0]
    else:
        theirs = TD.encode_train(body, locs, feats, dtype=torch.float64, neighbors=nbr)[0]
    assert float((mine - theirs).detach().abs().max()) <= 1e-11


# ---- log_pb_uniform ---------------------------------------------------------------------------------------------------------------
def _lgamma_gap():
    import scipy.special

    n = np.arange(0, 2049)
    ours, theirs = torch.lgamma(torch.from_numpy(n + 1).double()).numpy(), scipy.special.gammaln(n + 1)
    assert np.all(ours[theirs == 0] == 0)
    some = theirs != 0
    return float((np.abs(ours - theirs)[some] / np.abs(theirs[some])).max())


def test_log_pb_uniform_cvrp_is_the_reference_s_numpy_formula():
    from rl4co_amd import log_pb_uniform

    gap = _lgamma_gap()
    tol = max(4 * gap, 2.0 ** -50)
    print(f"torch.lgamma against scipy.special.gammaln, n = 0 .. 2048: worst relative gap {gap:.3e}; bound {tol:.3e}")
    rows = torch.tensor([
        [1, 2, 3, 4, 5, 6, 0, 0, 0, 0, 0],   # one route
        [1, 0, 2, 0, 3, 0, 4, 0, 5, 0, 6],   # all single-customer routes
        [1, 2, 0, 3, 4, 0, 5, 6, 0, 0, 0],   # two-customer routes
        [3, 1, 0, 2, 0, 0, 0, 0, 0, 0, 0],   # a zero-filled tail
        [6, 5, 4, 0, 3, 0, 2, 1, 0, 0, 0],
        [2, 0, 1, 3, 4, 5, 0, 6, 0, 0, 0],
    ], dtype=torch.int64)
    for n_ants in (1, 2, 3, 6):
        got, want = log_pb_uniform(rows, "cvrp", n_ants), G.reference_log_pb_cvrp(rows, n_ants)
        assert got.dtype == torch.float64 and got.shape == want.shape == (6 // n_ants, n_ants)
        assert bool(((got - want).abs() <= tol * want.abs()).all()), (got, want)
    # seeded valid rows: a permutation of 40 customers cut into routes at random places, zero-filled to the kernel's width
    gen = torch.Generator().manual_seed(3)
    long = torch.zeros(64, 79, dtype=torch.int64)
    for row in long:
        tour, at = torch.randperm(40, generator=gen) + 1, 0
        for i, customer in enumerate(tour):
            row[at] = customer
            at += 1 if i == 39 or torch.rand((), generator=gen) < 0.6 else 2  # (a skipped entry stays 0: back to the depot)
    got, want = log_pb_uniform(long, "cvrp", 8), G.reference_log_pb_cvrp(long, 8)
    assert bool(torch.isfinite(want).all()) and float(want.min()) < -20
    assert bool(((got - want).abs() <= tol * want.abs()).all())


def test_log_pb_uniform_constants():
    from rl4co_amd import log_pb_uniform

    for width in (5, 12, 100):
        assert log_pb_uniform(torch.zeros(6, width, dtype=torch.int64), "tsp", 3) == math.log(1 / 2 * width)  # as written
    for env in ("op", "pctsp"):
        assert log_pb_uniform(torch.zeros(6, 9, dtype=torch.int64), env, 3) == math.log(1 / 2)
    with pytest.raises(ValueError, match="Unknown environment"):
        log_pb_uniform(torch.zeros(6, 9, dtype=torch.int64), "pdp", 3)


# ---- the loss and the schedules -----------------------------------------------------------------------------------------------------
def _policy_out(env, b=3, ants=4, width=9, seed=5):
    g = torch.Generator().manual_seed(seed)
    out = {key: torch.randn(b, ants, generator=g) for key in ("reward", "log_likelihood", "ls_log_likelihood")}
    out["ls_reward"] = out["reward"] + torch.rand(b, ants, generator=g)
    out["logZ"], out["ls_logZ"] = torch.randn(b, 1, generator=g), torch.randn(b, 1, generator=g)
    for key in ("actions", "ls_actions"):  # valid depot rows: 5 customers cut into routes, zero-filled
        out[key] = torch.zeros(ants * b, width, dtype=torch.int64)
        for row in out[key]:
            tour, at = torch.randperm(5, generator=g) + 1, 0
            for i, customer in enumerate(tour):
                row[at] = customer
                at += 1 if i == 4 or torch.rand((), generator=g) < 0.5 else 2
    return out


@pytest.mark.parametrize("ls", (False, True))
@pytest.mark.parametrize("env", ENVS)
def test_gfacs_loss_is_the_reference_s_trajectory_balance(env, ls):
    from rl4co_amd import gfacs_loss

    out = _policy_out(env)
    for key in ("log_likelihood", "ls_log_likelihood", "logZ", "ls_logZ"):
        out[key].requires_grad_()
    alpha, beta = 0.7, 1.3
    got = gfacs_loss(out, env, alpha=alpha, beta=beta, train_with_local_search=ls)
    want = G.tb_loss(out, env, alpha, beta, ls)
    assert got.dtype == (torch.float64 if env == "cvrp" else torch.float32)  # the reference's own promotion
    assert abs(float(got.detach()) - float(want.detach())) <= 8 * 2.0 ** -23 * max(1.0, abs(float(want.detach())))
    got.backward()
    leaves = {key: out[key].detach().double().requires_grad_() for key in ("log_likelihood", "ls_log_likelihood", "logZ", "ls_logZ")}
    G.tb_loss({**out, **leaves}, env, alpha, beta, ls).backward()
    for key, leaf in leaves.items():
        if not ls and key.startswith("ls_"):
            assert out[key].grad is None
            continue
        assert float((out[key].grad.double() - leaf.grad).abs().max()) <= 8 * 2.0 ** -23 * max(1.0, float(leaf.grad.abs().max()))
    if not ls:  # the local-search keys are not read
        short = {k: v for k, v in out.items() if not k.startswith("ls_")}
        assert torch.equal(gfacs_loss(short, env, alpha=alpha, beta=beta), got.detach())


def test_schedules_are_the_reference_s_properties():
    from rl4co_amd import gfacs_alpha, gfacs_beta

    for epoch in (0, 1, 7, 44, 45, 60, 99):
        for max_epochs in (50, 100):
            want = 0.5 + (1.0 - 0.5) * min(epoch / (max_epochs - 5), 1.0)  # model.py:77-80 with its defaults
            assert gfacs_alpha(epoch, max_epochs) == want
            want = 0.2 + (0.9 - 0.2) * min(epoch / (max_epochs - 3), 1.0)
            assert gfacs_alpha(epoch, max_epochs, alpha_min=0.2, alpha_max=0.9, alpha_flat_epochs=3) == want
            assert gfacs_beta(epoch, max_epochs) == 1.0  # model.py:84-88 with its defaults: beta_min == beta_max
            want = 1.0 + (4.0 - 1.0) * min(math.log(epoch + 1) / math.log(max_epochs - 7), 1.0)
            assert gfacs_beta(epoch, max_epochs, beta_min=1.0, beta_max=4.0, beta_flat_epochs=7) == want
    assert gfacs_alpha(0, 50) == 0.5 and gfacs_alpha(45, 50) == 1.0 and gfacs_beta(0, 50, beta_max=3.0) == 1.0


def test_exports():
    import rl4co_amd

    for name in ("GFACSEncoder", "GFACSDepotEncoder", "GFACSPolicy", "gfacs_loss", "log_pb_uniform", "gfacs_alpha", "gfacs_beta"):
        assert name in rl4co_amd.__all__ and getattr(rl4co_amd, name) is not None
