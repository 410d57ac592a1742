"""GFACS on the MI355X: the log-partition head (csrc/nargnn_logz.hip) alone, forward and all five gradients, at the shapes
where tiling, the pooling stride or the row split can go wrong; run-to-run identity; gradient routing; the host refusals; the
two encoders against the records of the reference's own ``GFACSEncoder`` in ``.train()``; ``GFACSPolicy`` on TSP (with 2-opt)
and CVRP, and the trajectory-balance loss's gradient with the sampled actions fixed.

Tolerance. Per tensor T: ``max |got - ref64| <= 4 max(max |ref32 - ref64|, 2^-23 max |ref64|)`` (``G.bound``): the kernels may
be four times as far from float64 as the fp32 reference itself. ref32 and ref64 come from the record, or from the CPU
restatement (tests/gfacs_ref.py) run in both dtypes; never from kernel output. The heatmap is compared on the graph's entries.
Measured ratios are in DESIGN.md §4.25."""
import ctypes
from functools import lru_cache

import pytest
import torch

from tests import aco_grad_ref as A
from tests import gfacs_ref as G
from tests import nargnn_depot_ref as RD

pytestmark = pytest.mark.gpu

POOLINGS = ("reference", "instance")


def _K():
    from rl4co_amd import kernels as K

    return K


def _compare(tag, got, pairs, on=None):
    """Every tensor of ``pairs`` (name -> (ref32, ref64)) against ``got`` within ``G.bound``; prints the worst ratio."""
    worst = ("", 0.0)
    for name, (ref32, ref64) in pairs.items():
        g = got[name]
        if name.endswith("num_batches_tracked"):
            assert torch.equal(g, ref64), name
            continue
        if name == "heatmap":
            g, ref32, ref64 = g[on], ref32[on], ref64[on]
        tol = G.bound(ref32, ref64)
        err = float((g.double() - ref64.double()).abs().max())
        ratio = err / (tol / 4) if tol > 0 else 0.0
        if ratio > worst[1]:
            worst = (name, ratio)
        print(f"  {tag}: {name} error {err:.3e}, bound {tol:.3e}")
        assert err <= tol, f"{tag}: {name} is {err:.3e} from float64, the bound is {tol:.3e} ({ratio:.2f} x the floor)"
    print(f"{tag}: worst ratio to the fp32 reference's own error {worst[1]:.2f} ({worst[0]})")


# ---- 1. the head alone ----------------------------------------------------------------------------------------------------------
# (B, E, Z): fewer rows than a tile; 330 rows, a ragged last tile, tiles that span groups; the two edge shapes; the general
# case; the largest row count
HEAD_SHAPES = ((1, 2, 1), (3, 110, 2), (16, 17, 1), (17, 16, 2), (5, 240, 2), (1, 10240, 1))
HEAD_NAMES = ("w", "W1", "b1", "W2", "b2")


@lru_cache(maxsize=None)
def _head_inputs(shape):
    b, e, z = shape
    g = torch.Generator().manual_seed(7000 + HEAD_SHAPES.index(shape))
    params = G.z_net_state_dict(7100 + HEAD_SHAPES.index(shape), z)
    return (torch.randn(b, e, 64, generator=g), *(params[key] for key in G.Z_KEYS)), G.upstream_logz(b, z)


@lru_cache(maxsize=None)
def _head_reference(shape, pooling):
    """name -> (ref32, ref64): ``logZ`` and the five gradients of the CPU restatement under the fixed upstream."""
    inputs, upstream = _head_inputs(shape)
    runs = []
    for dtype in (torch.float32, torch.float64):
        leaves = [t.detach().to(dtype).clone().requires_grad_() for t in inputs]
        logz = G.head(*leaves, shape[0], pooling)
        logz.backward(upstream.to(dtype))
        runs.append({"logZ": logz.detach(), **{f"grad/{name}": leaf.grad for name, leaf in zip(HEAD_NAMES, leaves)}})
    return {key: (runs[0][key], runs[1][key]) for key in runs[1]}


def _head_kernel(shape, pooling, upstream=None):
    K = _K()
    inputs, fixed = _head_inputs(shape)
    dev = [t.cuda() for t in inputs]
    upstream = (fixed if upstream is None else upstream).float().cuda()
    logz = K.nargnn_logz_forward(*dev, batch=shape[0], pooling=pooling)
    grads = K.nargnn_logz_backward(*dev, upstream, batch=shape[0], pooling=pooling)
    return {"logZ": logz, **{f"grad/{name}": grads[name] for name in HEAD_NAMES}}


@pytest.mark.parametrize("pooling", POOLINGS)
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=lambda s: "b%d_e%d_z%d" % s)
def test_head_forward_and_all_five_gradients(shape, pooling):
    got = {key: value.cpu() for key, value in _head_kernel(shape, pooling).items()}
    assert got["logZ"].shape == (shape[0], shape[2]) and got["grad/w"].shape == (shape[0], shape[1], 64)
    _compare(f"head {shape} {pooling}", got, _head_reference(shape, pooling))


@pytest.mark.parametrize("shape", [s for s in HEAD_SHAPES if s[0] == 1], ids=lambda s: "b%d_e%d_z%d" % s)
def test_with_one_instance_the_two_pooling_rules_agree_bit_for_bit(shape):
    one, two = _head_kernel(shape, "reference"), _head_kernel(shape, "instance")
    for key in one:
        assert torch.equal(one[key].view(torch.int32), two[key].view(torch.int32)), key


def test_the_two_pooling_rules_differ_with_more_instances():
    shape = (3, 110, 2)
    one, two = _head_kernel(shape, "reference")["logZ"], _head_kernel(shape, "instance")["logZ"]
    ref = _head_reference(shape, "reference")["logZ"]
    assert float((one - two).abs().max()) > 1000 * G.bound(*ref)


@pytest.mark.parametrize("pooling", POOLINGS)
def test_two_runs_give_identical_bits(pooling):
    for shape in ((5, 240, 2), (1, 10240, 1)):
        one, two = _head_kernel(shape, pooling), _head_kernel(shape, pooling)
        for key in one:
            assert torch.equal(one[key].view(torch.int32), two[key].view(torch.int32)), (shape, key)


@pytest.mark.parametrize("pooling", POOLINGS)
def test_gradient_routing(pooling):
    shape = (5, 240, 2)
    zero = _head_kernel(shape, pooling, upstream=torch.zeros(5, 2))
    for name in HEAD_NAMES:
        assert not bool(zero[f"grad/{name}"].any()), name  # exact zeros
    column1 = G.upstream_logz(5, 2).clone()
    column1[:, 0] = 0
    got = _head_kernel(shape, pooling, upstream=column1)
    assert not bool(got["grad/W2"][0].any()) and float(got["grad/b2"][0]) == 0.0
    assert bool(got["grad/W2"][1].any()) and float(got["grad/b2"][1]) != 0.0 and bool(got["grad/W1"].any())


def test_no_double_backward():
    from rl4co_amd.nargnn import _LogZHead

    inputs, _ = _head_inputs((3, 110, 2))
    leaves = [t.cuda().requires_grad_() for t in inputs]
    logz = _LogZHead.apply(*leaves, 3, "reference")
    with pytest.raises(RuntimeError, match="no double backward"):
        torch.autograd.grad(logz.sum(), leaves[0], create_graph=True)
    (grad,) = torch.autograd.grad(logz.sum(), leaves[0])
    assert grad.shape == leaves[0].shape


def test_host_refusals_answer_by_status_and_message():
    from rl4co_amd import _lib

    handle = _lib.lib()
    b, e, z = 3, 110, 2
    inputs, _ = _head_inputs((b, e, z))
    t = dict(zip(HEAD_NAMES, (x.cuda() for x in inputs)))
    rows = b * e
    nbytes = handle.rl4co_nargnn_logz_workspace_bytes(rows)
    assert nbytes == 4 * (2 * rows + 4290 * ((rows + 63) // 64)) and handle.rl4co_nargnn_logz_workspace_bytes(0) == 0
    keep = dict(t, workspace=torch.empty(nbytes // 4, device="cuda"), logZ=torch.empty(b, z, device="cuda"),
                grad_logZ=torch.zeros(b, z, device="cuda"), grad_w=torch.empty(rows, 64, device="cuda"),
                grad_W1=torch.empty(64, 64, device="cuda"), grad_b1=torch.empty(64, device="cuda"),
                grad_W2=torch.empty(z, 64, device="cuda"), grad_b2=torch.empty(z, device="cuda"))

    def args(**change):
        a = _lib.NargnnLogzArgs()
        a.B, a.E, a.Z, a.pooling, a.rows, a.workspace_bytes = b, e, z, _lib.LOGZ_POOL_REFERENCE, rows, nbytes
        for name, tensor in keep.items():
            setattr(a, name, tensor.data_ptr())
        for name, value in change.items():
            setattr(a, name, value)
        return a

    stream = torch.cuda.current_stream().cuda_stream
    for entry in (handle.rl4co_nargnn_logz_forward, handle.rl4co_nargnn_logz_backward):
        assert entry(ctypes.byref(args()), stream) == 0
        for change, words in (({"Z": 3}, b"a.Z == 1 || a.Z == 2"), ({"Z": 0}, b"a.Z == 1 || a.Z == 2"),
                              ({"rows": rows + 1}, b"a.rows == (int64_t)a.B * a.E"), ({"E": e + 1}, b"a.rows == (int64_t)a.B * a.E"),
                              ({"w": None}, b"a.w != nullptr"), ({"b2": None}, b"a.b2 != nullptr"),
                              ({"workspace": None}, b"a.workspace != nullptr"),
                              ({"rows": 0, "B": 0}, b"a.rows >= 1"), ({"rows": -3, "B": -1, "E": 3}, b"a.rows >= 1"),
                              ({"pooling": 2}, b"a.pooling =="), ({"workspace_bytes": nbytes - 4}, b"a.workspace_bytes >=")):
            assert entry(ctypes.byref(args(**change)), stream) == 1, change  # RL4CO_ERR_ARG
            message = handle.rl4co_last_error()
            assert b"requirement failed" in message and words in message, (change, message)
        assert entry(None, stream) == 1
    assert handle.rl4co_nargnn_logz_forward(ctypes.byref(args(logZ=None)), stream) == 1
    assert b"a.logZ != nullptr" in handle.rl4co_last_error()
    assert handle.rl4co_nargnn_logz_backward(ctypes.byref(args(grad_W2=None)), stream) == 1
    assert b"a.grad_W2 != nullptr" in handle.rl4co_last_error()
    torch.cuda.synchronize()
    # and the binding's own: z_out_dim 3, rows that B does not divide, a CPU tensor
    K = _K()
    with pytest.raises(NotImplementedError, match="z_out_dim 1 or 2"):
        K.nargnn_logz_forward(t["w"], t["W1"], t["b1"], torch.zeros(3, 64, device="cuda"), torch.zeros(3, device="cuda"), batch=b)
    with pytest.raises(ValueError, match="rows"):
        K.nargnn_logz_forward(*t.values(), batch=4)
    with pytest.raises(_lib.Rl4coLibraryError, match="no CPU fallback"):
        K.nargnn_logz_forward(t["w"].cpu(), *list(t.values())[1:], batch=b)


# ---- 2. the encoders ------------------------------------------------------------------------------------------------------------
def _module(sd, env, z, pooling="reference"):
    from rl4co_amd import GFACSDepotEncoder, GFACSEncoder

    body = {k: v for k, v in sd.items() if not k.startswith("Z_net.")}
    layers, mlp_layers = RD.count_layers(body)
    enc = (GFACSEncoder if env == "tsp" else GFACSDepotEncoder)(
        env_name=env, num_layers_graph_encoder=layers, num_layers_heatmap_generator=mlp_layers, z_out_dim=z, pooling=pooling)
    enc.load_state_dict(sd, strict=True)
    return enc.cuda().train()


def _encoder_run(sd, env, z, locs, feats, nbr, pooling="reference"):
    """tests.gfacs_ref.run's dict from the module on the given graph."""
    enc = _module(sd, env, z, pooling)
    locs, nbr = locs.cuda(), nbr.cuda()
    b, n = locs.shape[:2]
    dist = RD.distances(locs)
    if env == "tsp":
        logits, embed, logz = enc.encode_train(locs, nbr.to(torch.int32).contiguous(), dist.gather(2, nbr).contiguous())
    else:
        logits, embed, logz = enc.encode_train(locs, feats.cuda(), nbr.to(torch.int32).contiguous(),
                                               dist[:, 1:].gather(2, nbr).contiguous(), dist[:, 1:, 0].contiguous())
    assert logz.shape == (b, z) and logz.requires_grad
    g_heat = (G.upstream_grad(b, n).cuda() * G.on_graph(env, nbr, n)).float()
    torch.autograd.backward([logits, logz], [g_heat, G.upstream_logz(b, z).float().cuda()])
    out = {"heatmap": logits.detach().cpu(), "node_embed": embed.detach().cpu(), "logZ": logz.detach().cpu()}
    named = dict(enc.named_parameters())
    for key, value in enc.state_dict().items():
        if G.is_buffer(key):
            out[f"buf/{key}"] = value.detach().cpu().clone()
        else:
            out[f"grad/{key}"] = (torch.zeros_like(value) if named[key].grad is None else named[key].grad).detach().cpu().clone()
    return out


@pytest.mark.parametrize("case", list(G.CASES))
def test_encoders_against_the_records(case):
    rec = G.record(case)
    env, locs, feats, nbr = G.record_graph(case, rec)
    z = G.CASES[case][2]
    got = _encoder_run(G.case_state_dict(case), env, z, locs, feats, nbr)
    pairs = G.record_pairs(rec)
    assert "grad/Z_net.2.weight" in pairs and "logZ" in pairs and sorted(pairs) == sorted(got)
    _compare(case, got, pairs, G.on_graph(env, nbr, locs.shape[1]))


@pytest.mark.parametrize("env,z,layers,pooling", [("tsp", 1, 0, "reference"), ("op", 2, 0, "instance"), ("pctsp", 2, 1, "instance")])
def test_encoders_against_the_restatement(env, z, layers, pooling):
    """Without GNN layers the head reads the activated edge embedding; the opt-in pooling; the other depot environments."""
    b, n = 3, 13
    sd = G.make_state_dict(env, 811, layers, 2, z)
    locs, feats = G.make_instance(env, b, n, 812)
    nbr = (G.R.select_neighbors(locs.clone(), 10)[0] if env == "tsp" else RD.select_neighbors(locs.clone(), 10)[0])
    refs = [G.run(sd, env, locs, feats, nbr, dtype, pooling) for dtype in (torch.float32, torch.float64)]
    got = _encoder_run(sd, env, z, locs, feats, nbr, pooling)
    _compare(f"{env} L={layers} {pooling}", got, {key: (refs[0][key], refs[1][key]) for key in refs[1]}, G.on_graph(env, nbr, n))


def test_eval_is_the_parent_and_returns_none_for_logz():
    from rl4co_amd import TrainableNARGNNEncoder

    sd = G.case_state_dict("tsp_n11")
    enc = _module(sd, "tsp", 2).eval()
    parent = TrainableNARGNNEncoder(num_layers_graph_encoder=2, num_layers_heatmap_generator=2).eval()
    parent.load_state_dict({k: v for k, v in sd.items() if not k.startswith("Z_net.")}, strict=True)
    td = {"locs": G.make_instance("tsp", 3, 11, 5)[0].cuda()}
    heat, embed, logz = enc(td)
    heat0, embed0 = parent.cuda()(td)
    assert logz is None and torch.equal(heat, heat0) and torch.equal(embed, embed0) and not heat.requires_grad
    out = enc.train()(td)
    assert len(out) == 3 and out[2].shape == (3, 2) and out[2].requires_grad and out[0].requires_grad


# ---- 3. GFACSPolicy on TSP --------------------------------------------------------------------------------------------------------
TSP = dict(n=12, b=4, ants=8, layers=2, mlp_layers=2, alpha=0.7, beta=1.3)


def _param_grads(module):
    return {key: (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu() for key, p in module.named_parameters()}


@lru_cache(maxsize=None)
def _tsp_step():
    """One train-phase forward of the policy and the loss's backward through the kernels."""
    from rl4co_amd import GFACSPolicy, gfacs_loss

    from rl4co_amd.envs import TSPEnv

    sd = G.make_state_dict("tsp", 901, TSP["layers"], TSP["mlp_layers"], 2)
    torch.manual_seed(20)
    env = TSPEnv(generator_params=dict(num_loc=TSP["n"]))
    td = env.reset(batch_size=[TSP["b"]])
    locs = td["locs"].cpu()
    policy = GFACSPolicy(env_name="tsp", aco_kwargs={"use_local_search": True}, n_ants=TSP["ants"], n_iterations=2,
                         num_layers_graph_encoder=TSP["layers"], num_layers_heatmap_generator=TSP["mlp_layers"])
    policy.encoder.load_state_dict(sd, strict=True)
    policy = policy.cuda().train()
    torch.manual_seed(21)
    out = policy(td, env, phase="train", return_hidden=True)
    loss = gfacs_loss(out, "tsp", alpha=TSP["alpha"], beta=TSP["beta"], train_with_local_search=True)
    loss.backward()
    return sd, locs, policy, (td, env), out, loss.detach(), _param_grads(policy.encoder)


def test_policy_tsp_outputs():
    from rl4co_amd.aco import heatmap_rollout

    _, locs, policy, (td, _env), out, loss, _ = _tsp_step()
    b, n, ants = TSP["b"], TSP["n"], TSP["ants"]
    assert set(out) == {"logZ", "reward", "log_likelihood", "actions", "ls_logZ", "ls_reward", "ls_log_likelihood",
                        "ls_actions", "hidden"}
    for key in ("reward", "log_likelihood", "ls_reward", "ls_log_likelihood"):
        assert out[key].shape == (b, ants), key
    assert out["logZ"].shape == out["ls_logZ"].shape == (b, 1)
    assert out["actions"].shape == out["ls_actions"].shape == (ants * b, n) and out["hidden"].shape == (b, n, n)
    assert all(out[key].requires_grad for key in ("logZ", "ls_logZ", "log_likelihood", "ls_log_likelihood"))
    assert bool((out["ls_reward"] >= out["reward"]).all()) and bool((out["ls_reward"] > out["reward"]).any())
    assert bool(torch.isfinite(loss))
    for rows in (out["actions"], out["ls_actions"]):  # permutations
        assert torch.equal(rows.sort(1).values, torch.arange(n, device="cuda").expand(ants * b, n))
    # ls_log_likelihood against the float64 masked log-softmax along ls_actions (tests/aco_grad_ref.py): the returned sums, and
    # step by step the per-step log-probs of the same launch on the same inputs (whose sum is the returned one, bit for bit)
    heat = out["hidden"].detach()
    again = heatmap_rollout(heat, td["locs"], n_ants=ants, actions=out["ls_actions"], temperature=policy.temperature)
    assert torch.equal(again["log_likelihood"].view(ants, b).t(), out["ls_log_likelihood"].detach())
    want = A.rollout_logps(heat.double().cpu(), out["ls_actions"].cpu(), policy.temperature)
    step_err = float((again["logps"].cpu().double() - want).abs().max())
    sum_err = float((out["ls_log_likelihood"].detach().cpu().double() - want.sum(1).view(ants, b).t()).abs().max())
    print(f"ls_log_likelihood: per-step error {step_err:.3e}, summed {sum_err:.3e} (bound {A.STEP_TOL:.3e} a step)")
    # the sum of the n - 1 steps taken (column 0 is the start) is within n - 1 of the file's per-step bounds
    assert step_err <= A.STEP_TOL and sum_err <= (n - 1) * A.STEP_TOL


def test_policy_tsp_loss_gradient_with_the_sampled_actions_fixed():
    sd, locs, policy, (td, _env), out, _, got = _tsp_step()
    b, ants = TSP["b"], TSP["ants"]
    nbr = policy.encoder.neighbors(td["locs"])[0].cpu().long()
    fixed = {key: out[key].detach().cpu() for key in ("reward", "ls_reward", "actions", "ls_actions")}
    refs = {}
    for dtype in (torch.float32, torch.float64):
        logits, _, logz, params, _ = G.encode_train(sd, "tsp", locs, None, nbr, dtype)
        ref = dict(fixed, logZ=logz[:, [0]], ls_logZ=logz[:, [1]])
        for key, rows in (("log_likelihood", "actions"), ("ls_log_likelihood", "ls_actions")):
            ref[key] = A.rollout_logps(logits, fixed[rows], policy.temperature).sum(1).view(ants, b).t()
        G.tb_loss(ref, "tsp", TSP["alpha"], TSP["beta"], True, dtype).backward()
        refs[dtype] = {key: (torch.zeros_like(p) if p.grad is None else p.grad) for key, p in params.items()}
    assert bool(got["Z_net.2.weight"][0].any()) and bool(got["Z_net.2.weight"][1].any())  # both columns of Z_net
    _compare("tsp loss gradient", got, {key: (refs[torch.float32][key], refs[torch.float64][key]) for key in got})


def test_policy_val_phase_returns_deepaco_s_keys():
    _, _, policy, (td, env), _, _, _ = _tsp_step()
    policy.eval()
    try:
        torch.manual_seed(22)
        out = policy(td, env, phase="val")
    finally:
        policy.train()
    assert set(out) == {"reward", "reward_000", "reward_001", "actions"}
    assert out["reward"].shape == (TSP["b"],) and out["actions"].shape == (TSP["b"], TSP["n"])
    assert torch.equal(out["reward"], out["reward_001"]) and bool((out["reward_001"] >= out["reward_000"]).all())


# ---- 4. GFACSPolicy on CVRP -------------------------------------------------------------------------------------------------------
def test_policy_cvrp_loss_gradient_and_log_pb_uniform():
    from rl4co_amd import GFACSPolicy, gfacs_loss, log_pb_uniform
    from rl4co_amd.aco import heatmap_rollout
    from tests import aco_depot_grad_ref as AD

    env, n, b, ants, layers, mlp_layers, beta = "cvrp", 8, 3, 6, 2, 2, 1.3
    data = AD.random_data(env, b, n, 63)
    td = AD.as_td(env, data)
    sd = G.make_state_dict(env, 911, layers, mlp_layers, 1)
    policy = GFACSPolicy(env_name=env, train_with_local_search=False, n_ants=ants, num_layers_graph_encoder=layers,
                         num_layers_heatmap_generator=mlp_layers)
    policy.encoder.load_state_dict(sd, strict=True)
    policy = policy.cuda().train()
    torch.manual_seed(23)
    out = policy(td, env, phase="train", return_hidden=True)
    width = _K().aco_depot_width(env, n)
    assert set(out) == {"logZ", "reward", "log_likelihood", "actions", "hidden"}
    assert out["actions"].shape == (ants * b, width) and out["reward"].shape == out["log_likelihood"].shape == (b, ants)
    assert out["logZ"].shape == (b, 1)
    log_pb = log_pb_uniform(out["actions"], env, ants)
    want = G.reference_log_pb_cvrp(out["actions"], ants)  # the numpy formula on the read-back rows
    assert log_pb.dtype == torch.float64 and log_pb.is_cuda and log_pb.shape == (b, ants)
    assert bool(((log_pb - want).abs() <= 2.0 ** -50 * want.abs()).all()) and bool(torch.isfinite(want).all())
    loss = gfacs_loss(out, env, beta=beta)
    assert loss.dtype == torch.float64
    loss.backward()
    got = _param_grads(policy.encoder)
    # the restatement on the CPU, driven with the same rows: its own heatmap and logZ, the ants' log-likelihood as the masked
    # log-softmax along the rows in the same dtype (tests/aco_depot_grad_ref.py: the masks and lengths from its replay of the
    # rows, which reads the instance and the rows, not the heatmap's values), the loss restated, one backward
    locs, feats = td["locs"].cpu(), td["demand"].cpu()[..., None]
    nbr = policy.encoder.neighbors(td["locs"])[0].cpu().long()
    rows = out["actions"].cpu()
    hidden = out["hidden"].detach()
    followed, lengths, _, _, masks = AD.replay(env, hidden.cpu(), data, actions=rows, temperature=policy.temperature)
    assert torch.equal(followed, rows)
    fixed = {"reward": out["reward"].detach().cpu(), "actions": rows}
    refs = {}
    for dtype in (torch.float32, torch.float64):
        logits, _, logz, params, _ = G.encode_train(sd, env, locs, feats, nbr, dtype)
        ll = AD.rollout_logps(logits, rows, lengths, masks, temperature=policy.temperature).sum(1).view(ants, b).t()
        G.tb_loss(dict(fixed, logZ=logz, log_likelihood=ll), env, 1.0, beta, False, dtype).backward()
        refs[dtype] = {key: (torch.zeros_like(p) if p.grad is None else p.grad) for key, p in params.items()}
    # the policy's own log_likelihood against the float64 masked log-softmax along its rows at its heatmap: the returned
    # sums, and step by step the per-step log-probs of the same launch on the same inputs (the same bits; the reward too)
    rolled = heatmap_rollout(hidden, td["locs"], n_ants=ants, actions=out["actions"], temperature=policy.temperature,
                             env_name=env, td=td)
    assert torch.equal(rolled["reward"].view(ants, b).t(), out["reward"])
    assert torch.equal(rolled["log_likelihood"].view(ants, b).t(), out["log_likelihood"].detach())
    want = AD.rollout_logps(hidden.double().cpu(), rows, lengths, masks, temperature=policy.temperature)
    step_err = float((rolled["logps"].cpu().double() - want).abs().max())
    sum_err = float((out["log_likelihood"].detach().cpu().double() - want.sum(1).view(ants, b).t()).abs().max())
    print(f"cvrp log_likelihood: per-step error {step_err:.3e}, summed {sum_err:.3e} (bound {AD.STEP_TOL[env]:.3e} a step)")
    assert step_err <= AD.STEP_TOL[env] and sum_err <= int(lengths.max()) * AD.STEP_TOL[env]
    _compare("cvrp loss gradient", got, {key: (refs[torch.float32][key], refs[torch.float64][key]) for key in got})
