"""The trainable depot-graph heatmap encoder on the MI355X (csrc/nargnn_train.hip's depot instantiation,
rl4co_amd.TrainableNARGNNDepotEncoder): one train-mode forward and backward against the records of the reference's own
``NARGNNEncoder(env_name=...)`` in ``.train()``, against the float64 restatement (tests/nargnn_depot_train_ref.py) at the
shapes where tiling, row segments or degrees can go wrong, on a hand-made graph, on bad input, for run-to-run identity, and
under NonAutoregressivePolicy end to end.

Tolerance. Per tensor T: ``max |got - ref64| <= 4 max(max |ref32 - ref64|, 2^-23 max |ref64|)`` (``T.bound``): the kernel may
be four times as far from float64 as the fp32 reference itself. ref32 and ref64 come from the record, or from the CPU
restatement run in both dtypes where there is no record; never from kernel output. The heatmap is compared on the graph's
entries (everywhere else both sides hold the fill constant). Measured ratios are in DESIGN.md §4.24."""
from functools import lru_cache

import pytest
import torch

from tests import nargnn_depot_ref as R
from tests import nargnn_depot_train_ref as T

pytestmark = pytest.mark.gpu


def _K():
    from rl4co_amd import kernels as K

    return K


def _module(sd, env, k_sparse=None, bias=True):
    from rl4co_amd import TrainableNARGNNDepotEncoder

    layers, mlp_layers = R.count_layers(sd)
    enc = TrainableNARGNNDepotEncoder(env_name=env, num_layers_graph_encoder=layers, num_layers_heatmap_generator=mlp_layers,
                                      k_sparse=k_sparse, linear_bias=bias)
    enc.load_state_dict(sd, strict=True)
    return enc.cuda().train()


def _kernel_run(sd, env, locs, feats, nbr, bias=True, enc=None):
    """tests.nargnn_depot_train_ref.run's dict from the module on the given graph."""
    enc = _module(sd, env, bias=bias) if enc is None else enc
    locs, feats, nbr = locs.cuda(), feats.cuda(), nbr.cuda()
    b, n = locs.shape[:2]
    dist = R.distances(locs)
    cost = dist[:, 1:].gather(2, nbr.long()).contiguous()
    depot_cost = dist[:, 1:, 0].contiguous()
    logits, embed = enc.encode_train(locs, feats, nbr.to(torch.int32).contiguous(), cost, depot_cost)
    logits.backward((T.upstream_grad(b, n).cuda() * R.on_graph(nbr, n)).float())
    out = {"heatmap": logits.detach().cpu(), "node_embed": embed.detach().cpu()}
    named = dict(enc.named_parameters())
    for key, value in enc.state_dict().items():
        if T.is_buffer(key):
            out[f"buf/{key}"] = value.detach().cpu().clone()
        else:
            out[f"grad/{key}"] = (torch.zeros_like(value) if named[key].grad is None else named[key].grad).detach().cpu().clone()
    return out


def _compare(tag, got, pairs, on):
    """Every tensor of ``pairs`` (name -> (ref32, ref64)) against ``got`` within ``T.bound``; prints the worst ratio."""
    worst = ("", 0.0)
    for name, (ref32, ref64) in pairs.items():
        g = got[name]
        if name.endswith("num_batches_tracked"):
            assert torch.equal(g, ref64), name
            continue
        if name == "heatmap":
            g, ref32, ref64 = g[on], ref32[on], ref64[on]
        tol = T.bound(ref32, ref64)
        err = float((g.double() - ref64.double()).abs().max())
        ratio = err / (tol / 4) if tol > 0 else 0.0
        if ratio > worst[1]:
            worst = (name, ratio)
        assert err <= tol, f"{tag}: {name} is {err:.3e} from float64, the bound is {tol:.3e} ({ratio:.2f} x the floor)"
    print(f"{tag}: worst ratio to the fp32 reference's own error {worst[1]:.2f} ({worst[0]})")


def _both(sd, locs, feats, nbr):
    ref32, ref64 = T.run(sd, locs, feats, nbr, torch.float32), T.run(sd, locs, feats, nbr, torch.float64)
    return {key: (ref32[key], ref64[key]) for key in ref64}


# ---- 1. the records ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(T.CASES))
def test_records(case):
    rec = T.record(case)
    env, n = T.CASES[case][:2]
    nbr = R.edge_index_to_neighbors(rec["edge_index"], T.BATCH, n)
    got = _kernel_run(T.case_state_dict(case), env, rec["locs"], rec["feats"], nbr)
    pairs = T.record_pairs(rec)
    assert "grad/init_embedding.init_embed_depot.weight" in pairs and sorted(pairs) == sorted(got)
    _compare(case, got, pairs, R.on_graph(nbr, n))


# ---- 2. seeded shapes against the restatement ---------------------------------------------------------------------------------
# id -> (env, B, N, K, GNN layers, MLP layers, linear_bias)
SHAPES = {
    "n3": ("cvrp", 1, 3, 1, 1, 2, True), "n4": ("op", 1, 4, 2, 1, 2, True), "c16": ("pctsp", 3, 17, 10, 2, 2, True),
    "c17": ("cvrp", 3, 18, 10, 2, 2, True), "n34": ("op", 3, 34, 10, 2, 2, True), "k17": ("pctsp", 3, 40, 17, 2, 2, True),
    "k40": ("cvrp", 1, 60, 40, 1, 2, True), "b1": ("op", 1, 24, 10, 2, 2, True), "b5": ("pctsp", 5, 24, 10, 2, 2, True),
    "one_layer": ("cvrp", 3, 24, 10, 1, 2, True), "no_bias": ("op", 3, 24, 10, 2, 3, False),
    "n200_k40": ("pctsp", 2, 200, 40, 1, 2, True), "n1024": ("cvrp", 1, 1024, 10, 1, 2, True),
    "past_the_cap": ("op", 8, 200, 40, 1, 2, True),
}


@lru_cache(maxsize=None)
def _shape_case(name):
    env, b, n, k, layers, mlp_layers, bias = SHAPES[name]
    seed = 3000 + list(SHAPES).index(name)
    sd = R.make_state_dict(env, seed, layers, mlp_layers, linear_bias=bias)
    locs, feats = R.make_instance(env, b, n, seed + 500)
    nbr, _, _ = R.select_neighbors(locs.clone(), k)
    return sd, locs, feats, nbr, _both(sd, locs, feats, nbr)


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name):
    sd, locs, feats, nbr, pairs = _shape_case(name)
    env, b, n, k = SHAPES[name][:4]
    assert nbr.shape == (b, n - 1, k)
    if name == "past_the_cap":
        assert b * (n - 1) * (k + 2) > 64 * 1024  # more rows than 1024 workgroups of 64
    got = _kernel_run(sd, env, locs, feats, nbr, bias=SHAPES[name][6])
    _compare(name, got, pairs, R.on_graph(nbr, n))


# ---- 3. a hand-made graph -------------------------------------------------------------------------------------------------------
def test_a_customer_everybody_lists_and_a_customer_nobody_lists():
    b, n, k = 2, 10, 3
    c = n - 1
    gen = torch.Generator().manual_seed(9)
    nbr = torch.empty(b, c, k, dtype=torch.int64)
    for bb in range(b):
        for i in range(1, n):  # customer 1 is in every other customer's list, customer 2 in nobody's
            others = [j for j in range(3, n) if j != i]
            pick = [others[int(t)] for t in torch.randperm(len(others), generator=gen)[:k]]
            nbr[bb, i - 1] = torch.tensor(pick if i == 1 else [1] + pick[:k - 1])
    ptr, _ = _K().depot_incoming_csr(nbr.to(torch.int32).cuda())
    degree = (ptr[1:] - ptr[:-1]).view(b, n).cpu()
    # customer 1: the c - 1 other customers and the depot; customer 2: the depot alone; the depot: every customer
    assert bool((degree[:, 1] == c).all()) and bool((degree[:, 2] == 1).all()) and bool((degree[:, 0] == c).all())
    sd = R.make_state_dict("pctsp", 31, 2, 2)
    locs, feats = R.make_instance("pctsp", b, n, 32)
    got = _kernel_run(sd, "pctsp", locs, feats, nbr)
    _compare("hand-made graph", got, _both(sd, locs, feats, nbr), R.on_graph(nbr, n))


# ---- 4. bad input ---------------------------------------------------------------------------------------------------------------
def _stack_inputs(name="c17"):
    sd, locs, feats, nbr, _ = _shape_case(name)
    enc = _module(sd, SHAPES[name][0])
    b, c, k = nbr.shape
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(b, c + 1, 64, generator=gen).cuda()
    w = torch.randn(b, c * (k + 2), 64, generator=gen).cuda()
    p = enc.packed_parameters("cuda")
    layers = list(enc.graph_network.layers)
    bn_w = torch.stack([torch.stack((m.v_bn.module.weight, m.e_bn.module.weight)) for m in layers]).detach().contiguous()
    bn_b = torch.stack([torch.stack((m.v_bn.module.bias, m.e_bn.module.bias)) for m in layers]).detach().contiguous()
    return nbr.to(torch.int32).cuda().contiguous(), x, w, dict(lin_w=p["lin_w"], lin_b=p["lin_b"], bn_w=bn_w, bn_b=bn_b)


def test_bad_neighbour_lists_and_a_wrong_csr_are_refused_through_the_error_word():
    from rl4co_amd import _lib

    K = _K()
    nbr, x, w, p = _stack_inputs()
    n = nbr.shape[1] + 1
    ptr, src = K.depot_incoming_csr(nbr)
    K.nargnn_depot_train_forward(nbr, ptr, src, x, w, **p)  # the good lists pass
    for bad in (0, n, -1):  # the depot as a kNN neighbour, a node of the next instance, a negative index
        broken = nbr.clone()
        broken[1, 7, 3] = bad
        with pytest.raises(AssertionError, match="index out of range"):
            K.nargnn_depot_train_forward(broken, *K.depot_incoming_csr(broken), x, w, **p)
        err = K.new_error_word("cuda")
        K.nargnn_depot_train_forward(broken, ptr, src, x, w, err=err, **p)
        assert int(err.item()) == _lib.EBIT_TOUR_INDEX
    swapped = src.clone()
    swapped[[0, -1]] = src[[-1, 0]]  # a row listed under a node it does not point at
    shifted = ptr.clone()
    shifted[5] += 1
    for bad_ptr, bad_src in ((ptr, swapped), (shifted, src), (ptr, torch.full_like(src, src.numel()))):
        err = K.new_error_word("cuda")
        K.nargnn_depot_train_forward(nbr, bad_ptr, bad_src, x, w, err=err, **p)
        assert int(err.item()) == _lib.EBIT_TOUR_INDEX
        with pytest.raises(AssertionError, match="index out of range"):
            K.nargnn_depot_train_forward(nbr, bad_ptr, bad_src, x, w, **p)
    x_out, w_out, stats, _ = K.nargnn_depot_train_forward(nbr, ptr, src, x, w, **p)  # and the good lists still pass
    assert bool(torch.isfinite(x_out).all()) and bool(torch.isfinite(w_out).all()) and bool(torch.isfinite(stats).all())


# ---- 5. identity of runs, running statistics, eval ------------------------------------------------------------------------------
def test_two_runs_give_identical_bits():
    K = _K()
    nbr, x, w, p = _stack_inputs("k17")
    ptr, src = K.depot_incoming_csr(nbr)
    gen = torch.Generator().manual_seed(5)
    gx, gw = torch.randn(x.shape, generator=gen).cuda(), torch.randn(w.shape, generator=gen).cuda()
    runs = []
    for _ in range(2):
        x_out, w_out, stats, ws = K.nargnn_depot_train_forward(nbr, ptr, src, x, w, **p)
        grads = K.nargnn_depot_train_backward(nbr, ptr, src, x, w, stats=stats, workspace=ws, grad_x_out=gx, grad_w_out=gw, **p)
        runs.append([x_out, w_out, stats] + [grads[key] for key in sorted(grads)])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    sd, locs, feats, nbr64, _ = _shape_case("k17")
    one, two = _kernel_run(sd, "pctsp", locs, feats, nbr64), _kernel_run(sd, "pctsp", locs, feats, nbr64)
    assert all(torch.equal(one[key], two[key]) for key in one)


def test_running_statistics_after_two_forwards():
    sd, locs, feats, nbr, _ = _shape_case("n34")
    enc = _module(sd, "op")
    locs2, feats2 = R.make_instance("op", *locs.shape[:2], 8)
    nbr2, _, _ = R.select_neighbors(locs2.clone(), nbr.shape[2])
    refs = {}
    for dtype in (torch.float32, torch.float64):
        first = T.run(sd, locs, feats, nbr, dtype)
        carried = {**sd, **{key[4:]: value for key, value in first.items() if key.startswith("buf/")}}
        refs[dtype] = T.run(carried, locs2, feats2, nbr2, dtype)
    _kernel_run(sd, "op", locs, feats, nbr, enc=enc)
    got = _kernel_run(sd, "op", locs2, feats2, nbr2, enc=enc)
    pairs = {key: (refs[torch.float32][key], refs[torch.float64][key]) for key in got if key.startswith("buf/")}
    assert all(int(got[key]) == 9 for key in pairs if key.endswith("num_batches_tracked"))  # 7 in the state dict, + 2
    _compare("two forwards", got, pairs, None)


def test_eval_is_the_parent_bit_for_bit():
    from rl4co_amd import NARGNNDepotEncoder

    sd, locs, feats, _, _ = _shape_case("n34")
    enc = _module(sd, "op").eval()
    parent = NARGNNDepotEncoder(env_name="op", num_layers_graph_encoder=2, num_layers_heatmap_generator=2).eval()
    parent.load_state_dict(enc.state_dict(), strict=True)
    td = {key: value.cuda() for key, value in R.td_of("op", locs, feats).items()}
    (heat, embed), (heat0, embed0) = enc(td), parent.cuda()(td)
    assert torch.equal(heat, heat0) and torch.equal(embed, embed0) and not heat.requires_grad and not embed.requires_grad


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", list(R.FEATURES))
def test_nonautoregressive_policy_trains_the_encoder(env):
    from rl4co_amd import NonAutoregressivePolicy, TrainableNARGNNDepotEncoder
    from rl4co_amd.aco import deepaco_loss, heatmap_rollout
    from rl4co_amd.nargnn import _depot_features
    from tests import aco_depot_grad_ref as G

    b, n, ants = 4, 13, 8
    data = G.random_data(env, b, n, 61)
    td = G.as_td(env, data)
    if env == "pctsp":
        td["expected_prize"] = data["prize"][:, 1:].cuda()
    sd = R.make_state_dict(env, 55, 2, 5)
    enc = TrainableNARGNNDepotEncoder(env_name=env, num_layers_graph_encoder=2)
    enc.load_state_dict(sd, strict=True)
    pol = NonAutoregressivePolicy(encoder=enc, env_name=env).cuda().train()
    opt = torch.optim.SGD(pol.parameters(), lr=0.1)
    torch.manual_seed(11)
    out = pol(td, env, phase="train", return_hidden=True, multisample=True, num_samples=ants)
    assert out["hidden"].requires_grad and out["reward"].shape == (ants * b,)

    def loss_of(rolled):
        return deepaco_loss({"reward": rolled["reward"].view(ants, b).t(), "log_likelihood": rolled["log_likelihood"].view(ants, b).t()})

    loss_of(out).backward()
    # the restatement, driven with the same rows: the loss's gradient at ITS heatmap through the same rollout kernels
    locs, feats = td["locs"].cpu(), _depot_features(env, td).cpu()
    nbr = enc.neighbors(td["locs"])[0].cpu().long()
    refs = {}
    for dtype in (torch.float32, torch.float64):
        logits, _, params, _, _ = T.encode_train(sd, locs, feats, dtype=dtype, neighbors=nbr)
        leaf = logits.detach().float().cuda().requires_grad_(True)
        rolled = heatmap_rollout(leaf, td["locs"], n_ants=ants, actions=out["actions"], temperature=pol.temperature,
                                 env_name=env, td=td)
        assert torch.equal(rolled["reward"], out["reward"])
        loss_of(rolled).backward()
        logits.backward(leaf.grad.cpu().to(dtype))
        refs[dtype] = {key: (torch.zeros_like(p) if p.grad is None else p.grad) for key, p in params.items()}
    named = dict(enc.named_parameters())
    got = {key: (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu() for key, p in named.items()}
    _compare(f"policy step, {env}", got, {key: (refs[torch.float32][key], refs[torch.float64][key]) for key in got}, None)
    before = {key: p.detach().clone() for key, p in named.items()}
    opt.step()
    # every GNN parameter whose gradient is not zero in exact arithmetic: the last layer's node update reaches no output
    # (v_lin1, v_lin2 and v_bn there), and a bias directly ahead of a batch norm (v_lin1, v_lin3, v_lin4, e_lin) is a constant
    # the normalisation removes
    dead = tuple(f"graph_network.layers.1.{name}." for name in ("v_lin1", "v_lin2", "v_bn"))
    constant = tuple(f"{name}.bias" for name in ("v_lin1", "v_lin3", "v_lin4", "e_lin"))
    for key, p in named.items():
        if key.startswith("graph_network") and not key.startswith(dead) and not key.endswith(constant):
            assert not torch.equal(p.detach(), before[key]), f"{key} did not move"
