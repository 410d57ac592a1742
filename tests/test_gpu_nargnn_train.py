"""The trainable heatmap encoder on the MI355X (csrc/nargnn_train.hip, rl4co_amd.TrainableNARGNNEncoder): one train-mode
forward and backward against the records of the reference's own NARGNNEncoder in ``.train()``, against the float64
restatement (tests/nargnn_train_ref.py) at the shapes where the tiling can go wrong, on bad input, for run-to-run identity,
and under DeepACOPolicy end to end.

Tolerance. Per tensor T: ``max |got - ref64| <= 4 max(max |ref32 - ref64|, 2^-23 max |ref64|)`` (``T.bound``): the kernel may
be four times as far from float64 as the fp32 reference itself. ref32 and ref64 come from the record, or from the CPU
restatement run in both dtypes where there is no record; never from kernel output. The heatmap is compared on the graph's
entries (everywhere else both sides hold the fill constant). Measured ratios are in DESIGN.md §4.23."""
from functools import lru_cache

import pytest
import torch

from tests import nargnn_ref as R
from tests import nargnn_train_ref as T

pytestmark = pytest.mark.gpu


def _K():
    from rl4co_amd import kernels as K

    return K


def _module(sd, k_sparse=None, bias=True):
    from rl4co_amd import TrainableNARGNNEncoder

    layers, mlp_layers = R.count_layers(sd)
    enc = TrainableNARGNNEncoder(num_layers_graph_encoder=layers, num_layers_heatmap_generator=mlp_layers, k_sparse=k_sparse,
                                 linear_bias=bias)
    enc.load_state_dict(sd, strict=True)
    return enc.cuda().train()


def _kernel_run(sd, locs, nbr, bias=True, upstream=None, enc=None):
    """tests.nargnn_train_ref.run's dict from the module on the given graph."""
    enc = _module(sd, bias=bias) if enc is None else enc
    locs = locs.cuda()
    nbr = nbr.cuda()
    cost = (locs[:, :, None, :] - R.gather_nodes(locs, nbr.long())).norm(p=2, dim=-1).contiguous()
    logits, embed = enc.encode_train(locs, nbr.to(torch.int32).contiguous(), cost)
    b, n = locs.shape[:2]
    g = T.upstream_grad(b, n) if upstream is None else upstream
    logits.backward((g.cuda() * T.graph_mask(nbr, n)).float())
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


# ---- 1. the records ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(T.CASES))
def test_records(case):
    rec = T.record(case)
    n = T.CASES[case][0]
    sd = T.case_state_dict(case)
    nbr = R.edge_index_to_neighbors(rec["edge_index"], T.BATCH, n)
    got = _kernel_run(sd, rec["locs"], nbr)
    _compare(case, got, T.record_pairs(rec), T.graph_mask(nbr, n))


# ---- 2. seeded shapes against the restatement ---------------------------------------------------------------------------------
# id -> (B, N, K, GNN layers, MLP layers, linear_bias)
SHAPES = {
    "n2": (1, 2, 1, 1, 2, True), "n3": (1, 3, 2, 1, 2, True), "n17": (3, 17, 10, 2, 2, True), "n33": (3, 33, 10, 2, 2, True),
    "k17": (3, 40, 17, 2, 2, True), "k40": (1, 60, 40, 1, 2, True), "b1": (1, 24, 10, 2, 2, True), "b5": (5, 24, 10, 2, 2, True),
    "no_layers": (3, 24, 10, 0, 3, True), "one_layer": (3, 24, 10, 1, 2, True), "no_bias": (3, 24, 10, 2, 3, False),
    "n200_k40": (2, 200, 40, 1, 2, True), "n1024": (1, 1024, 10, 1, 2, True),
}


@lru_cache(maxsize=None)
def _shape_case(name):
    b, n, k, layers, mlp_layers, bias = SHAPES[name]
    seed = 2000 + list(SHAPES).index(name)
    sd = R.make_state_dict(seed, layers, mlp_layers, linear_bias=bias)
    locs = torch.rand(b, n, 2, generator=torch.Generator().manual_seed(seed + 500))
    nbr, _ = R.select_neighbors(locs.clone(), k)
    ref32, ref64 = T.run(sd, locs, nbr, torch.float32), T.run(sd, locs, nbr, torch.float64)
    return sd, locs, nbr, {key: (ref32[key], ref64[key]) for key in ref64}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name):
    sd, locs, nbr, pairs = _shape_case(name)
    got = _kernel_run(sd, locs, nbr, bias=SHAPES[name][5])
    _compare(name, got, pairs, T.graph_mask(nbr, locs.shape[1]))


def test_a_node_nobody_points_to_and_a_node_everybody_points_to():
    b, n, k = 2, 9, 3
    gen = torch.Generator().manual_seed(9)
    nbr = torch.empty(b, n, k, dtype=torch.int64)
    for bb in range(b):
        for i in range(n):
            others = [j for j in range(2, n) if j != i]
            pick = [others[int(t)] for t in torch.randperm(len(others), generator=gen)[:k]]
            nbr[bb, i] = torch.tensor(pick if i == 1 else [1] + pick[:k - 1])
    assert not bool((nbr == 0).any()) and bool(((nbr == 1).sum(2) == 1)[:, [0] + list(range(2, n))].all())
    ptr, _ = _K().incoming_csr(nbr.to(torch.int32).cuda())
    degree = (ptr[1:] - ptr[:-1]).view(b, n).cpu()
    assert bool((degree[:, 0] == 0).all()) and bool((degree[:, 1] == n - 1).all())
    sd = R.make_state_dict(31, 2, 2)
    locs = torch.rand(b, n, 2, generator=gen)
    ref32, ref64 = T.run(sd, locs, nbr, torch.float32), T.run(sd, locs, nbr, torch.float64)
    got = _kernel_run(sd, locs, nbr)
    _compare("hand-made graph", got, {key: (ref32[key], ref64[key]) for key in ref64}, T.graph_mask(nbr, n))


# ---- 3. bad input, identity of runs, running statistics, eval -------------------------------------------------------------------
def _stack_inputs(name="n17"):
    sd, locs, nbr, _ = _shape_case(name)
    enc = _module(sd)
    b, n, k = nbr.shape
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(b, n, 64, generator=gen).cuda()
    w = torch.randn(b, n, k, 64, generator=gen).cuda()
    p = enc.packed_parameters("cuda")
    layers = list(enc.graph_network.layers)
    bn_w = torch.stack([torch.stack((m.v_bn.module.weight, m.e_bn.module.weight)) for m in layers]).detach().contiguous()
    bn_b = torch.stack([torch.stack((m.v_bn.module.bias, m.e_bn.module.bias)) for m in layers]).detach().contiguous()
    return nbr.to(torch.int32).cuda().contiguous(), x, w, dict(lin_w=p["lin_w"], lin_b=p["lin_b"], bn_w=bn_w, bn_b=bn_b)


def test_bad_neighbour_lists_and_a_wrong_csr_are_refused_through_the_error_word():
    from rl4co_amd import _lib

    K = _K()
    nbr, x, w, p = _stack_inputs()
    ptr, src = K.incoming_csr(nbr)
    K.nargnn_train_forward(nbr, ptr, src, x, w, **p)  # the good lists pass
    for bad in (nbr.shape[1], -1):
        broken = nbr.clone()
        broken[1, 7, 3] = bad
        with pytest.raises(AssertionError, match="index out of range"):
            K.nargnn_train_forward(broken, *K.incoming_csr(broken), x, w, **p)
        err = K.new_error_word("cuda")
        K.nargnn_train_forward(broken, ptr, src, x, w, err=err, **p)
        assert int(err.item()) == _lib.EBIT_TOUR_INDEX
    swapped = src.clone()
    swapped[[0, -1]] = src[[-1, 0]]  # an edge listed under a node it does not point at
    shifted = ptr.clone()
    shifted[5] += 1
    for bad_ptr, bad_src in ((ptr, swapped), (shifted, src), (ptr, torch.full_like(src, nbr.numel()))):
        err = K.new_error_word("cuda")
        K.nargnn_train_forward(nbr, bad_ptr, bad_src, x, w, err=err, **p)
        assert int(err.item()) == _lib.EBIT_TOUR_INDEX


def test_two_runs_give_identical_bits():
    K = _K()
    nbr, x, w, p = _stack_inputs("k17")
    ptr, src = K.incoming_csr(nbr)
    gen = torch.Generator().manual_seed(5)
    gx, gw = torch.randn(x.shape, generator=gen).cuda(), torch.randn(w.shape, generator=gen).cuda()
    runs = []
    for _ in range(2):
        x_out, w_out, stats, ws = K.nargnn_train_forward(nbr, ptr, src, x, w, **p)
        grads = K.nargnn_train_backward(nbr, ptr, src, x, w, stats=stats, workspace=ws, grad_x_out=gx, grad_w_out=gw, **p)
        runs.append([x_out, w_out, stats] + [grads[key] for key in sorted(grads)])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    sd, locs, nbr64, _ = _shape_case("k17")
    one, two = _kernel_run(sd, locs, nbr64), _kernel_run(sd, locs, nbr64)
    assert all(torch.equal(one[key], two[key]) for key in one)


def test_running_statistics_after_two_forwards():
    sd, locs, nbr, _ = _shape_case("n33")
    enc = _module(sd)
    locs2 = torch.rand(locs.shape, generator=torch.Generator().manual_seed(8))
    nbr2, _ = R.select_neighbors(locs2.clone(), nbr.shape[2])
    refs = {}
    for dtype in (torch.float32, torch.float64):
        first = T.run(sd, locs, nbr, dtype)
        carried = {**sd, **{key[4:]: value for key, value in first.items() if key.startswith("buf/")}}
        refs[dtype] = T.run(carried, locs2, nbr2, dtype)
    _kernel_run(sd, locs, nbr, enc=enc)
    got = _kernel_run(sd, locs2, nbr2, enc=enc)
    pairs = {key: (refs[torch.float32][key], refs[torch.float64][key]) for key in got if key.startswith("buf/")}
    assert all(int(got[key]) == 9 for key in pairs if key.endswith("num_batches_tracked"))  # 7 in the state dict, + 2
    _compare("two forwards", got, pairs, None)


def test_eval_is_the_parent_bit_for_bit():
    from rl4co_amd import NARGNNEncoder

    sd, locs, _, _ = _shape_case("n33")
    enc = _module(sd).eval()
    parent = NARGNNEncoder(num_layers_graph_encoder=2, num_layers_heatmap_generator=2).eval()
    parent.load_state_dict(enc.state_dict(), strict=True)
    td = {"locs": locs.cuda()}
    (heat, embed), (heat0, embed0) = enc(td), parent.cuda()(td)
    assert torch.equal(heat, heat0) and torch.equal(embed, embed0) and not heat.requires_grad


# ---- 4. end to end --------------------------------------------------------------------------------------------------------------
def test_deepaco_policy_trains_the_encoder():
    from rl4co_amd import DeepACOPolicy, TrainableNARGNNEncoder
    from rl4co_amd.aco import deepaco_loss, heatmap_rollout
    from rl4co_amd.envs import TSPEnv

    torch.manual_seed(11)
    b, n, ants = 4, 12, 8
    env = TSPEnv(generator_params=dict(num_loc=n))
    td = env.reset(batch_size=[b])
    sd = R.make_state_dict(55, 2, 5)
    enc = TrainableNARGNNEncoder(num_layers_graph_encoder=2)
    enc.load_state_dict(sd, strict=True)
    pol = DeepACOPolicy(encoder=enc, n_ants=ants).cuda().train()
    opt = torch.optim.SGD(pol.parameters(), lr=0.1)
    out = pol(td, env, phase="train")
    assert out["hidden"].requires_grad and out["reward"].shape == (b, ants)
    deepaco_loss(out).backward()
    # the restatement, driven with the same tours: the loss's gradient at ITS heatmap through the same rollout kernels
    locs = td["locs"].cpu()
    nbr, _ = enc.neighbors(td["locs"])
    nbr = nbr.cpu().long()
    refs = {}
    for dtype in (torch.float32, torch.float64):
        logits, _, params, _, _ = T.encode_train(sd, locs, dtype=dtype, neighbors=nbr)
        leaf = logits.detach().float().cuda().requires_grad_(True)
        rolled = heatmap_rollout(leaf, td["locs"], n_ants=ants, actions=out["actions"], temperature=pol.temperature)
        assert torch.equal(rolled["reward"], out["reward"].t().reshape(-1))
        view = {"reward": rolled["reward"].view(ants, b).t(), "log_likelihood": rolled["log_likelihood"].view(ants, b).t()}
        deepaco_loss(view).backward()
        logits.backward(leaf.grad.cpu().to(dtype))
        refs[dtype] = {key: (torch.zeros_like(p) if p.grad is None else p.grad) for key, p in params.items()}
    named = dict(enc.named_parameters())
    got = {key: (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu() for key, p in named.items()}
    _compare("policy step", got, {key: (refs[torch.float32][key], refs[torch.float64][key]) for key in got}, None)
    before = {key: p.detach().clone() for key, p in named.items()}
    opt.step()
    # every GNN parameter whose gradient is not zero in exact arithmetic: the last layer's node update reaches no output
    # (v_lin1, v_lin2 and v_bn there), and a bias directly ahead of a batch norm (v_lin1, v_lin3, v_lin4, e_lin) is a constant
    # the normalisation removes; the reference leaves those where they are too
    dead = tuple(f"graph_network.layers.1.{name}." for name in ("v_lin1", "v_lin2", "v_bn"))
    constant = tuple(f"{name}.bias" for name in ("v_lin1", "v_lin3", "v_lin4", "e_lin"))
    for key, p in named.items():
        if key.startswith("graph_network") and not key.startswith(dead) and not key.endswith(constant):
            assert not torch.equal(p.detach(), before[key]), f"{key} did not move"
