"""DeepACO's heatmap encoder on the MI355X (csrc/nargnn.hip, rl4co_amd.nargnn): the one-launch kernel against the records
of the reference's own NARGNNEncoder, against the float64 restatement (tests/nargnn_ref.py) at the shapes where the kernel
can go wrong, on bad input, and DeepACOPolicy end to end.

Tolerance. Every comparison of logits is against float64 and allows 4 x the fp32 REFERENCE's own distance from float64
(``max |ref32 - ref64|`` over the graph's entries): from the record where there is one, else from the fp32 restatement run
beside the float64 one on the same inputs. The factor covers another summation order in the 64-long dot products, the
folded batch norm and the device's exp / log, all rounding of the same order. Measured ratios (kernel error / floor) are in
DESIGN.md. Entries off the graph equal ``torch.log(torch.tensor(1e-12))`` exactly."""
from functools import lru_cache

import pytest
import torch

from tests import nargnn_ref as R

pytestmark = pytest.mark.gpu
FILL = torch.log(torch.tensor(R.SMALL))


def _K():
    from rl4co_amd import kernels as K

    return K


def _kernel(sd, locs, nbr, **kw):
    cost = (locs[:, :, None, :] - R.gather_nodes(locs, nbr.long())).norm(p=2, dim=-1)
    heat, embed = _K().nargnn_heatmap(locs.cuda(), nbr.to(torch.int32).cuda().contiguous(), cost.cuda().contiguous(),
                                      **R.kernel_parameters(sd), **kw)
    return heat.cpu(), embed.cpu()


def _check_graph(heat, nbr):
    b, n, _ = heat.shape
    on = torch.zeros(b, n, n, dtype=torch.bool).scatter_(2, nbr.long(), True)
    assert torch.equal(heat[~on], FILL.expand(int((~on).sum()))), "an entry off the graph is not the fill constant"
    assert bool(torch.isfinite(heat[on]).all()) and bool((heat[on] > FILL).all())
    return on


# ---- 1. the records ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
def test_records(case):
    rec = R.record(case)
    n = R.CASES[case][0]
    sd = R.case_state_dict(case)
    nbr = R.edge_index_to_neighbors(rec["edge_index"], R.BATCH, n)
    heat, embed = _kernel(sd, rec["locs"], nbr)
    on = _check_graph(heat, nbr)
    floor = R.floor32(rec)
    err = float((heat.double() - rec["heatmap64"])[on].abs().max())
    print(f"{case}: floor {floor:.3e} kernel error {err:.3e} ratio {err / floor:.2f}")
    assert err <= 4 * floor
    # through the module: its own neighbour selection on the device gives the reference's graph
    from rl4co_amd import NARGNNEncoder

    _, k_sparse, layers, mlp_layers, _, _ = R.CASES[case]
    enc = NARGNNEncoder(num_layers_graph_encoder=layers, num_layers_heatmap_generator=mlp_layers, k_sparse=k_sparse).eval()
    enc.load_state_dict(sd, strict=True)
    heat2, embed2 = enc.cuda()({"locs": rec["locs"].cuda()})
    assert torch.equal(torch.isfinite(heat2.cpu()) & (heat2.cpu() != FILL), on)
    assert float((heat2.cpu().double() - rec["heatmap64"])[on].abs().max()) <= 4 * floor
    assert torch.equal(embed2.cpu(), embed)


# ---- 2. seeded shapes against the float64 restatement -------------------------------------------------------------------------
def _lds_nodes(k):
    return _K().nargnn_lds_nodes(k)


# id -> (B, N, K, GNN layers, MLP layers, linear_bias); N None: the LDS tier's last size for K, "+1": one above it
SHAPES = {
    "b1": (1, 24, 10, 2, 2, True), "b3": (3, 24, 10, 2, 2, True), "b67_tails": (67, 13, 5, 1, 2, True),
    "k1": (3, 18, 1, 2, 2, True), "k16": (3, 40, 16, 2, 2, True), "k17": (3, 40, 17, 2, 2, True), "k20": (3, 100, 20, 2, 3, True),
    "lds_last_k10": (2, None, 10, 2, 2, True), "lds_next_k10": (2, "+1", 10, 2, 2, True),
    "lds_last_k20": (2, None, 20, 1, 2, True), "lds_next_k20": (2, "+1", 20, 1, 2, True),
    "n200_k40": (2, 200, 40, 1, 2, True), "n2": (3, 2, 1, 2, 2, True),
    "node_scratch_n301": (1, 301, 10, 1, 2, True), "n1024": (1, 1024, 10, 1, 1, True),
    "no_layers": (3, 24, 10, 0, 3, True), "output_only": (3, 24, 10, 1, 1, True), "no_bias": (3, 24, 10, 2, 3, False),
}


@lru_cache(maxsize=None)
def _shape_case(name):
    b, n, k, layers, mlp_layers, bias = SHAPES[name]
    if n is None:
        n = _lds_nodes(k)
    elif n == "+1":
        n = _lds_nodes(k) + 1
    seed = 1000 + list(SHAPES).index(name)
    sd = R.make_state_dict(seed, layers, mlp_layers, linear_bias=bias)
    locs = torch.rand(b, n, 2, generator=torch.Generator().manual_seed(seed + 500))
    nbr, _ = R.select_neighbors(locs.clone(), k)
    want64, embed64, _, _ = R.encode(sd, locs, dtype=torch.float64, neighbors=nbr, return_edges=True)
    ref32, _ = R.encode(sd, locs, dtype=torch.float32, neighbors=nbr)
    on = torch.zeros(b, n, n, dtype=torch.bool).scatter_(2, nbr, True)
    floor = float((ref32.double() - want64)[on].abs().max())
    return sd, locs, nbr, want64, embed64, on, floor


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name):
    sd, locs, nbr, want64, embed64, on, floor = _shape_case(name)
    heat, embed = _kernel(sd, locs, nbr)
    assert torch.equal(_check_graph(heat, nbr), on)
    err = float((heat.double() - want64)[on].abs().max())
    print(f"{name}: N {locs.shape[1]} floor {floor:.3e} kernel error {err:.3e} ratio {err / floor:.2f}")
    assert err <= 4 * floor
    # node_embed: a two-term dot product and a bias, |terms| <= 1 / sqrt(2) each: three roundings of values below 2
    assert float((embed.double() - embed64).abs().max()) <= 3 * 2.0 ** -23


@pytest.mark.parametrize("name", ["b3", "lds_next_k10"])
def test_neighbour_order_does_not_matter(name):
    sd, locs, nbr, want64, _, on, floor = _shape_case(name)
    g = torch.Generator().manual_seed(5)
    perm = torch.stack([torch.randperm(nbr.shape[2], generator=g) for _ in range(nbr.shape[0] * nbr.shape[1])]).view(nbr.shape)
    heat, _ = _kernel(sd, locs, nbr.gather(2, perm))
    assert torch.equal(_check_graph(heat, nbr), on)
    assert float((heat.double() - want64)[on].abs().max()) <= 4 * floor


def test_grid_stride_and_single_workgroup_agree():
    sd, locs, nbr, _, _, _, _ = _shape_case("b67_tails")
    one, _ = _kernel(sd, locs, nbr, n_workgroups=1)
    five, _ = _kernel(sd, locs, nbr, n_workgroups=5)
    full, _ = _kernel(sd, locs, nbr)
    assert torch.equal(one, five) and torch.equal(one, full)


def test_out_of_range_neighbour_is_refused_through_the_error_word():
    from rl4co_amd import _lib

    sd, locs, nbr, _, _, _, _ = _shape_case("b3")
    K = _K()
    cost = (locs[:, :, None, :] - R.gather_nodes(locs, nbr)).norm(p=2, dim=-1).cuda().contiguous()
    for bad in (locs.shape[1], -1):
        broken = nbr.clone()
        broken[1, 7, 3] = bad
        with pytest.raises(AssertionError, match="index out of range"):
            K.nargnn_heatmap(locs.cuda(), broken.to(torch.int32).cuda(), cost, **R.kernel_parameters(sd))
        err = K.new_error_word("cuda")
        heat, _ = K.nargnn_heatmap(locs.cuda(), broken.to(torch.int32).cuda(), cost, err=err, **R.kernel_parameters(sd))
        assert int(err.item()) == _lib.EBIT_TOUR_INDEX
        good, _ = _kernel(sd, locs, nbr)
        assert torch.equal(heat.cpu()[0], good[0]) and torch.equal(heat.cpu()[2], good[2])  # the other instances are served


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------
def _policy_run(seed):
    from rl4co_amd import DeepACOPolicy
    from rl4co_amd.envs import TSPEnv

    torch.manual_seed(11)
    env = TSPEnv(generator_params=dict(num_loc=20))
    td = env.reset(batch_size=[4])
    pol = DeepACOPolicy(n_ants=8, n_iterations=3, temperature=1.5, num_layers_graph_encoder=3, num_layers_heatmap_generator=2)
    pol.encoder.load_state_dict(R.make_state_dict(77, 3, 2), strict=True)
    pol = pol.eval().cuda()
    torch.manual_seed(seed)
    out = pol(td, env, phase="test")
    return pol, env, td, out


def test_deepaco_policy_end_to_end():
    pol, env, td, out = _policy_run(3)
    assert sorted(out) == ["actions", "reward", "reward_000", "reward_001", "reward_002"]
    actions = out["actions"]
    assert actions.shape == (4, 20) and torch.equal(actions.cpu().sort(1).values, torch.arange(20).expand(4, 20))
    assert torch.equal(out["reward"], env.get_reward(td, actions)) and torch.equal(out["reward"], out["reward_002"])
    assert bool((out["reward_000"] <= out["reward_001"]).all()) and bool((out["reward_001"] <= out["reward_002"]).all())
    heat, _ = pol.encoder(td)
    assert torch.equal(pol.last_aco.log_heuristic, heat / 1.5) and pol.last_aco.n_ants == 8
    _, _, _, again = _policy_run(3)
    assert torch.equal(again["actions"], actions) and torch.equal(again["reward"], out["reward"])
    assert "actions" not in pol(td, env, phase="val", return_actions=False)
    assert len(pol.last_aco.final_reward_cache) == 3
