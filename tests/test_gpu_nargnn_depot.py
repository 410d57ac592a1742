"""DeepACO's heatmap encoder for the depot graphs of CVRP, OP and PCTSP on the MI355X (csrc/nargnn_depot.hip,
rl4co_amd.nargnn.NARGNNDepotEncoder): the one-launch kernel against the records of the reference's own
NARGNNEncoder(env_name=...), against the float64 restatement (tests/nargnn_depot_ref.py) at the shapes where the kernel can
go wrong, on bad input, and DeepACOPolicy end to end for the three environments.

Tolerance (tests/test_gpu_nargnn.py's rule). Every comparison of logits is against float64 and allows 4 x the fp32
REFERENCE's own distance from float64 (``max |ref32 - ref64|`` over the graph's entries): from the record where there is
one, else from the fp32 restatement run beside the float64 one on the same inputs. Entries off the graph (the diagonal and
heat[0][0] among them) equal ``torch.log(torch.tensor(1e-12))`` exactly. Measured ratios are in DESIGN.md 4.18.
``node_embed`` is a (2 + F)-term dot product and a bias: 2 + F products and as many additions of values below 4 (weights
within 1 / sqrt(2 + F), inputs in [0, 1)), each rounding at most 2^-23, so the bound is 2 (2 + F) 2^-23; the depot's row
has F = 0.

End to end, the returned reward equals ``env.get_reward(td, actions)``. For OP and PCTSP the search's final reward sums
the W-wide row and ``env.get_reward`` the row trimmed to the batch's longest, another association of the same terms that
can differ by one ulp in general (tests/aco_prize_ref.py REWARD_ULPS); on these seeded instances the two
are equal (0 ulps measured, printed before the assertion), and the encoder has no part in that sum."""
from functools import lru_cache

import pytest
import torch

from tests import nargnn_depot_ref as R

pytestmark = pytest.mark.gpu
FILL = torch.log(torch.tensor(R.SMALL))


def _K():
    from rl4co_amd import kernels as K

    return K


def _inputs(locs, feats, nbr):
    dist = R.distances(locs)
    cost = dist[:, 1:].gather(2, nbr.long())
    return (locs.cuda(), feats.cuda().contiguous(), nbr.to(torch.int32).cuda().contiguous(), cost.cuda().contiguous(),
            dist[:, 1:, 0].cuda().contiguous())


def _kernel(sd, locs, feats, nbr, **kw):
    heat, embed = _K().nargnn_depot_heatmap(*_inputs(locs, feats, nbr), **R.kernel_parameters(sd), **kw)
    return heat.cpu(), embed.cpu()


def _check_graph(heat, nbr):
    n = heat.shape[1]
    on = R.on_graph(nbr.long(), n)
    assert torch.equal(heat[~on], FILL.expand(int((~on).sum()))), "an entry off the graph is not the fill constant"
    assert bool(torch.isfinite(heat[on]).all()) and bool((heat[on] > FILL).all())
    # row 0 is on for all customers, column 0 for every customer row; the diagonal and heat[0][0] are fill
    assert bool((heat[:, 0, 1:] > FILL).all()) and bool((heat[:, 1:, 0] > FILL).all())
    assert bool((heat.diagonal(dim1=1, dim2=2) == FILL).all())
    return on


# ---- 1. the records ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
def test_records(case):
    rec = R.record(case)
    env, n, k_sparse, layers, mlp_layers, _, _ = R.CASES[case]
    sd = R.case_state_dict(case)
    nbr = R.edge_index_to_neighbors(rec["edge_index"], R.BATCH, n)
    heat, embed = _kernel(sd, rec["locs"], rec["feats"], nbr)
    on = _check_graph(heat, nbr)
    floor = R.floor32(rec)
    err = float((heat.double() - rec["heatmap64"])[on].abs().max())
    print(f"{case}: floor {floor:.3e} kernel error {err:.3e} ratio {err / floor:.2f}")
    assert err <= 4 * floor
    assert float((embed - rec["node_embed32"]).abs().max()) <= 2 * (2 + R.FEATURES[env]) * 2.0 ** -23
    # through the module: its own neighbour selection on the device gives the reference's graph
    from rl4co_amd import NARGNNDepotEncoder

    enc = NARGNNDepotEncoder(env_name=env, num_layers_graph_encoder=layers, num_layers_heatmap_generator=mlp_layers,
                             k_sparse=k_sparse).eval()
    enc.load_state_dict(sd, strict=True)
    td = {k: v.cuda() for k, v in R.td_of(env, rec["locs"], rec["feats"]).items()}
    heat2, embed2 = enc.cuda()(td)
    assert heat2.shape == (R.BATCH, n, n) and embed2.shape == (R.BATCH, n, 64)
    assert torch.equal(torch.isfinite(heat2.cpu()) & (heat2.cpu() != FILL), on)
    assert float((heat2.cpu().double() - rec["heatmap64"])[on].abs().max()) <= 4 * floor
    assert torch.equal(embed2.cpu(), embed)


# ---- 2. seeded shapes against the float64 restatement -------------------------------------------------------------------------
def _lds_nodes(k):
    return _K().nargnn_depot_lds_nodes(k)


# id -> (env, B, N, K, GNN layers, MLP layers, linear_bias); N None: the LDS tier's last size for K, "+1": one above it
SHAPES = {
    "n3": ("cvrp", 3, 3, 1, 2, 2, True), "n4": ("pctsp", 3, 4, 2, 2, 2, True),
    "b1": ("cvrp", 1, 14, 5, 2, 2, True), "b3": ("pctsp", 3, 14, 5, 2, 2, True), "b67_tails": ("op", 67, 14, 5, 1, 2, True),
    "k14_stride15": ("cvrp", 2, 40, 14, 2, 2, True), "k15_stride16": ("op", 2, 40, 15, 2, 2, True),
    "k16_stride17": ("pctsp", 2, 40, 16, 2, 2, True),
    "c15": ("cvrp", 2, 16, 3, 2, 2, True), "c16": ("pctsp", 2, 17, 3, 2, 2, True), "c17": ("op", 2, 18, 3, 2, 2, True),
    "c21_waves": ("cvrp", 2, 22, 4, 2, 3, True),
    "lds_last_k10": ("cvrp", 2, None, 10, 2, 2, True), "lds_next_k10": ("pctsp", 2, "+1", 10, 2, 2, True),
    "lds_last_k20": ("op", 2, None, 20, 1, 2, True), "lds_next_k20": ("cvrp", 2, "+1", 20, 1, 2, True),
    "node_scratch_n301": ("pctsp", 1, 301, 10, 1, 2, True), "n1024_depot_mean": ("cvrp", 1, 1024, 10, 1, 1, True),
    "n200_k40": ("op", 2, 200, 40, 1, 2, True),
    "no_layers": ("cvrp", 3, 24, 10, 0, 3, True), "output_only": ("pctsp", 3, 24, 10, 1, 1, True),
    "no_bias": ("op", 3, 24, 10, 2, 3, False),
}


@lru_cache(maxsize=None)
def _shape_case(name):
    env, b, n, k, layers, mlp_layers, bias = SHAPES[name]
    if n is None:
        n = _lds_nodes(k)
    elif n == "+1":
        n = _lds_nodes(k) + 1
    seed = 2000 + list(SHAPES).index(name)
    sd = R.make_state_dict(env, seed, layers, mlp_layers, linear_bias=bias)
    locs, feats = R.make_instance(env, b, n, seed + 500)
    nbr, _, _ = R.select_neighbors(locs, k)
    want64, embed64 = R.encode(sd, locs, feats, dtype=torch.float64, neighbors=nbr)
    ref32, _ = R.encode(sd, locs, feats, dtype=torch.float32, neighbors=nbr)
    on = R.on_graph(nbr, n)
    floor = float((ref32.double() - want64)[on].abs().max())
    return env, sd, locs, feats, nbr, want64, embed64, on, floor


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name):
    env, sd, locs, feats, nbr, want64, embed64, on, floor = _shape_case(name)
    heat, embed = _kernel(sd, locs, feats, nbr)
    assert torch.equal(_check_graph(heat, nbr), on)
    err = float((heat.double() - want64)[on].abs().max())
    print(f"{name}: {env} N {locs.shape[1]} K {nbr.shape[2]} floor {floor:.3e} kernel error {err:.3e} ratio {err / floor:.2f}")
    assert err <= 4 * floor
    assert float((embed.double() - embed64).abs().max()) <= 2 * (2 + R.FEATURES[env]) * 2.0 ** -23


@pytest.mark.parametrize("name", ["b3", "lds_next_k10"])
def test_neighbour_order_does_not_matter(name):
    _, sd, locs, feats, nbr, want64, _, on, floor = _shape_case(name)
    g = torch.Generator().manual_seed(5)
    perm = torch.stack([torch.randperm(nbr.shape[2], generator=g) for _ in range(nbr.shape[0] * nbr.shape[1])]).view(nbr.shape)
    heat, _ = _kernel(sd, locs, feats, nbr.gather(2, perm))
    assert torch.equal(_check_graph(heat, nbr), on)
    assert float((heat.double() - want64)[on].abs().max()) <= 4 * floor


def test_grid_stride_and_single_workgroup_agree():
    _, sd, locs, feats, nbr, _, _, _, _ = _shape_case("b67_tails")
    one, e1 = _kernel(sd, locs, feats, nbr, n_workgroups=1)
    five, e5 = _kernel(sd, locs, feats, nbr, n_workgroups=5)
    full, ef = _kernel(sd, locs, feats, nbr)
    assert torch.equal(one, five) and torch.equal(one, full) and torch.equal(e1, e5) and torch.equal(e1, ef)


def test_bad_neighbour_is_refused_through_the_error_word():
    from rl4co_amd import _lib

    _, sd, locs, feats, nbr, _, _, _, _ = _shape_case("b3")
    K = _K()
    good, _ = _kernel(sd, locs, feats, nbr)
    for bad in (locs.shape[1], -1, 0):  # 0, the depot, would repeat the depot edge
        broken = nbr.clone()
        broken[1, 7, 3] = bad
        args = _inputs(locs, feats, nbr)
        args = args[:2] + (broken.to(torch.int32).cuda(),) + args[3:]
        with pytest.raises(AssertionError, match="index out of range"):
            K.nargnn_depot_heatmap(*args, **R.kernel_parameters(sd))
        err = K.new_error_word("cuda")
        heat, _ = K.nargnn_depot_heatmap(*args, err=err, **R.kernel_parameters(sd))
        assert int(err.item()) == _lib.EBIT_TOUR_INDEX
        assert torch.equal(heat.cpu()[0], good[0]) and torch.equal(heat.cpu()[2], good[2])  # the other instances are served


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------
def _policy_run(env_name, seed, multistart=False):
    from rl4co_amd import DeepACOPolicy
    from rl4co_amd.envs import get_env

    torch.manual_seed(11)
    env = get_env(env_name, generator_params=dict(num_loc=19))  # 20 nodes with the depot
    td = env.reset(batch_size=[4])
    pol = DeepACOPolicy(env_name=env_name, n_ants=8, n_iterations=3, temperature=1.5, multistart=multistart,
                        num_layers_graph_encoder=3, num_layers_heatmap_generator=2)
    pol.encoder.load_state_dict(R.make_state_dict(env_name, 77, 3, 2), strict=True)
    pol = pol.eval().cuda()
    torch.manual_seed(seed)
    out = pol(td, env, phase="test")
    return pol, env, td, out


@pytest.mark.parametrize("env_name,multistart", [("cvrp", False), ("cvrp", True), ("op", False), ("pctsp", False)])
def test_deepaco_policy_end_to_end(env_name, multistart):
    from rl4co_amd import NARGNNDepotEncoder

    pol, env, td, out = _policy_run(env_name, 3, multistart)
    assert type(pol.encoder) is NARGNNDepotEncoder
    assert sorted(out) == ["actions", "reward", "reward_000", "reward_001", "reward_002"]
    actions = out["actions"]
    assert actions.shape[0] == 4 and torch.equal(out["reward"], out["reward_002"])
    env.check_solution_validity(td, actions)
    got = env.get_reward(td, actions)
    if env_name != "cvrp":
        from tests import aco_prize_ref as P

        data = {"locs": td["locs"].cpu(), "prize": td["prize" if env_name == "op" else "real_prize"].cpu()}
        data["max_length" if env_name == "op" else "penalty"] = td["max_length" if env_name == "op" else "penalty"].cpu()
        off = float(P.ulps(out["reward"].cpu(), got.cpu(), P.reward_scale(env_name, data, actions.cpu())).max())
        print(f"{env_name}: reward off env.get_reward on the returned actions by {off} ulps (bound {P.REWARD_ULPS})")
    assert torch.equal(out["reward"], got)
    assert bool((out["reward_000"] <= out["reward_001"]).all()) and bool((out["reward_001"] <= out["reward_002"]).all())
    heat, embed = pol.encoder(td)
    assert heat.shape == (4, 20, 20) and embed.shape == (4, 20, 64)
    assert torch.equal(pol.last_aco.log_heuristic, heat / 1.5) and pol.last_aco.n_ants == 8
    _, _, _, again = _policy_run(env_name, 3, multistart)
    assert torch.equal(again["actions"], actions) and torch.equal(again["reward"], out["reward"])
