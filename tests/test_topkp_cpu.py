"""CPU checks of the top-k / top-p (nucleus) decoding filter's host side: argument handling as the reference's
process_logits (utils/decoding.py:138-188), the decode arguments the binding fills, and the float64 checker the GPU tests
use (tests/topkp_ref.py), pinned to the reference's own process_logits through a recorded run."""
import ctypes

import pytest
import torch

from tests.helpers import reference_record
from tests.topkp_ref import filter_f64, process_logits_f64, unpack_bits


def test_decoding_filter_arguments_as_the_reference():
    from rl4co_amd.kernels import decoding_filter

    assert decoding_filter(0, 0.0, 50) == (0, 0.0)      # neutral values
    assert decoding_filter(None, None, 50) == (0, 0.0)
    assert decoding_filter(-3, -0.5, 50) == (0, 0.0)    # top_k <= 0, top_p <= 0: off
    assert decoding_filter(5, 0.9, 50) == (5, pytest.approx(0.9))
    assert decoding_filter(50, 1.0, 50) == (0, 0.0)     # k clamped to N removes nothing; p = 1 is a no-op
    assert decoding_filter(55, 0.0, 50) == (0, 0.0)
    with pytest.raises(AssertionError, match="top-p should be in"):
        decoding_filter(0, 1.5, 50)


def test_parse_decoding_accepts_the_filter():
    from oracle import reference_torch as R
    from rl4co_amd.policy import AttentionModelPolicy

    torch.manual_seed(0)
    pol = AttentionModelPolicy("tsp")
    env = R.get_env("tsp", 10)
    td = env.reset(env.generate(2))
    kw = dict(decode_type="sampling", top_k=5, top_p=0.8)
    opt = pol._parse_decoding(td, env, "test", None, kw)
    assert (opt.top_k, opt.top_p) == (5, pytest.approx(0.8)) and kw == {}
    opt = pol._parse_decoding(td, env, "test", None, dict(decode_type="greedy"))
    assert (opt.top_k, opt.top_p) == (0, 0.0)
    with pytest.raises(AssertionError, match="top-p should be in"):
        pol._parse_decoding(td, env, "test", None, dict(decode_type="sampling", top_p=1.01))
    with pytest.raises(NotImplementedError):
        pol._parse_decoding(td, env, "test", None, dict(decode_type="sampling", softmax_temp=0.5))


def test_decode_args_carry_the_filter():
    from rl4co_amd import _lib

    a = _lib.AmDecodeArgs()
    assert (a.top_k, a.top_p, a.kept_bits, a.kept_words) == (0, 0.0, None, 0)  # zero-initialised: no filter
    names = [f[0] for f in _lib.AmDecodeArgs._fields_]
    assert names[-5:] == ["top_k", "top_p", "kept_bits", "kept_words", "reserved1"]
    assert ctypes.sizeof(_lib.AmDecodeArgs) % 8 == 0
    assert _lib.AmDecodeArgs.top_k.offset == _lib.AmDecodeArgs.ctx_batch_stride.offset + 8


def _rows():
    """Processed-logit rows with masks, temperature, saturated-tanh ties at the k-th value and at the top-p cut."""
    g = torch.Generator().manual_seed(7)
    n = 24
    logits = torch.randn(6, n, generator=g, dtype=torch.float64) * 3.0
    mask = torch.rand(6, n, generator=g) > 0.25
    mask[:, 0] = True
    logits[1, :6] = 40.0   # tanh saturates: six exact ties at the top (k-th value inside the tie group)
    logits[2, :] = 0.5     # all equal: the top-p cut falls inside one tie group
    logits[3, 3:9] = -40.0  # ties at the bottom
    return logits.float(), mask


CASES = [(0, 0.0, 1.0), (5, 0.0, 1.0), (3, 0.0, 1.0), (40, 0.0, 1.0), (0, 0.5, 1.0), (0, 0.9, 1.0), (0, 1.0, 1.0),
         (10, 0.8, 0.7), (4, 0.9, 2.0)]


@pytest.mark.parametrize("top_k,top_p,temp", CASES)
def test_f64_checker_matches_reference_process_logits(top_k, top_p, temp):
    logits, mask = _rows()

    def reference():
        from oracle import ref_import

        ns = ref_import.load()
        return {"logp": ns.decoding.process_logits(logits.double().clone(), mask.clone(), temperature=temp, top_p=top_p,
                                                   top_k=top_k, tanh_clipping=10.0, mask_logits=True)}

    theirs = reference_record(f"topkp_process_logits_k{top_k}_p{top_p}_t{temp}", reference)["logp"]
    ours = process_logits_f64(logits, mask, temperature=temp, top_p=top_p, top_k=top_k, tanh_clipping=10.0)
    z = (torch.tanh(logits.double()) * 10.0).masked_fill(~mask, float("-inf")) / temp
    for r in range(z.shape[0]):
        ko, kt = ~torch.isinf(ours[r]), ~torch.isinf(theirs[r])
        if not torch.equal(ko, kt):
            # the reference sorts with torch.sort(stable=False): which members of a tie group at the top-p cut survive is
            # its sort's choice; the product's contract is the stable order. Same count, and only inside one tie group
            diff = ko ^ kt
            assert ko.sum() == kt.sum() and z[r][diff].unique().numel() == 1, r
            continue
        torch.testing.assert_close(ours[r][ko], theirs[r][kt], rtol=1e-12, atol=1e-12)


def test_f64_checker_tie_rules():
    z = torch.tensor([[1.0, 3.0, 3.0, 2.0, 3.0, float("-inf")]], dtype=torch.float64)
    assert filter_f64(z, 2).tolist() == [[False, True, True, False, True, False]]  # every tie at the k-th value kept
    assert filter_f64(z, 9).tolist() == [[True] * 5 + [False]]                      # k > F: nothing removed
    zt = torch.zeros(1, 4, dtype=torch.float64)  # equal mass: stable ascending order, the highest positions survive
    assert filter_f64(zt, 0, 0.5).tolist() == [[False, False, True, True]]


def test_unpack_bits_layout():
    bits = torch.tensor([[0b101, 0, 1, 0]], dtype=torch.int32)  # nodes 0, 2 and 64
    got = unpack_bits(bits, 70)[0].nonzero().flatten().tolist()
    assert got == [0, 2, 64]


@pytest.mark.parametrize("case", ["k5", "p0.9", "k10_p0.8_t0.7", "greedy_p0.5", "sampling_eval"])
@pytest.mark.parametrize("env_name", ["tsp", "cvrp"])
def test_reference_rollouts_with_a_filter_are_recorded(env_name, case):
    """The reference rollouts tests/test_gpu_topkp.py compares the policy with (TSP-50 / CVRP-50 x 64, fp32, seeded): the
    record holds whole batches, TSP permutations and finite log-likelihoods."""
    from tests.topkp_ref import rollout_record

    rec = rollout_record(env_name, 50, 64, case)
    a, ll = rec["actions"], rec["log_likelihood"]
    assert a.shape[0] == 64 and torch.isfinite(ll).all() and (ll <= 0).all()
    if env_name == "tsp":
        assert torch.equal(a.sort(1).values, torch.arange(50).expand(64, 50))
