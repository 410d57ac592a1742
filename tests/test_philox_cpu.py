"""Pins the in-kernel noise generator (rl4co_philox4x32 / rl4co_exp1_noise of rl4co_amd/csrc/rl4co_math.h) without a GPU.

The C oracle includes the product header, so "HIP == C oracle bit for bit" cannot see an error in the rounds, the constants
or the counter layout. Here (1) the numpy restatement (tests/philox_ref.py) and the header's raw block both reproduce the
published Random123 known answers of philox4x32-10, (2) the header's Exp(1) draw equals the restatement's bit for bit over
a sweep of seeds, steps, trajectories and nodes that reaches every word of counter and key, and (3) the stream AS THE ANT
SYSTEM KERNELS INDEX IT (tests/philox_ref.py's builders; tests/test_gpu_aco_philox.py ties the kernels to them bit for bit)
selects nodes with the stated probabilities, independently across ants and across iterations."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

from oracle import c_oracle
from tests import aco_ref as R
from tests import philox_ref as P

# ---- 1. known answers ------------------------------------------------------------------------------------------------------
# Random123's kat_vectors for philox4x32, 10 rounds: (counter, key, result)
KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_restatement_reproduces_the_published_vectors(counter, key, want):
    assert tuple(int(w) for w in P.philox4x32(list(counter), list(key))) == want


def test_restatement_is_vectorised_over_counters_and_keys():
    got = P.philox4x32(np.array([k[0] for k in KAT], dtype=np.uint64), np.array([k[1] for k in KAT], dtype=np.uint64))
    assert got.dtype == np.uint32 and got.shape == (3, 4)
    assert [tuple(int(w) for w in row) for row in got] == [k[2] for k in KAT]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_header_reproduces_the_published_vectors(counter, key, want):
    c = (C.c_uint32 * 4)(*counter)
    c_oracle.lib().oracle_philox4x32(c, key[0], key[1])
    assert tuple(c) == want


# ---- 2. the header's draw equals the restatement's ---------------------------------------------------------------------------
SEEDS = (0, 1, 0x1234ABCD5678, 2**62 - 1, 0x8000000000000001, 2**64 - 1, 0xDEADBEEF00000000, 0x00000000FFFFFFFF, 2**32)
STEPS = (0, 1, 7, 2**31, 2**32 - 1, 2**32, 2**32 + 5, 0x0123456789ABCDEF, 2**64 - 1)
TRAJS = (0, 1, 2, 47, 4095, 2**31 - 1, 2**31, 2**32 - 1)
NODES = tuple(range(12)) + (63, 64, 65, 66, 127, 128, 129, 130, 139, 140, 141, 142) + tuple(range(1016, 1024))


def test_header_noise_equals_the_restatement_bit_for_bit():
    seed, step, traj, node = (np.array(x, dtype=np.uint64) for x in (SEEDS, STEPS, TRAJS, NODES))
    grid = [g.reshape(-1) for g in np.meshgrid(seed, step, traj, node, indexing="ij")]
    assert grid[0].size >= 20000 and {int(n) & 3 for n in NODES} == {0, 1, 2, 3} and max(NODES) == 1023
    # a random part on top of the grid: every bit of every word moves
    rng = np.random.default_rng(20260)
    rand = [rng.integers(0, 2**64, 8192, dtype=np.uint64), rng.integers(0, 2**64, 8192, dtype=np.uint64),
            rng.integers(0, 2**32, 8192, dtype=np.uint64), rng.integers(0, 1024, 8192, dtype=np.uint64)]
    seed, step, traj, node = (np.concatenate((g, r)) for g, r in zip(grid, rand))
    want = P.exp1(seed, step, traj, node)
    fn = c_oracle.lib().oracle_exp1_noise
    got = torch.tensor([fn(int(s), int(t), int(r), int(n)) for s, t, r, n in zip(seed, step, traj, node)], dtype=torch.float32)
    assert bool((want > 0).all()) and bool(torch.isfinite(want).all())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # and the logarithm of it, the word the Ant System kernels use
    assert torch.equal(c_oracle.math_array("log", got).view(torch.int32), P.ln_exp1(seed, step, traj, node).view(torch.int32))


def test_stream_builders_index_as_the_headers_state():
    seed, offset, iters, n, rows = 0x1234ABCD5678, 2**32 - 3, 2, 7, 5
    fn, log = c_oracle.lib().oracle_exp1_noise, lambda x: float(c_oracle.math_array("log", torch.tensor([x])))
    tsp = P.tsp_stream(seed, offset, iters, n, rows)
    assert tsp.shape == (iters, n - 1, rows, n) and tsp.dtype == torch.float32 and tsp.is_contiguous()
    w = P.cvrp_width(n)
    cvrp = P.cvrp_stream(seed, offset, iters, n, rows)
    assert w == 11 and P.cvrp_width(3) == 3 and cvrp.shape == (iters, w, rows, n) and cvrp.is_contiguous()
    for it, t, row, node in ((0, 1, 0, 0), (1, 1, 0, 0), (1, 6, 4, 6), (0, 3, 2, 5), (1, 2, 3, 4)):
        assert float(tsp[it, t - 1, row, node]) == log(fn(seed, offset + it * n + t, row, node))
        assert float(cvrp[it, t, row, node]) == log(fn(seed, offset + it * w + t, row, node))
    assert float(cvrp[1, 0, 1, 2]) == log(fn(seed, offset + w, 1, 2))


# ---- 3. independence of the stream as the kernels index it ------------------------------------------------------------------
N, ROWS, ITERS = 6, 4096, 2
P_TAIL = 1e-4  # every statistic must lie below the upper 1e-4 quantile of its chi-square law


def _chi2_cap(df: int) -> float:
    try:
        from scipy.stats import chi2

        return float(chi2.isf(P_TAIL, df))
    except ImportError:  # Wilson-Hilferty: chi2_df ~ df * (1 - 2 / (9 df) + z * sqrt(2 / (9 df)))^3, z the normal quantile
        z = 3.719016485455709  # the upper 1e-4 quantile of the standard normal law
        return df * (1.0 - 2.0 / (9.0 * df) + z * (2.0 / (9.0 * df)) ** 0.5) ** 3


@lru_cache(maxsize=None)
def _step_one():
    """One instance, N = 6, a fixed non-uniform pheromone, every ant on node 0: the log-probs of step t = 1."""
    locs = torch.tensor([[[0.50, 0.50], [0.10, 0.20], [0.90, 0.30], [0.35, 0.95], [0.80, 0.85], [0.20, 0.60]]])
    phe = torch.tensor([1.0, 0.6, 1.7, 0.9, 2.2, 0.5]).repeat(1, N, 1)
    visited = torch.zeros(N, dtype=torch.bool)
    visited[0] = True
    lp = R.step_logps(R.logits(phe, R.heuristic(locs), 1.0, 1.0)[0, 0], visited)
    p = lp[1:].double().exp()
    # the chi-square laws need every expected cell well above 5: 2048 * p_i * p_j in the 5 x 5 tables
    assert abs(float(p.sum()) - 1) < 1e-6 and float(p.min()) > 0.08 and float(p.max() / p.min()) > 2
    return lp, visited, p.numpy()


def _choices(stream: torch.Tensor) -> np.ndarray:
    """stream [ITERS, >= 1, ROWS, N] -> the node (1 .. 5) ant r takes at step 1 of iteration it, [ITERS, ROWS]."""
    lp, visited, _ = _step_one()
    return np.array([[R.select(lp, stream[it, 0, r], visited) for r in range(ROWS)] for it in range(ITERS)])


def _fit(counts: np.ndarray, expected: np.ndarray) -> float:
    return float(((counts - expected) ** 2 / expected).sum())


def _contingency(x: np.ndarray, y: np.ndarray) -> float:
    """Pearson's statistic of the 5 x 5 table of (x, y) against the product of its margins: df 16."""
    table = np.zeros((N - 1, N - 1))
    np.add.at(table, (x - 1, y - 1), 1)
    expected = table.sum(1, keepdims=True) * table.sum(0, keepdims=True) / table.sum()
    return _fit(table, expected)


def _statistics(stream: torch.Tensor) -> dict:
    ch = _choices(stream)
    p = _step_one()[2]
    return {
        "a": _fit(np.bincount(ch[0] - 1, minlength=N - 1).astype(np.float64), ROWS * p),  # df 4
        "b": _contingency(ch[0, 0::2], ch[0, 1::2]),            # ants (2 k, 2 k + 1), df 16
        "c": _contingency(ch[0], ch[1]),                        # the same ant, iteration 0 against iteration 1, df 16
        "d": _contingency(ch[0, : ROWS // 2], ch[0, ROWS // 2 :]),  # ants (r, r + 2048), df 16
    }


CAPS = {"a": _chi2_cap(4), "b": _chi2_cap(16), "c": _chi2_cap(16), "d": _chi2_cap(16)}  # 23.51, 45.92, 45.92, 45.92


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_stream_selects_with_the_stated_probabilities_independently(seed):
    """(a) the counts of iteration 0 against 4096 exp(lp); (b) neighbouring ants; (c) the same ant in two iterations;
    (d), added to the three the check was specified with, ants half the colony apart: the pairing in which a trajectory
    word that wraps at 2048 shows (see the self-test below).

    Observed on the CPU (the stream is host arithmetic and deterministic), against the caps 23.51 / 45.92 / 45.92 / 45.92:
      seed 1: a 2.75  b 12.09  c 22.83  d 14.44
      seed 2: a 7.90  b 13.88  c 18.93  d 15.18
      seed 3: a 4.98  b 13.99  c 12.00  d 19.64
    A correct stream exceeds one of its caps with probability 1e-4 each."""
    stats = _statistics(P.tsp_stream(seed, 0, ITERS, N, ROWS)[:, :1])
    print(f"seed {seed}: " + "  ".join(f"{k} {v:.2f} (cap {CAPS[k]:.2f})" for k, v in stats.items()))
    for k, v in stats.items():  # observed: a 2.75 7.90 4.98, b 12.09 13.88 13.99, c 22.83 18.93 12.00, d 14.44 15.18 19.64
        assert v < CAPS[k], (k, v, CAPS[k])


def _broken_stream(seed, row_of, per_iteration):
    """The TSP stream of step t = 1 with another trajectory word (row_of(r)) or another iteration stride."""
    it = np.arange(ITERS, dtype=np.uint64).reshape(-1, 1, 1, 1)
    row = row_of(np.arange(ROWS, dtype=np.uint64)).reshape(1, 1, -1, 1)
    node = np.arange(N, dtype=np.uint64).reshape(1, 1, 1, -1)
    return P.ln_exp1(seed, it * np.uint64(per_iteration) + np.uint64(1), row, node)


def test_the_check_rejects_deliberately_broken_streams():
    """The check has teeth. Observed statistics (seed 1), caps as above:
      trajectory r % 2048 (ants r and r + 2048 share their noise):  a 7.00  b 23.77  c 35.26  d 8192.00
      trajectory r // 2   (ants 2 k and 2 k + 1 share their noise): b 8192.00
      no it * N in the step (every iteration replays the noise):    c 16384.00
    With the trajectory r % 2048 the pairs (2 k, 2 k + 1) and (ant, same ant one iteration on) still have distinct counter
    words, so (b) and (c) see 2048 independent pairs counted twice and cannot reject by construction; (d) pairs exactly
    the ants that share a word. (b)'s own teeth are shown on the stream whose neighbours share a word."""
    ok = _statistics(_broken_stream(1, lambda r: r, N))  # the helper itself restates the correct stream
    want = _statistics(P.tsp_stream(1, 0, ITERS, N, ROWS)[:, :1])
    assert ok == want
    wrapped = _statistics(_broken_stream(1, lambda r: r % np.uint64(ROWS // 2), N))
    halved = _statistics(_broken_stream(1, lambda r: r // np.uint64(2), N))
    replayed = _statistics(_broken_stream(1, lambda r: r, 0))
    print("wrapped", wrapped, "halved b", halved["b"], "replayed c", replayed["c"])
    assert wrapped["b"] > CAPS["b"] or wrapped["c"] > CAPS["c"] or wrapped["d"] > CAPS["d"]
    assert wrapped["d"] > CAPS["d"]  # identical choices: the table is diagonal, the statistic 4 * 2048
    assert halved["b"] > CAPS["b"]
    assert replayed["c"] > CAPS["c"]
