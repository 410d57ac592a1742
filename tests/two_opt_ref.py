"""TSP 2-opt local search: (a) a vectorised CPU restatement of the reference's best-improvement 2-opt
(envs/routing/tsp/local_search.py:16-81) — every pair's ``change`` in fp32 with the reference's association, the first
minimum in ``(i, j)`` order, the move threshold compared in double as numba does — and (b) the recorder that runs the
reference's own ``local_search.py`` (through oracle/ref_import.py, with a stand-in ``numba`` that runs the functions as
plain Python) and writes ``tests/golden/reference/two_opt_<case>.npz``. Helper of tests/test_two_opt_cpu.py and
tests/test_gpu_two_opt.py; not collected."""
import numpy as np
import torch

THRESHOLD = -1e-6  # a Python float: compared in double


# ---- (a) the restatement ---------------------------------------------------------------------------------------------
def distance_matrix(locs: torch.Tensor) -> torch.Tensor:
    """utils/ops.py:93-100 on the CPU: ATen's norm(p=2) over the two coordinates. [B, N, 2] -> [B, N, N]"""
    locs = locs.detach().cpu().float()
    return (locs[..., :, None, :] - locs[..., None, :, :]).norm(p=2, dim=-1)


def with_diagonal(distances) -> np.ndarray:
    """local_search.py:38: 1e9 added on the diagonal, in fp32. [B, N, N]"""
    d = np.asarray(distances.detach().cpu().numpy() if torch.is_tensor(distances) else distances, dtype=np.float32)
    return d + np.float32(1e9) * np.eye(d.shape[1], dtype=np.float32)[None, :, :]


def pair_list(t: int):
    """The pairs 1 <= i < j <= t - 1, i ascending then j ascending (the order of the reference's two loops)."""
    i, j = np.triu_indices(t, 1)
    keep = i >= 1
    return i[keep], j[keep]


def best_move(d: np.ndarray, tour: np.ndarray, pairs):
    """One scan: (change, i, j) of the first pair of the smallest ``change`` below 0, or None. ``d`` [N, N] fp32 with
    its diagonal, ``tour`` [T] integers."""
    i, j = pairs
    if i.size == 0:
        return None
    t = tour.shape[0]
    ni, nj, prev, nxt = tour[i], tour[j], tour[i - 1], tour[(j + 1) % t]
    with np.errstate(invalid="ignore"):
        change = ((d[prev, nj] + d[ni, nxt]) - d[prev, ni]) - d[nj, nxt]  # fp32 arrays: one rounding per operation
        assert change.dtype == np.float32
        ok = (prev != nj) & (nxt != ni) & (change < np.float32(0))  # NaN and -0.0 are not below 0
    if not ok.any():
        return None
    k = int(np.argmin(np.where(ok, change, np.float32(np.inf))))  # argmin: the FIRST minimum
    return change[k], int(i[k]), int(j[k])


def two_opt(distances, tours, max_iterations: int = 1000):
    """``distances`` [B, N, N] fp32 (WITHOUT the 1e9 diagonal: it is added here, as local_search does), ``tours`` [B, T]
    -> (tours int64 [B, T], iterations int32 [B]) as torch tensors."""
    d = with_diagonal(distances)
    tours = np.array(tours.detach().cpu().numpy() if torch.is_tensor(tours) else tours, dtype=np.int64)
    pairs = pair_list(tours.shape[1])
    iters = np.zeros(tours.shape[0], dtype=np.int32)
    for b, tour in enumerate(tours):
        it, min_change = 0, -1.0
        while min_change < THRESHOLD and it < max_iterations:
            move = best_move(d[b], tour, pairs)
            if move is not None and float(move[0]) < THRESHOLD:  # float(): the fp32 value widened to double
                tour[move[1] : move[2] + 1] = tour[move[1] : move[2] + 1][::-1].copy()
                min_change = float(move[0])
            else:
                min_change = 0.0
            it += 1
        iters[b] = it
    return torch.from_numpy(tours), torch.from_numpy(iters)


def tour_length64(distances, tours) -> torch.Tensor:
    """Closed tour length in float64 over the given matrix [B, N, N] (no diagonal involved for a permutation)."""
    d = torch.as_tensor(distances).detach().cpu().double()
    t = torch.as_tensor(tours).detach().cpu().long()
    rows = torch.arange(t.shape[0])[:, None]
    return d[rows, t, t.roll(-1, dims=1)].sum(1)


def random_tours(b: int, n: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(n, generator=g) for _ in range(b)])


def random_locs(b: int, n: int, seed: int) -> torch.Tensor:
    return torch.rand(b, n, 2, generator=torch.Generator().manual_seed(seed))


# ---- (b) the recorder (needs the reference checkout) -------------------------------------------------------------------
# case -> (kind, batch, nodes, max_iterations, seed); starting tours are seeded random permutations
CASES = {
    "tsp20": ("locs", 16, 20, 1000, 20),
    "tsp20_cap2": ("locs", 16, 20, 2, 20),      # the inputs of tsp20
    "tsp50": ("locs", 8, 50, 1000, 50),
    "lattice16": ("lattice", 8, 16, 1000, 16),  # a 4 x 4 grid of quarters: many exactly equal changes, the tie rule decides
    "asym12": ("distances", 8, 12, 1000, 12),   # explicit asymmetric matrix
}


def case_inputs(case: str) -> dict:
    kind, b, n, _, seed = CASES[case]
    g = torch.Generator().manual_seed(seed)
    if kind == "locs":
        data = {"in_locs": torch.rand(b, n, 2, generator=g)}
    elif kind == "lattice":
        grid = torch.stack(torch.meshgrid(torch.arange(4), torch.arange(4), indexing="ij"), -1).reshape(16, 2).float() / 4
        data = {"in_locs": torch.stack([grid[torch.randperm(16, generator=g)] for _ in range(b)])}
    else:
        data = {"in_distances": torch.rand(b, n, n, generator=g)}
    data["in_actions"] = torch.stack([torch.randperm(n, generator=g) for _ in range(b)])
    return data


def _numba_stand_in():
    """A module that lets local_search.py import and run without numba: ``njit(...)`` returns the function itself,
    ``prange`` is ``range``, the type objects of the signatures can be subscripted and called."""
    import types

    class _Type:
        def __getitem__(self, item):
            return self

        def __call__(self, *args, **kwargs):
            return self

    m = types.ModuleType("numba")
    m.njit = lambda *a, **k: (lambda fn: fn)
    m.prange = range
    m.set_num_threads = lambda n: None
    m.float32 = m.uint16 = m.int64 = _Type()
    return m


def _reference_module():
    import importlib
    import sys

    from oracle import ref_import

    ref_import.install()
    had = sys.modules.get("numba")
    sys.modules["numba"] = _numba_stand_in()
    try:
        return importlib.import_module("rl4co.envs.routing.tsp.local_search")
    finally:
        if had is None:
            del sys.modules["numba"]
        else:
            sys.modules["numba"] = had


def reference_run(case: str) -> dict:
    """The reference's ``local_search`` on the case, one tour at a time so that the calls of ``two_opt_once`` can be
    counted per tour. Every scan is also checked: the stand-in compares the move threshold in fp32 where numba compares
    in double, so no scan's best change may be one on which the two comparisons differ."""
    mod = _reference_module()
    kind, b, n, max_iterations, _ = CASES[case]
    data = case_inputs(case)
    key = "distances" if kind == "distances" else "locs"
    once = mod.two_opt_once
    calls = []

    def counted(distmat, tour, fixed_i=0):
        move = best_move(distmat, tour.astype(np.int64), pair_list(tour.shape[0]))
        if move is not None:
            assert bool(move[0] < np.float32(THRESHOLD)) == (float(move[0]) < THRESHOLD), (case, move)
        calls.append(1)
        return once(distmat, tour, fixed_i)

    mod.two_opt_once = counted
    try:
        outs, iters = [], []
        for k in range(b):
            calls.clear()
            td = {key: data[f"in_{key}"][k : k + 1]}
            outs.append(mod.local_search(td, data["in_actions"][k : k + 1], max_iterations=max_iterations))
            iters.append(len(calls))
    finally:
        mod.two_opt_once = once
    rec = dict(data)
    rec["out_actions"] = torch.cat(outs).to(torch.int64)
    rec["iterations"] = torch.tensor(iters, dtype=torch.int32)
    return rec


def record(case: str) -> dict:
    from tests.helpers import reference_record

    return reference_record(f"two_opt_{case}", lambda: reference_run(case))


def record_distances(rec: dict) -> torch.Tensor:
    """The matrix (without diagonal) a record's search ran over."""
    return rec["in_distances"] if "in_distances" in rec else distance_matrix(rec["in_locs"])


if __name__ == "__main__":  # RL4CO_RECORD_REFERENCE=1 python -m tests.two_opt_ref
    for name, (_, _, _, cap, _) in CASES.items():
        r = record(name)
        tours, iters = two_opt(record_distances(r), r["in_actions"], cap)
        assert torch.equal(tours, r["out_actions"]) and torch.equal(iters, r["iterations"]), name
        print(name, {k: tuple(v.shape) for k, v in r.items()}, "iterations", r["iterations"].tolist(), "== restatement")
