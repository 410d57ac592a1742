"""Philox4x32-10 restated in numpy from the published algorithm (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as
easy as 1, 2, 3", SC'11), and on top of it the noise stream the Ant System kernels draw when no ``ln_noise`` is given.

Nothing here calls the product header (rl4co_amd/csrc/rl4co_math.h) or the C oracle for the rounds, the counter layout or
the word-to-uniform map: tests/test_philox_cpu.py pins the header to this file and this file to the published known answers.
The two natural logs of ``ln_exp1`` are the header's ``rl4co_logf`` (through the C oracle's array form): tests/test_math.py
pins that function against float64 libm and its device copy bit for bit, so it is not restated a second time.

The stream layouts are the ones include/rl4co_amd.h and the header comments of csrc/aco_tsp.hip and csrc/aco_cvrp.hip state:
TSP   ln_noise [iterations, N - 1, rows, N], entry [it, t - 1, row, n] is the draw of step ``offset + it * N + t``, t = 1 .. N - 1;
CVRP  ln_noise [iterations, W, rows, N], entry [it, t, row, n] is the draw of step ``offset + it * W + t``, W = max(N, 2 N - 3);
the trajectory word is the row (ant-major: ``ant * B + instance``), the node picks block ``n >> 2`` and word ``n & 3``."""
import numpy as np
import torch

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)  # the two round multipliers
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)  # the Weyl increments of the two key words
LOW = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
STEP_TAG = np.uint64(0x52344C43)  # XOR-ed into the high word of the step (rl4co_math.h: rl4co_exp1_noise)


def _u64(x):
    """Python ints (up to 2^64 - 1) or integer arrays -> uint64 array."""
    if isinstance(x, int):
        return np.array(x & (2**64 - 1), dtype=np.uint64)
    return np.asarray(x).astype(np.uint64)


def philox4x32(counter, key, rounds: int = 10):
    """counter [..., 4], key [2] (or [..., 2]) of 32-bit words held in any integer type -> the four output words
    [..., 4] as uint32. One round: (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2,
    c <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key is bumped by the Weyl constants between rounds."""
    c = _u64(counter) & LOW
    k = _u64(key) & LOW
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for r in range(rounds):
        if r:
            k0, k1 = (k0 + W0) & LOW, (k1 + W1) & LOW
        p0, p1 = M0 * c0, M1 * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & LOW, (p0 >> S32) ^ c3 ^ k1, p0 & LOW
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def uniform(seed, step, traj, node):
    """The uniform in (0, 1) of (seed, step, trajectory, node), broadcast over the arguments, as fp32:
    counter (step lo, traj, node >> 2, step hi ^ tag), key (seed lo, seed hi), word node & 3,
    u = (float32(w >> 9) + 0.5) * 2^-23 (23 bits: exact in fp32, never 0 or 1)."""
    seed, step, traj, node = np.broadcast_arrays(_u64(seed), _u64(step), _u64(traj), _u64(node))
    counter = np.stack((step & LOW, traj & LOW, (node & LOW) >> np.uint64(2), ((step >> S32) & LOW) ^ STEP_TAG), -1)
    key = np.stack((seed & LOW, (seed >> S32) & LOW), -1)
    words = philox4x32(counter, key)
    w = np.take_along_axis(words, (node & np.uint64(3)).astype(np.int64)[..., None], -1)[..., 0]
    return ((w >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0**-23)


def _log(x: torch.Tensor) -> torch.Tensor:
    from oracle import c_oracle

    return c_oracle.math_array("log", x.contiguous())


def exp1(seed, step, traj, node) -> torch.Tensor:
    """The Exp(1) draw -log(u) as an fp32 tensor."""
    u = torch.from_numpy(np.ascontiguousarray(uniform(seed, step, traj, node)))
    return -_log(u)


def ln_exp1(seed, step, traj, node) -> torch.Tensor:
    """log(-log(u)): what the Ant System kernels subtract from the log-probs."""
    return _log(exp1(seed, step, traj, node))


def cvrp_width(n: int) -> int:
    """W = max(C + 1, 2 C - 1) with C = n - 1 customers."""
    return max(n, 2 * n - 3)


def _stream(seed: int, first_step: int, per_iteration: int, iterations: int, steps: int, rows: int, n: int) -> torch.Tensor:
    it = np.arange(iterations, dtype=np.uint64).reshape(-1, 1, 1, 1)
    t = np.arange(steps, dtype=np.uint64).reshape(1, -1, 1, 1)
    row = np.arange(rows, dtype=np.uint64).reshape(1, 1, -1, 1)
    node = np.arange(n, dtype=np.uint64).reshape(1, 1, 1, -1)
    step = _u64(first_step) + it * np.uint64(per_iteration) + t  # (uint64: wraps as the kernel's counter does)
    return ln_exp1(seed, step, row, node).reshape(iterations, steps, rows, n).contiguous()


def tsp_stream(seed: int, offset: int, iterations: int, n: int, rows: int) -> torch.Tensor:
    """fp32 [iterations, N - 1, rows, N]: entry [it, t - 1, row, node] is the draw of step offset + it * N + t."""
    return _stream(seed, offset + 1, n, iterations, n - 1, rows, n)


def cvrp_stream(seed: int, offset: int, iterations: int, n: int, rows: int) -> torch.Tensor:
    """fp32 [iterations, W, rows, N]: entry [it, t, row, node] is the draw of step offset + it * W + t."""
    w = cvrp_width(n)
    return _stream(seed, offset, w, iterations, w, rows, n)
