"""The host decisions of the decode launch over a grid: which variant serves (``rl4co_am_decode_variant``) and the
glimpse row groups the oracle mirrors (``rl4co_am_decode_row_groups``). Both are pure host functions: no GPU, no launch,
no pointer is dereferenced (the non-null ones here are dummy integers).

    python -m oracle.gen_dispatch_table          # records tests/golden/decode_dispatch_table.npz from the built library

Run at the commit BEFORE a change to the launchers; ``tests/test_decode_dispatch_cpu.py`` recomputes ``table()`` at the
change and asks for equality on every entry. Reads nothing but the library.
"""
from __future__ import annotations

import ctypes
import itertools
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parents[1] / "tests" / "golden" / "decode_dispatch_table.npz"

ENVS = tuple(range(8))  # RL4CO_ENV_TSP .. RL4CO_ENV_MTSP
DTYPES = (0, 1, 2)  # RL4CO_DT_F32, _BF16, _F16
NODES = (2, 20, 100, 106, 107, 112, 113, 128, 129, 501)
STEPS = (1, 3, 4, None)  # None: 2 N
BATCHES = ((64, 64), (1024, 1024), (1025, 1025), (2048, 2048), (2049, 2049), (4096, 4096), (8192, 4096), (12288, 4096),
           (28672, 4096), (32768, 4096))  # (B, B_inst)
VARIANTS = tuple(range(6))  # RL4CO_VARIANT_AUTO .. _STREAM_REG
FLAGS = ("none", "all_logps", "entropy", "top_k", "kept_bits", "unfold")
AXES = ("env", "cache_dtype", "N", "max_steps", "B_Binst", "variant", "flag")
DUMMY = 0x1000  # a non-null pointer that is never followed


def table() -> tuple[np.ndarray, np.ndarray]:
    """(variant, row_groups), int8, one entry per point of the grid in the order of AXES."""
    from rl4co_amd import _lib

    lib = _lib.lib()
    variant_of, groups_of = lib.rl4co_am_decode_variant, lib.rl4co_am_decode_row_groups
    shape = (len(ENVS), len(DTYPES), len(NODES), len(STEPS), len(BATCHES), len(VARIANTS), len(FLAGS))
    variant, groups = np.empty(shape, np.int8), np.empty(shape, np.int8)
    a = _lib.AmDecodeArgs()
    ref = ctypes.byref(a)
    for idx in itertools.product(*(range(n) for n in shape)):
        e, d, n, s, b, v, f = idx
        a.env, a.cache_dtype, a.N, a.variant = ENVS[e], DTYPES[d], NODES[n], VARIANTS[v]
        a.max_steps = 2 * NODES[n] if STEPS[s] is None else STEPS[s]
        a.B, a.B_inst = BATCHES[b]
        flag = FLAGS[f]
        a.all_logps = DUMMY if flag == "all_logps" else None
        a.entropy = DUMMY if flag == "entropy" else None
        a.kept_bits = DUMMY if flag == "kept_bits" else None
        a.top_k = 5 if flag == "top_k" else 0
        a.unfold = 1 if flag == "unfold" else 0
        variant[idx], groups[idx] = variant_of(ref), groups_of(ref)
    return variant, groups


if __name__ == "__main__":
    variant, groups = table()
    np.savez_compressed(GOLDEN, variant=variant, row_groups=groups, axes=np.array(AXES), nodes=np.array(NODES),
                        steps=np.array([0 if s is None else s for s in STEPS]), batches=np.array(BATCHES),
                        flags=np.array(FLAGS))
    print(f"{GOLDEN}: {variant.size} entries, {GOLDEN.stat().st_size} bytes; variants {np.unique(variant).tolist()}, "
          f"row groups {np.unique(groups).tolist()}")
