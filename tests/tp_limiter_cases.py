"""The signals and shapes the CPU and the GPU tests of the deliveries' true-peak limiter share, and the oracle's answer to
each, computed once per process (tests/tp_limiter_oracle.py).  Test infrastructure.
"""

import functools

import numpy as np

import tp_limiter_oracle as oracle

TILE = 4096                 # T: TPL_TILE (csrc/tp_limit_kernel.h; test_tp_limiter_host.py checks these against the header)
BLOCK = 4096                # B: TPL_BLOCK -- block k ends where tile k + 1's window into the d0 plane begins
THREADS = 256
LOOKAHEAD_MAX = 2048
LOOKAHEADS = (1, 8, 66, 2048)
RELEASES = (0, 32, 2205)
PRE_GAIN, CEILING = 1.25, 0.8


def edge_sizes(lookahead):
    """Frames: the smallest tracks, the look-ahead and its window, a tile and an aggregate block one short, exact and one
    over, and more than two tiles with a ragged end."""
    t = TILE
    return sorted({1, 2, lookahead, 2 * lookahead + 1, t - 1, t, t + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1, 2 * t + 3})


def edge_signal(n, seed=0):
    """Noise at 0.2 with frames far above the ceiling at 0, T - 1, T and n - 1."""
    rng = np.random.RandomState(seed + n)
    x = (0.2 * rng.standard_normal((n, 2))).astype(np.float32)
    for frame in (0, TILE - 1, TILE, n - 1):
        if frame < n:
            x[frame] = (1.7, -1.3)
    return x


@functools.lru_cache(maxsize=None)
def edge_case(n, lookahead, release):
    """(x, the oracle's Limited) -- read-only: the tests share them."""
    x = edge_signal(n)
    want = oracle.limit(x, PRE_GAIN, CEILING, lookahead, release)
    for array in (x, want.out, want.s, want.e):
        array.setflags(write=False)
    return x, want


CARRY = dict(n=65536, pre_gain=1.0, ceiling=0.5, lookahead=66, release=2205)


@functools.lru_cache(maxsize=None)
def carry_case():
    """One impulse at frame 100 in 64 k frames of 0.05 noise: the gain's recovery at R = 2205 crosses about 11 tiles."""
    rng = np.random.RandomState(5)
    x = (0.05 * rng.standard_normal((CARRY["n"], 2))).astype(np.float32)
    x[100] = (1.5, 1.5)
    want = oracle.limit(x, CARRY["pre_gain"], CARRY["ceiling"], CARRY["lookahead"], CARRY["release"])
    for array in (x, want.out, want.s, want.e):
        array.setflags(write=False)
    return x, want


def within(got, x, pre_gain, want):
    """(ok, worst error / tolerance) of float32 frames ``got`` against the oracle's ``want``."""
    error = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    ratio = error / oracle.tolerance(x, pre_gain, want)
    worst = float(np.nanmax(ratio)) if ratio.size else 0.0
    return worst <= 1.0, worst


def quiet_signal(n, seed=3):
    """Under every ceiling the tests use at pre-gain up to 2: the limiter has nothing to do."""
    rng = np.random.RandomState(seed)
    return rng.uniform(-0.1, 0.1, (n, 2)).astype(np.float32)
