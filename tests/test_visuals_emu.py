"""The visuals' kernels on a machine without a GPU: their per-thread phase functions (window and load with both
overhangs, the mirror separation, the pooling indices; the overview's record) driven on the host against the float64
oracle at 256 and 4096 points, and the emulation's stand-alone program under the host sanitizers."""
import subprocess

import numpy as np
import pytest

import emu_build
import visuals_emu as emu
import visuals_oracle as oracle
from matchering_amd import visuals

BOUND = 4e-6          # of the picture's largest value, per channel: the analysis bound (2e-6 in magnitude) carried to power


def track(n, seed, tone_bin=None, fft_size=256):
    rng = np.random.default_rng(seed)
    x = 0.1 * rng.standard_normal((n, 2)).astype(np.float32)
    if tone_bin is not None:
        t = np.arange(n)
        x[:, 0] += (0.5 * np.sin(2 * np.pi * tone_bin * t / fft_size)).astype(np.float32)
        x[:, 1] += (0.25 * np.cos(2 * np.pi * (tone_bin + 3) * t / fft_size)).astype(np.float32)
    return x


def worst(got, want):
    return max(float(np.max(np.abs(got[:, ch] - want[:, ch])) / np.max(want[:, ch])) for ch in range(2))


@pytest.mark.parametrize("fft_size, n, hop, columns, mode", [
    (256, 640, 64, 0, 0),            # hops over the start (the first two) and over the end
    (256, 640, 64, 0, 1),
    (256, 300, 1, 3, 0),             # 100 hops a column: four workgroups each, the last a short one
    (256, 1, 256, 0, 0),             # one frame
    (256, 127, 100, 1, 1),           # a track shorter than half a window
    (4096, 10240, 1024, 0, 0),
    (4096, 10240, 1000, 4, 1),       # a hop that does not divide N
    (4096, 4097, 4096, 2, 0),        # no overlap
])
def test_every_bin_against_the_oracle(fft_size, n, hop, columns, mode):
    x = track(n, fft_size + n + hop, tone_bin=fft_size // 8, fft_size=fft_size)
    edges = visuals.linear_bands(fft_size)
    want = oracle.spectrogram(x, fft_size, hop, columns, edges, mode)
    got = emu.spectrogram(x, fft_size, hop, columns, edges, mode)
    assert got.shape == want.shape and np.all(np.isfinite(got))
    error = worst(got.astype(np.float64), want)
    print(f"N {fft_size} n {n} hop {hop} columns {columns} mode {mode}: {error:.3e}")
    assert error <= BOUND


@pytest.mark.parametrize("fft_size", [256, 4096])
def test_pooling_indices(fft_size):
    x = track(3 * fft_size, 11, tone_bin=fft_size // 16, fft_size=fft_size)
    hop = fft_size // 4
    for edges in (visuals.log_bands(fft_size, 44100, 24), np.array([0, fft_size // 2 + 1], dtype=np.int32),
                  np.array([3, 4, fft_size // 2, fft_size // 2 + 1], dtype=np.int32)):
        for columns in (0, 5, 1):
            want = oracle.spectrogram(x, fft_size, hop, columns, edges)
            got = emu.spectrogram(x, fft_size, hop, columns, edges)
            assert got.shape == want.shape
            assert worst(got.astype(np.float64), want) <= BOUND


def test_an_impulse_at_either_end_reads_the_window():
    fft_size, hop, n = 256, 64, 700
    w = oracle.window(fft_size).astype(np.float64)
    scale = (2.0 / w.sum()) ** 2
    for pos in (0, n - 1):
        x = np.zeros((n, 2), dtype=np.float32)
        x[pos, 0] = 1.0
        got = emu.spectrogram(x, fft_size, hop, 0, visuals.linear_bands(fft_size))
        for t in range(got.shape[0]):
            inside = pos - (t * hop - fft_size // 2)
            want = w[inside] ** 2 * scale if 0 <= inside < fft_size else 0.0
            assert np.max(np.abs(got[t, 0] - want)) <= BOUND * scale, (pos, t)
            # the silent channel shares the transform: what leaks is rounding, the square of float32's epsilon
            assert np.max(got[t, 1]) <= 1e-12 * scale


def test_overview_against_the_oracle():
    share = emu.constants()["share"]
    n = 2 * share + 1234
    x = track(n, 5)
    x[100, 0], x[200, 1], x[300, 0] = np.nan, np.inf, -np.inf
    for columns in (1, 2, 7, n // 3):
        lo, hi, sq = emu.overview(x, columns)
        want_lo, want_hi, want_sq = oracle.overview(x, columns)
        assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi)
        finite = np.isfinite(want_sq)
        assert np.array_equal(finite, np.isfinite(sq)) and np.array_equal(np.isnan(want_sq), np.isnan(sq))
        frames = np.diff(oracle.column_bounds(n, columns))[:, None]
        bound = (frames * 2.0 ** -52 * want_sq)[finite]
        assert np.all(np.abs(sq[finite] - want_sq[finite]) <= bound)


def test_constants():
    c = emu.constants()
    assert 1 <= c["run_cap"] <= 64 and c["run_cap"] == 32          # (tests/test_gpu_visuals.py places its hops by it)
    assert c["share"] == 16384 and c["share"] % c["threads"] == 0 and c["threads"] % 64 == 0
    assert c["columns_max"] == 65536 and c["frames_max"] == 500_000_000


def test_standalone_program_under_sanitizers(tmp_path):
    out = str(tmp_path / "emu_visuals_driver")
    emu_build.build_driver(emu.NAME, out, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    done = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip().endswith("ok"), done.stdout + done.stderr
