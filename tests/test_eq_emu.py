"""The matching EQ's device phase functions (csrc/eq_shape_kernels.h) under the host emulation (tests/emu/emu_eq_shape.cpp)
against tests/eq_oracle.py, without a GPU: the sizes at which the minimum-phase chain changes its route -- 1024 taps, the
largest at which a channel's transform is one workgroup; 2048, the smallest that is split -- the smallest size, 64, and
16384, where sixteen workgroups share a transform; 128 and 512, whose transforms have an odd log2 (the radix-2 stage in
front of the radix-4 passes), and 8192, eight workgroups.
"""

import numpy as np
import pytest

import eq_oracle
import eq_shape_emu


def curve(fft, seed):
    k = np.arange(fft // 2 + 1) / (fft // 2)
    db = 10.0 * np.sin(2 * np.pi * (1.7 + seed) * k + seed) + 6.0 * np.cos(2 * np.pi * 5.3 * k) + 20.0 * k ** 4 - 5.0
    out = 10.0 ** (db / 20.0)
    out[0] = 0.0
    return out


def test_route_boundaries():
    """One workgroup per channel and transform up to N = 4096 points, then 4096-point sub-transforms; the LDS of a
    workgroup stays under the 150 KB a launch may ask for, the scratch is two [2][N] double2 planes and two maxima."""
    want = {64: (8, 1), 128: (9, 1), 256: (10, 1), 512: (11, 1), 1024: (12, 1), 2048: (12, 2), 4096: (12, 4), 8192: (12, 8), 16384: (12, 16)}
    for fft, (log2m, r) in want.items():
        g = eq_shape_emu.geometry(fft)
        assert (g["log2m"], g["r"]) == (log2m, r)
        assert (1 << g["log2m"]) * g["r"] == 4 * fft
        assert g["threads"] == min(1024, max(64, (1 << log2m) // 4)) and g["lds_bytes"] <= 150 * 1024
        assert g["work_bytes"] == 4 * (4 * fft) * 16 + 16


@pytest.mark.parametrize("fft", [64, 128, 512, 1024, 2048, 8192, 16384])
def test_emulated_chain_matches_the_oracle(fft):
    """float32 linear taps in, float32 minimum-phase taps out: <= 2e-7 of the peak against eq_oracle's float64 chain on the
    same float32 input (one float32 rounding, 6e-8, with margin), both channels; zero before F/2."""
    lin = np.stack([eq_oracle.linear_taps(curve(fft, seed)) for seed in (0, 1)]).astype(np.float32)
    got, r = eq_shape_emu.minimum_phase(lin)
    assert r == eq_shape_emu.geometry(fft)["r"]
    for mine, linear in zip(got, lin):
        want = eq_oracle.minimum_phase(linear)
        assert np.abs(mine - want).max() <= 2e-7 * np.abs(want).max()
        assert not mine[:fft // 2].any()


def test_emulated_chain_takes_a_deep_floor():
    """A response with bins at zero (an odd-symmetric pair of taps): the logarithm is clamped at 1e-9 of the maximum."""
    fft = 1024
    lin = np.zeros((2, fft), dtype=np.float32)
    lin[0, fft // 2 - 1], lin[0, fft // 2 + 1] = 0.5, -0.5            # H(0) = H(pi) = 0
    lin[1] = eq_oracle.linear_taps(curve(fft, 2)).astype(np.float32)
    got, _ = eq_shape_emu.minimum_phase(lin)
    for mine, linear in zip(got, lin):
        want = eq_oracle.minimum_phase(linear)
        assert np.abs(mine - want).max() <= 2e-7 * np.abs(want).max()


@pytest.mark.parametrize("shape", [dict(amount=0.0), dict(amount=0.5), dict(amount=2.0),
                                   dict(amount=1.0, max_boost_db=3.0, max_cut_db=2.0),
                                   dict(amount=0.5, max_boost_db=6.0), dict(amount=1.5, max_cut_db=0.0)])
def test_emulated_shape_stage_matches_the_oracle(shape):
    """k_eq_shape's phase function on a curve with non-positive entries, float64 on both sides: 1e-14 relative."""
    smooth = curve(512, 3)
    smooth[7::9] = -1.0
    smooth[4::17] = 0.0
    got = eq_shape_emu.shape_curve(smooth, 1e-6, **shape)
    want = eq_oracle.shape_curve(smooth, 1e-6, **shape)
    assert got[0] == 0.0 and want[0] == 0.0
    assert np.abs(got[1:] / want[1:] - 1.0).max() <= 1e-14
