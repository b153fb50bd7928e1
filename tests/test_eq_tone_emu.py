"""The tone stage's device phase function (csrc/eq_tone.h, what k_eq_tone runs per thread) under the host emulation
(tests/emu/emu_eq_tone.cpp) against tests/eq_tone_oracle.py, without a GPU: whole planes at 33 bins (F = 64, one partial
workgroup), 2049 bins (nine workgroups, the last with one thread at work) and 8193 bins at 96 kHz; the edge cases of the
definition, one test case each; and the bits of the emulated k_eq_shape where the tone asks for nothing new.

Measured: 5.8e-16 relative to the oracle at most over the three sizes and every tone (bound 1e-9).
"""

import numpy as np
import pytest

import eq_shape_emu
import eq_tone_emu
import eq_tone_oracle as tone_oracle
from eq_tone_emu import shape_struct

BOUND = 1e-9
MIN_VALUE = 1e-6
SIZES = [(64, 44100), (4096, 44100), (16384, 96000)]                   # bins 33, 2049, 8193


def planes_of(fft, seed=0):
    """Two smooth planes with the look of matching curves, some entries non-positive (clamped at min_value)."""
    k = np.arange(fft // 2 + 1) / (fft // 2)
    out = np.empty((2, fft // 2 + 1))
    for plane in (0, 1):
        db = 10.0 * np.sin(2 * np.pi * (1.7 + seed + plane) * k + seed) + 6.0 * np.cos(2 * np.pi * 5.3 * k) + 20.0 * k ** 4 - 5.0
        out[plane] = 10.0 ** (db / 20.0)
    out[0, 7::9] = -1.0
    out[1, 4::17] = 0.0
    out[:, 0] = 0.37                                                     # (whatever bin 0 held, it leaves as 0)
    return out


def oracle_planes(planes, fs, tone, **shape):
    return np.stack([tone_oracle.tone_curve(planes[c], MIN_VALUE, fs, c, tone, **shape) for c in (0, 1)])


def close(got, want):
    assert np.all(np.isfinite(got))
    scale = np.maximum(np.abs(want), 1e-300)
    return float((np.abs(got - want) / scale).max())


def tones(fs):
    r = fs / 44100.0
    bands = ((2, 3, 9000.0 * r, 1.0, 0.7071), (0, 1, 300.0 * r, -2.5, 1.4), (1, 2, 180.0 * r, 3.0, 0.5))
    return {
        "range": tone_oracle.tone_of(low_hz=60.0 * r, high_hz=12000.0 * r),
        "side_amount": tone_oracle.tone_of(side_amount=0.25),
        "mono": tone_oracle.tone_of(mono_below_hz=120.0 * r),
        "tilt": tone_oracle.tone_of(tilt_db_per_octave=-0.5),
        "bands": tone_oracle.tone_of(bands=bands),
        "all": tone_oracle.tone_of(low_hz=60.0 * r, high_hz=12000.0 * r, range_octaves=0.5, side_amount=0.3,
                                   mono_below_hz=120.0 * r, mono_octaves=1.5, tilt_db_per_octave=0.75,
                                   tilt_pivot_hz=700.0 * r, bands=bands),
    }


SHAPE = dict(amount=0.8, max_boost_db=9.0, max_cut_db=7.0)


@pytest.mark.parametrize("name", sorted(tones(44100)))
@pytest.mark.parametrize("fft,fs", SIZES)
def test_emulated_tone_stage_matches_the_oracle(fft, fs, name):
    """Whole planes through the launch's grid: within 1e-9 of the oracle, relative, bin 0 zero; the mono gate's zeros are
    zeros on both sides."""
    planes, tone = planes_of(fft), tones(fs)[name]
    got = eq_tone_emu.tone_planes(planes, fs, MIN_VALUE, tone, shape_struct(**SHAPE))
    want = oracle_planes(planes, fs, tone, **SHAPE)
    assert got.shape == planes.shape and not got[:, 0].any()
    assert np.array_equal(got == 0.0, want == 0.0)
    err = close(got, want)
    print(f"{fft} {name}: {err:.3g} off the oracle")
    assert err <= BOUND
    # a null shape is amount 1 without caps
    assert close(eq_tone_emu.tone_planes(planes, fs, MIN_VALUE, tone), oracle_planes(planes, fs, tone)) <= BOUND


@pytest.mark.parametrize("shape", [dict(amount=0.5), dict(amount=0.0), dict(amount=2.0, max_boost_db=3.0, max_cut_db=2.0), dict(amount=1.0)])
@pytest.mark.parametrize("fft,fs", SIZES)
def test_side_amount_equal_to_amount_gives_the_shape_stage_bits(fft, fs, shape):
    """A tone that only sets side_amount = amount: a * 1, d + 0 and * 1 change no bit of the emulated k_eq_shape's planes."""
    planes = planes_of(fft, 1)
    got = eq_tone_emu.tone_planes(planes, fs, MIN_VALUE, tone_oracle.tone_of(side_amount=shape["amount"]), shape_struct(**shape))
    want = np.stack([eq_shape_emu.shape_curve(planes[c], MIN_VALUE, **shape) for c in (0, 1)])
    assert np.array_equal(got, want)


# ---- the edge cases, each its own case ------------------------------------------------------------------------------------
FFT, FS = 4096, 44100
F1 = FS / FFT                                                            # 10.77 Hz


def run_both(tone, planes=None, **shape):
    planes = planes_of(FFT, 2) if planes is None else planes
    got = eq_tone_emu.tone_planes(planes, FS, MIN_VALUE, tone, shape_struct(**shape))
    want = oracle_planes(planes, FS, tone, **shape)
    assert close(got, want) <= BOUND and np.array_equal(got == 0.0, want == 0.0)
    return planes, got


def test_edge_low_hz_below_the_first_bin():
    """low_hz a quarter of f_1 with a half-octave edge: every bin is fully inside, the stage is the plain shape stage."""
    planes, got = run_both(tone_oracle.tone_of(low_hz=F1 / 4, range_octaves=0.5), amount=0.7)
    assert np.array_equal(got, np.stack([eq_shape_emu.shape_curve(planes[c], MIN_VALUE, amount=0.7) for c in (0, 1)]))
    # ... and with a four-octave edge bin 1 lies on it, three quarters up, and bin 2 exactly at its top
    planes, got = run_both(tone_oracle.tone_of(low_hz=F1 / 2, range_octaves=4.0), amount=0.7)
    weights = tone_oracle.terms(FFT, FS, 0, tone_oracle.tone_of(low_hz=F1 / 2, range_octaves=4.0))[0]
    assert abs(weights[1] - (0.5 - 0.5 * np.cos(0.75 * np.pi))) <= 1e-15 and weights[2] == 1.0


def test_edge_high_hz_at_nyquist():
    """high_hz == fs/2 with a one-octave edge: the weight at the last bin is exactly 1/2."""
    tone = tone_oracle.tone_of(high_hz=FS / 2)
    run_both(tone, amount=1.0)
    weight = tone_oracle.terms(FFT, FS, 0, tone)[0]
    assert abs(weight[-1] - 0.5) <= 1e-15 and weight[FFT // 8] == 1.0


def test_edge_hard_range_edge_exactly_on_a_bin():
    """range_octaves == 0 with low_hz exactly f_8 (k * fs / F is exact): f >= low gives 1, so bin 8 is inside, bin 7 out."""
    low = (8 * FS) / FFT
    tone = tone_oracle.tone_of(low_hz=low, high_hz=(100 * FS) / FFT, range_octaves=0.0)
    planes, got = run_both(tone, amount=1.0)
    assert np.all(got[:, 1:8] == 1.0) and np.all(got[:, 100:] == 1.0)                  # outside: left alone (1 - edge is 0 AT high)
    shaped = np.stack([eq_shape_emu.shape_curve(planes[c], MIN_VALUE, amount=1.0, max_boost_db=200.0) for c in (0, 1)])
    assert np.array_equal(got[:, 8:100], shaped[:, 8:100])


def test_edge_band_centred_exactly_on_a_bin():
    """A bell at f_300 exactly: its gain there is gain_db to the last bit, since f/hz - hz/f is 0."""
    hz = (300 * FS) / FFT
    tone = tone_oracle.tone_of(bands=((0, 3, hz, 6.0, 4.0),))
    planes = np.ones((2, FFT // 2 + 1))
    _, got = run_both(tone, planes=planes, amount=1.0)
    assert np.all(got[:, 300] == 10.0 ** (6.0 / 20.0))
    assert np.all(got[:, 290:300] < got[:, 300:301]) and np.all(got[:, 301:310] < got[:, 300:301])


def test_edge_mono_edge_narrower_than_a_bin():
    """mono_below_hz between f_11 and f_12 with an edge of 0.01 octave: no bin lies on the edge; bins up to 11 are zero on
    the side, 12 and up untouched; the mid plane does not see it."""
    tone = tone_oracle.tone_of(mono_below_hz=11.5 * F1, mono_octaves=0.01)
    planes, got = run_both(tone, amount=0.5)
    plain = np.stack([eq_shape_emu.shape_curve(planes[c], MIN_VALUE, amount=0.5) for c in (0, 1)])
    assert not got[1, :12].any() and np.array_equal(got[1, 12:], plain[1, 12:]) and np.array_equal(got[0], plain[0])


def test_edge_eight_bands():
    """band_count == 8, every kind and channel mask."""
    bands = tuple((i % 3, 1 + i % 3, 40.0 * 2.2 ** i, 3.0 if i % 2 else -4.5, 0.3 + 0.6 * i) for i in range(8))
    run_both(tone_oracle.tone_of(bands=bands), **SHAPE)
    # the shelves at extreme ratios: (f/hz)^(4q) overflows to infinity, the gain goes to 0 and nothing turns NaN
    steep = ((1, 3, 1e-3, 24.0, 20.0), (2, 3, FS / 2, -24.0, 20.0))
    _, got = run_both(tone_oracle.tone_of(bands=steep), planes=np.ones((2, FFT // 2 + 1)), amount=1.0)
    assert np.all(got[:, 1:FFT // 4] == 1.0)


def test_edge_side_amount_zero_with_mono_bass():
    """side_amount == 0 together with mono_below_hz: the side plane is the gate itself."""
    tone = tone_oracle.tone_of(side_amount=0.0, mono_below_hz=120.0)
    _, got = run_both(tone, **SHAPE)
    gate = tone_oracle.terms(FFT, FS, 1, tone)[2]
    assert np.array_equal(got[1], gate) and not got[1, :8].any() and np.all(got[1, 16:] == 1.0)


def test_edge_amount_zero_with_bands_only():
    """amount == 0 with bands only: the planes are the trims alone, whatever the curves held."""
    tone = tone_oracle.tone_of(bands=((2, 3, 9000.0, 2.0, 0.7071), (0, 2, 250.0, -3.0, 2.0)), tilt_db_per_octave=0.3)
    _, got = run_both(tone, amount=0.0)
    _, other = run_both(tone, planes=planes_of(FFT, 9), amount=0.0)
    assert np.array_equal(got, other)
    for c in (0, 1):
        trim = tone_oracle.terms(FFT, FS, c, tone, 0.0)[1]
        assert np.abs(20.0 * np.log10(got[c, 1:]) - trim[1:]).max() <= 1e-9


def test_edge_bin_zero_stays_zero():
    """Bin 0 leaves as 0 under every tone, whatever it held, NaN included; no other bin is touched by it."""
    for fft, fs in SIZES:
        for tone in tones(fs).values():
            planes = planes_of(fft)
            planes[:, 0] = np.nan
            got = eq_tone_emu.tone_planes(planes, fs, MIN_VALUE, tone, shape_struct(**SHAPE))
            assert not got[:, 0].any() and np.all(np.isfinite(got))
