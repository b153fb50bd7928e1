"""Matching EQ tone controls without a GPU: ``MatchingEq``'s tone fields and ``ToneBand``, ``mgx_eq_tone_check``,
``mgx_eq_tone_curve`` and ``mgx_tone_fir`` -- the library's host twin of the tone stage -- against tests/eq_tone_oracle.py;
the properties of the definition on the oracle and then on the host code; the stand-alone program under the sanitizers.

Measured here (float64 on both sides): mgx_tone_fir against the oracle 6e-14 of the peak tap at most in linear phase and
4.7e-10 in minimum phase (the side channel under mono bass at 16384 taps, whose response has zeros; 9e-14 without mono
bass; 3.8e-10 on the golden curves) (bound 1e-9); mgx_eq_tone_curve's terms 1.7e-16 (weight), 8.9e-16 dB (trim) and 0
(gate) off the oracle at most (bound 1e-9).
"""

import ctypes
import json
import subprocess

import numpy as np
import pytest

import eq_tone_oracle as tone_oracle
import mastering_oracle as mo
from cases import CASES, build_inputs, oracle_params
from eq_tone_emu import NAN, shape_struct, tone_struct

c_double_p = ctypes.POINTER(ctypes.c_double)
BOUND = 1e-9                     # the project's bound for mgx_shape_fir


def native(fft=4096, fs=44100):
    """The default Config's mgx_config at another size and rate (set on the struct: the host entry points take any size)."""
    import matchering_amd as mg

    cfg = mg.Config().to_native()
    cfg.fft_size = fft
    cfg.internal_sample_rate = fs
    return cfg


def tones(fs=44100):
    """Each control alone and all together; frequencies scale with the rate so that every one is valid at every rate."""
    r = fs / 44100.0
    air = (2, 3, 9000.0 * r, 1.0, 0.7071)                   # high shelf, both
    dip = (0, 1, 300.0 * r, -2.5, 1.4)                      # bell, mid
    warm = (1, 2, 180.0 * r, 3.0, 0.5)                      # low shelf, side
    return {
        "range": tone_oracle.tone_of(low_hz=60.0 * r, high_hz=12000.0 * r),
        "range_low_only": tone_oracle.tone_of(low_hz=200.0 * r, range_octaves=2.0),
        "side_amount": tone_oracle.tone_of(side_amount=0.0),
        "mono": tone_oracle.tone_of(mono_below_hz=120.0 * r),
        "tilt": tone_oracle.tone_of(tilt_db_per_octave=-0.5),
        "bands": tone_oracle.tone_of(bands=(air, dip, warm)),
        "all": tone_oracle.tone_of(low_hz=60.0 * r, high_hz=12000.0 * r, range_octaves=0.5, side_amount=0.3,
                                   mono_below_hz=120.0 * r, mono_octaves=1.5, tilt_db_per_octave=0.75,
                                   tilt_pivot_hz=700.0 * r, bands=(air, dip, warm)),
    }


SHAPE = dict(amount=0.8, max_boost_db=9.0, max_cut_db=7.0)


def host_tone_fir(smooth, fft, fs, channel, tone, **shape):
    from matchering_amd._native import check, library

    smooth = np.ascontiguousarray(smooth, dtype=np.float64)
    assert smooth.shape == (fft // 2 + 1,)
    taps = np.full(fft, 7.0)
    check(library().mgx_tone_fir(ctypes.byref(native(fft, fs)), ctypes.byref(shape_struct(**shape)),
                                 None if tone is None else ctypes.byref(tone_struct(tone)), channel,
                                 smooth.ctypes.data_as(c_double_p), taps.ctypes.data_as(c_double_p)))
    return taps


def host_terms(fft, fs, channel, tone, **shape):
    from matchering_amd._native import check, library

    out = [np.full(fft // 2 + 1, 7.0) for _ in range(3)]
    check(library().mgx_eq_tone_curve(ctypes.byref(native(fft, fs)), ctypes.byref(shape_struct(**shape)),
                                      ctypes.byref(tone_struct(tone)), channel, *(v.ctypes.data_as(c_double_p) for v in out)))
    return out


def synthetic_curve(fft, seed=0):
    """A smoothed matching curve's look: a few dB of slow ripple, a steep rise at the top, bin 0 zero."""
    k = np.arange(fft // 2 + 1) / (fft // 2)
    rng = np.random.RandomState(seed)
    db = 9.0 * np.sin(2 * np.pi * (1.3 + seed) * k + rng.rand()) + 7.0 * np.cos(2 * np.pi * 4.1 * k) + 25.0 * k ** 6 - 6.0
    curve = 10.0 ** (db / 20.0)
    curve[0] = 0.0
    return curve


@pytest.fixture(scope="module")
def golden_curves():
    """The smoothed curves of four golden cases (mid and side) at their own sizes and rates: computed once, never written."""
    out = []
    for name in ("cd_default", "hot_lowrate", "custom_limiter", "robust_second_order"):
        case = CASES[name]
        target, reference = build_inputs(case)
        cfg = oracle_params(case["config"])
        trace = {}
        mo.master(target, reference, cfg, False, True, False, trace=trace)
        for channel, key in enumerate(("mid", "side")):
            smooth = np.array(trace[key].smooth, dtype=np.float64)
            smooth.setflags(write=False)
            out.append((name, channel, cfg, smooth))
    return out


# ---- mgx_tone_fir against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", ["linear", "minimum"])
@pytest.mark.parametrize("name", sorted(tones()))
@pytest.mark.parametrize("fft,fs", [(64, 44100), (4096, 44100), (16384, 96000)])
def test_tone_fir_matches_the_oracle(fft, fs, name, phase):
    """float64 on both sides, both channels: <= 1e-9 of the peak tap, each control alone and all together."""
    tone = tones(fs)[name]
    for channel in (0, 1):
        curve = synthetic_curve(fft, channel)
        want = tone_oracle.tone_fir(curve, 1e-6, fs, channel, tone, phase=phase, **SHAPE)
        got = host_tone_fir(curve, fft, fs, channel, tone, phase=phase, **SHAPE)
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{fft} {name} {phase} channel {channel}: {err:.3g} of the peak")
        assert err <= BOUND


def test_tone_fir_on_the_golden_curves(golden_curves):
    """The same on the golden cases' curves at their own sizes and rates, both phases."""
    worst = 0.0
    for case, channel, cfg, smooth in golden_curves:
        fft, fs = cfg.fft_size, cfg.internal_sample_rate
        for name, tone in tones(fs).items():
            for phase in ("linear", "minimum"):
                want = tone_oracle.tone_fir(smooth, cfg.min_value, fs, channel, tone, phase=phase, **SHAPE)
                got = host_tone_fir(smooth, fft, fs, channel, tone, phase=phase, **SHAPE)
                err = np.abs(got - want).max() / np.abs(want).max()
                worst = max(worst, err)
                assert err <= BOUND, (case, channel, name, phase, err)
    print(f"mgx_tone_fir on the golden curves: {worst:.3g} of the peak at most")


def test_neutral_and_null_tone_are_mgx_shape_fir():
    """A neutral tone is the call without a tone, bit for bit -- also where the shape stage is skipped."""
    from matchering_amd._native import check, library

    curve = synthetic_curve(4096, 3)
    for shape in (dict(), SHAPE, dict(SHAPE, phase="minimum")):
        plain = np.zeros(4096)
        check(library().mgx_shape_fir(ctypes.byref(native()), ctypes.byref(shape_struct(**shape)),
                                      curve.ctypes.data_as(c_double_p), plain.ctypes.data_as(c_double_p)))
        for channel in (0, 1):
            assert np.array_equal(host_tone_fir(curve, 4096, 44100, channel, None, **shape), plain)
            assert np.array_equal(host_tone_fir(curve, 4096, 44100, channel, tone_oracle.tone_of(range_octaves=3.0), **shape), plain)
        assert not np.array_equal(host_tone_fir(curve, 4096, 44100, 0, tone_oracle.tone_of(tilt_db_per_octave=0.01), **shape), plain)


def test_null_shape_with_a_tone_is_the_default_shape():
    from matchering_amd._native import check, library

    curve, tone = synthetic_curve(512, 1), tones()["all"]
    taps = np.zeros(512)
    check(library().mgx_tone_fir(ctypes.byref(native(512)), None, ctypes.byref(tone_struct(tone)), 1,
                                 curve.ctypes.data_as(c_double_p), taps.ctypes.data_as(c_double_p)))
    assert np.array_equal(taps, host_tone_fir(curve, 512, 44100, 1, tone))


# ---- mgx_eq_tone_curve against the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("fft,fs", [(64, 44100), (4096, 44100), (16384, 96000)])
def test_tone_curve_matches_the_oracle(fft, fs):
    """The three per-bin terms: weight times amount and gate within 1e-9 (linear), the trim within 1e-9 dB; entry 0 is 0."""
    worst = [0.0, 0.0, 0.0]
    for name, tone in tones(fs).items():
        for channel in (0, 1):
            got = host_terms(fft, fs, channel, tone, **SHAPE)
            want = tone_oracle.terms(fft, fs, channel, tone, SHAPE["amount"])
            for i, (mine, theirs) in enumerate(zip(got, want)):
                assert mine[0] == 0.0 and theirs[0] == 0.0
                worst[i] = max(worst[i], np.abs(mine - theirs).max())
                assert np.abs(mine - theirs).max() <= BOUND, (name, channel, i)
    print(f"{fft}: weight {worst[0]:.3g}, trim {worst[1]:.3g} dB, gate {worst[2]:.3g} off the oracle at most")


# ---- properties of the definition: on the oracle, then on the host code --------------------------------------------------
def test_outside_the_range_the_matching_part_is_exactly_zero(golden_curves):
    """More than range_octaves / 2 outside the range the weight is exactly 0, so without trims the toned curve is exactly 1:
    the target's own spectrum is left alone there."""
    for case, channel, cfg, smooth in golden_curves:
        fft, fs = cfg.fft_size, cfg.internal_sample_rate
        for octaves in (0.0, 1.0, 3.0):
            low, high = 0.02 * fs, 0.12 * fs
            tone = tone_oracle.tone_of(low_hz=low, high_hz=high, range_octaves=octaves)
            f = tone_oracle.frequencies(fft, fs)
            outside = (f < low * 2.0 ** (-octaves / 2) * (1 - 1e-9)) | (f > high * 2.0 ** (octaves / 2) * (1 + 1e-9))
            outside[0] = False
            inside = (f > low * 2.0 ** (octaves / 2) * (1 + 1e-9)) & (f < high * 2.0 ** (-octaves / 2) * (1 - 1e-9))
            assert outside.any()
            for weight in (tone_oracle.terms(fft, fs, channel, tone, 0.8)[0], host_terms(fft, fs, channel, tone, amount=0.8)[0]):
                assert not weight[outside].any()
                assert np.all(weight[inside] == 0.8)
            toned = tone_oracle.tone_curve(smooth, cfg.min_value, fs, channel, tone, amount=0.8)
            assert np.all(toned[outside] == 1.0)


def test_side_amount_zero_leaves_a_flat_side_curve(golden_curves):
    """side_amount = 0 without trims: the side curve is exactly 1 for k >= 1 -- whatever the matching curve, so the host's
    side taps do not depend on it at all -- and the mid taps are the ones without the control, bit for bit."""
    tone = tone_oracle.tone_of(side_amount=0.0)
    for case, channel, cfg, smooth in golden_curves:
        fft, fs = cfg.fft_size, cfg.internal_sample_rate
        if channel == 1:
            toned = tone_oracle.tone_curve(smooth, cfg.min_value, fs, 1, tone, **SHAPE)
            assert toned[0] == 0.0 and np.all(toned[1:] == 1.0)
            other = synthetic_curve(fft, 5)
            assert np.array_equal(host_tone_fir(smooth, fft, fs, 1, tone, **SHAPE), host_tone_fir(other, fft, fs, 1, tone, **SHAPE))
            flat = np.ones(fft // 2 + 1)
            flat[0] = 0.0
            assert np.array_equal(host_tone_fir(smooth, fft, fs, 1, tone, **SHAPE), host_tone_fir(flat, fft, fs, 1, None))
        else:
            assert np.array_equal(host_tone_fir(smooth, fft, fs, 0, tone, **SHAPE), host_tone_fir(smooth, fft, fs, 0, None, **SHAPE))


def test_side_only_controls_leave_the_mid_plane_alone(golden_curves):
    """The mid taps are bit-identical with and without any side-only control: side amount, mono bass, a side band."""
    for case, channel, cfg, smooth in golden_curves:
        if channel != 0:
            continue
        fft, fs = cfg.fft_size, cfg.internal_sample_rate
        base = tones(fs)["range"]
        want = host_tone_fir(smooth, fft, fs, 0, base, **SHAPE)
        oracle_want = tone_oracle.tone_curve(smooth, cfg.min_value, fs, 0, base, **SHAPE)
        for extra in (dict(side_amount=0.2), dict(mono_below_hz=0.003 * fs), dict(bands=((0, 2, 0.01 * fs, 6.0, 2.0),)),
                      dict(side_amount=1.7, mono_below_hz=0.003 * fs, mono_octaves=0.0, bands=((2, 2, 0.1 * fs, -3.0, 1.0),))):
            tone = dict(base, **extra)
            assert np.array_equal(host_tone_fir(smooth, fft, fs, 0, tone, **SHAPE), want)
            assert np.array_equal(tone_oracle.tone_curve(smooth, cfg.min_value, fs, 0, tone, **SHAPE), oracle_want)
            assert not np.array_equal(host_tone_fir(smooth, fft, fs, 1, tone, **SHAPE), host_tone_fir(smooth, fft, fs, 1, base, **SHAPE))


MONO_DROP_DB = 60.0


def test_mono_bass_takes_the_side_channel_out(golden_curves):
    """F = 4096 at 44.1 kHz, mono_below_hz = 120 over one octave: at every f <= 60 Hz the side taps' response lies at least
    60 dB under the same call's response without the control.  Measured on the oracle, the least over 30 frequencies from
    2 to 60 Hz: 79.2 dB on a flat curve and 84.04 dB on the golden curve used here (cd_default's side; the host function
    reads the same to 0.001 dB)."""
    tone = tone_oracle.tone_of(mono_below_hz=120.0)
    hz = np.linspace(2.0, 60.0, 30)
    flat = np.ones(2049)
    flat[0] = 0.0
    drop = tone_oracle.response_db(tone_oracle.tone_fir(flat, 1e-6, 44100, 1, None), hz, 44100) - \
        tone_oracle.response_db(tone_oracle.tone_fir(flat, 1e-6, 44100, 1, tone), hz, 44100)
    print(f"flat curve: {drop.min():.1f} dB under at f <= 60 Hz")
    assert drop.min() >= MONO_DROP_DB
    found = False
    for case, channel, cfg, smooth in golden_curves:
        if channel != 1 or cfg.fft_size != 4096 or cfg.internal_sample_rate != 44100:
            continue
        found = True
        for fir in (lambda t: tone_oracle.tone_fir(smooth, cfg.min_value, 44100, 1, t),
                    lambda t: host_tone_fir(smooth, 4096, 44100, 1, t)):
            drop = tone_oracle.response_db(fir(None), hz, 44100) - tone_oracle.response_db(fir(tone), hz, 44100)
            print(f"{case}: {drop.min():.3f} dB under at f <= 60 Hz")
            assert drop.min() >= MONO_DROP_DB
    assert found


# ---- refusals ------------------------------------------------------------------------------------------------------------
BAD_TONES = [(dict(low_hz=0.0), "low_hz"), (dict(low_hz=-5.0), "low_hz"), (dict(low_hz=22050.0), "low_hz"),
             (dict(low_hz=float("inf")), "low_hz"), (dict(high_hz=0.0), "high_hz"), (dict(high_hz=22050.5), "high_hz"),
             (dict(low_hz=500.0, high_hz=500.0), "low_hz"), (dict(low_hz=800.0, high_hz=500.0), "low_hz"),
             (dict(range_octaves=-0.1), "range_octaves"), (dict(range_octaves=4.5), "range_octaves"),
             (dict(range_octaves=NAN), "range_octaves"), (dict(side_amount=-0.1), "side_amount"),
             (dict(side_amount=2.5), "side_amount"), (dict(mono_below_hz=0.0), "mono_below_hz"),
             (dict(mono_below_hz=22050.0), "mono_below_hz"), (dict(mono_octaves=5.0), "mono_octaves"),
             (dict(mono_octaves=NAN), "mono_octaves"), (dict(tilt_db_per_octave=6.5), "tilt_db_per_octave"),
             (dict(tilt_db_per_octave=-7.0), "tilt_db_per_octave"), (dict(tilt_db_per_octave=NAN), "tilt_db_per_octave"),
             (dict(tilt_pivot_hz=0.0), "tilt_pivot_hz"), (dict(tilt_pivot_hz=NAN), "tilt_pivot_hz"),
             (dict(bands=((3, 3, 100.0, 1.0, 1.0),)), "bands[0].kind"), (dict(bands=((0, 0, 100.0, 1.0, 1.0),)), "bands[0].channels"),
             (dict(bands=((0, 4, 100.0, 1.0, 1.0),)), "bands[0].channels"),
             (dict(bands=((0, 3, 100.0, 1.0, 1.0), (0, 3, 0.0, 1.0, 1.0))), "bands[1].hz"),
             (dict(bands=((0, 3, 30000.0, 1.0, 1.0),)), "bands[0].hz"), (dict(bands=((0, 3, 100.0, 24.5, 1.0),)), "bands[0].gain_db"),
             (dict(bands=((0, 3, 100.0, NAN, 1.0),)), "bands[0].gain_db"), (dict(bands=((0, 3, 100.0, 1.0, 0.05),)), "bands[0].q"),
             (dict(bands=((0, 3, 100.0, 1.0, 21.0),)), "bands[0].q")]


def test_eq_tone_check_refuses_by_name():
    from matchering_amd._native import ERR_ARGUMENT, ERR_UNSUPPORTED, MgxEqTone, library

    lib = library()
    cfg = native()
    default = MgxEqTone()
    assert lib.mgx_eq_tone_default(ctypes.byref(default)) == 0
    assert bytes(default) == bytes(tone_struct(tone_oracle.tone_of()))
    assert lib.mgx_eq_tone_check(ctypes.byref(cfg), None, ctypes.byref(default)) == 0
    for tone in tones().values():
        assert lib.mgx_eq_tone_check(ctypes.byref(cfg), ctypes.byref(shape_struct(**SHAPE)), ctypes.byref(tone_struct(tone))) == 0
    # the ends of the ranges are inside
    edges = tone_oracle.tone_of(low_hz=1e-3, high_hz=22050.0, range_octaves=4.0, side_amount=2.0, mono_below_hz=22049.0,
                                mono_octaves=0.0, tilt_db_per_octave=-6.0, tilt_pivot_hz=1e-3,
                                bands=((2, 1, 22050.0, -24.0, 0.1), (1, 2, 1e-3, 24.0, 20.0)))
    assert lib.mgx_eq_tone_check(ctypes.byref(cfg), None, ctypes.byref(tone_struct(edges))) == 0
    for bad, field in BAD_TONES:
        struct = tone_struct(tone_oracle.tone_of(**bad))
        assert lib.mgx_eq_tone_check(ctypes.byref(cfg), None, ctypes.byref(struct)) == ERR_ARGUMENT, bad
        assert lib.mgx_last_error().decode().startswith(field + ":"), (bad, lib.mgx_last_error())
        curve, taps = np.ones(2049), np.zeros(4096)
        assert lib.mgx_tone_fir(ctypes.byref(cfg), None, ctypes.byref(struct), 0, curve.ctypes.data_as(c_double_p),
                                taps.ctypes.data_as(c_double_p)) == ERR_ARGUMENT
        assert lib.mgx_eq_tone_curve(ctypes.byref(cfg), None, ctypes.byref(struct), 0, None, None, None) == ERR_ARGUMENT
    for count in (-1, 9):
        assert lib.mgx_eq_tone_check(ctypes.byref(cfg), None, ctypes.byref(tone_struct(tone_oracle.tone_of(), band_count=count))) == ERR_ARGUMENT
        assert lib.mgx_last_error().decode().startswith("band_count:")
    assert lib.mgx_eq_tone_check(ctypes.byref(cfg), None, ctypes.byref(tone_struct(tone_oracle.tone_of(), reserved=1))) == ERR_ARGUMENT
    assert lib.mgx_last_error().decode().startswith("reserved:")
    # a band beyond band_count is not looked at
    beyond = tone_struct(tone_oracle.tone_of(bands=((0, 3, 100.0, 1.0, 1.0), (9, 9, -1.0, 99.0, 0.0))), band_count=1)
    assert lib.mgx_eq_tone_check(ctypes.byref(cfg), None, ctypes.byref(beyond)) == 0
    assert lib.mgx_eq_tone_check(None, None, ctypes.byref(default)) == ERR_ARGUMENT
    assert lib.mgx_eq_tone_check(ctypes.byref(cfg), None, None) == ERR_ARGUMENT
    assert lib.mgx_eq_tone_default(None) == ERR_ARGUMENT
    for channel in (-1, 2):
        assert lib.mgx_eq_tone_curve(ctypes.byref(cfg), None, ctypes.byref(default), channel, None, None, None) == ERR_ARGUMENT
        assert "channel" in lib.mgx_last_error().decode()
    # mgx_eq_shape_check's refusals come through
    assert lib.mgx_eq_tone_check(ctypes.byref(cfg), ctypes.byref(shape_struct(amount=3.0)), ctypes.byref(default)) == ERR_ARGUMENT
    assert "amount" in lib.mgx_last_error().decode()
    for fft in (32, 32768):
        minimum = shape_struct(phase="minimum")
        assert lib.mgx_eq_tone_check(ctypes.byref(native(fft)), ctypes.byref(minimum), ctypes.byref(tone_struct(tones()["tilt"]))) == ERR_UNSUPPORTED
        assert f"not {fft}" in lib.mgx_last_error().decode()
    # a frequency that is fine at one rate is refused at another
    assert lib.mgx_eq_tone_check(ctypes.byref(native(512, 8000)), None, ctypes.byref(tone_struct(tones()["range"]))) == ERR_ARGUMENT
    assert lib.mgx_last_error().decode().startswith("high_hz:") and "8000" in lib.mgx_last_error().decode()


def test_python_refuses_by_name():
    import matchering_amd as mg

    for bad, field in ((dict(match_range=(0.0, 100.0)), "match_range"), (dict(match_range=(500.0, 100.0)), "match_range"),
                       (dict(match_range=(100.0,)), "match_range"), (dict(match_range=("60", None)), "match_range"),
                       (dict(match_range=5.0), "match_range"), (dict(range_octaves=4.5), "range_octaves"),
                       (dict(range_octaves=None), "range_octaves"), (dict(side_amount=2.5), "side_amount"),
                       (dict(side_amount=True), "side_amount"), (dict(mono_below_hz=0.0), "mono_below_hz"),
                       (dict(mono_below_hz=NAN), "mono_below_hz"), (dict(mono_octaves=-1.0), "mono_octaves"),
                       (dict(tilt_db_per_octave=7.0), "tilt_db_per_octave"), (dict(tilt_db_per_octave=None), "tilt_db_per_octave"),
                       (dict(tilt_pivot_hz=0.0), "tilt_pivot_hz"), (dict(bands=({"kind": "bell"},)), "bands"),
                       (dict(bands="bell"), "bands"), (dict(bands=5), "bands"),
                       (dict(bands=tuple(mg.ToneBand("bell", 100.0 * (i + 1), 1.0) for i in range(9))), "bands")):
        with pytest.raises(ValueError, match=field):
            mg.MatchingEq(**bad)
    for bad, field in ((dict(kind="notch"), "kind"), (dict(kind=0), "kind"), (dict(hz=0.0), "hz"), (dict(hz="1k"), "hz"),
                       (dict(gain_db=25.0), "gain_db"), (dict(gain_db=NAN), "gain_db"), (dict(q=0.05), "q"), (dict(q=21.0), "q"),
                       (dict(channels="left"), "channels"), (dict(channels=3), "channels")):
        with pytest.raises(ValueError, match=f"ToneBand: {field}"):
            mg.ToneBand(**dict(dict(kind="bell", hz=1000.0, gain_db=1.0), **bad))
    with pytest.raises(Exception):
        mg.ToneBand("bell", 100.0, 1.0).hz = 5.0                      # frozen
    # what depends on the rate is check's, through mgx_eq_tone_check, with the library's message
    eq = mg.MatchingEq(match_range=(60.0, 12000.0))
    eq.check(mg.Config())
    with pytest.raises(ValueError, match="high_hz.*8000"):
        eq.check(mg.Config(internal_sample_rate=8000, fft_size=512))
    with pytest.raises(ValueError, match=r"bands\[1\]\.hz"):
        mg.MatchingEq(bands=(mg.ToneBand("bell", 100.0, 1.0), mg.ToneBand("high_shelf", 30000.0, 1.0))).check(mg.Config())
    with pytest.raises(ValueError, match="mono_below_hz"):
        mg.MatchingEq(mono_below_hz=30000.0).check(mg.Config())
    with pytest.raises(ValueError, match="32768"):
        mg.MatchingEq(phase="minimum", tilt_db_per_octave=1.0).check(mg.Config(fft_size=32768))


def test_process_refuses_a_bad_tone_before_any_file_is_read(tmp_path):
    import matchering_amd as mg

    results = [mg.pcm16(str(tmp_path / "out.wav"))]
    with pytest.raises(ValueError, match="mono_below_hz"):
        mg.process(str(tmp_path / "no_target.wav"), str(tmp_path / "no_reference.wav"), results,
                   eq=mg.MatchingEq(mono_below_hz=40000.0))
    with pytest.raises(ValueError, match="unknown keys"):
        mg.process(str(tmp_path / "no_target.wav"), str(tmp_path / "no_reference.wav"), results, eq={"mono_below": 120})
    jobs = [{"target": str(tmp_path / "t.wav"), "reference": str(tmp_path / "r.wav"), "results": results,
             "eq": {"bands": [{"kind": "bell", "hz": 30000.0, "gain_db": 2.0}]}}]
    with pytest.raises(ValueError, match=r"bands\[0\]\.hz"):
        mg.process_batch(jobs, rank=0, world_size=1)


# ---- MatchingEq: JSON, describe(), the structs ---------------------------------------------------------------------------
def test_neutral_matching_eq_is_unchanged():
    import matchering_amd as mg

    eq = mg.MatchingEq(0.5, 6, 6, "minimum")                           # positional construction: the four old fields first
    assert (eq.amount, eq.max_boost_db, eq.max_cut_db, eq.phase) == (0.5, 6, 6, "minimum")
    assert eq.describe() == "matching EQ: 50 %, +6/−6 dB, minimum phase" and eq.tone_native() is None and not eq.has_tone
    assert mg.MatchingEq().is_default and mg.MatchingEq().describe() == "matching EQ: 100 %, no caps, linear phase"
    assert mg.MatchingEq(range_octaves=2.0, mono_octaves=0.5, tilt_pivot_hz=500.0).tone_native() is None
    assert mg.MatchingEq(match_range=(None, None)).tone_native() is None
    s = eq.to_native()
    assert (s.amount, s.max_boost_db, s.max_cut_db, s.phase, s.reserved) == (0.5, 6.0, 6.0, 1, 0)
    toned = mg.MatchingEq(0.5, 6, 6, "minimum", tilt_db_per_octave=1.0)
    assert bytes(toned.to_native()) == bytes(s) and not toned.is_default
    assert not mg.MatchingEq(side_amount=1.0).is_default


def test_describe_appends_the_tone():
    import matchering_amd as mg

    bands = (mg.ToneBand("high_shelf", 10000.0, 1.0), mg.ToneBand("bell", 300.0, -2.0, q=1.4, channels="mid"))
    eq = mg.MatchingEq(amount=0.5, max_boost_db=6, max_cut_db=6, match_range=(60, 12000), side_amount=0, mono_below_hz=120,
                       tilt_db_per_octave=-0.5, bands=bands)
    assert eq.describe() == ("matching EQ: 50 %, +6/−6 dB, linear phase, 60 Hz – 12 kHz, side 0 %, mono below 120 Hz, "
                             "tilt −0.5 dB/oct, 2 bands")
    assert mg.MatchingEq(match_range=(60, None)).describe().endswith("linear phase, from 60 Hz")
    assert mg.MatchingEq(match_range=(None, 8500)).describe().endswith("linear phase, up to 8.5 kHz")
    assert mg.MatchingEq(tilt_db_per_octave=0.25, bands=bands[:1]).describe().endswith("linear phase, tilt +0.25 dB/oct, 1 band")
    assert mg.MatchingEq(side_amount=1.5).describe().endswith("linear phase, side 150 %")


def test_json_round_trip_and_unknown_keys():
    import matchering_amd as mg

    entry = {"amount": 0.5, "phase": "minimum", "match_range": [60, 12000], "range_octaves": 0.5, "side_amount": 0,
             "mono_below_hz": 120, "mono_octaves": 2, "tilt_db_per_octave": -0.5, "tilt_pivot_hz": 800,
             "bands": [{"kind": "high_shelf", "hz": 10000, "gain_db": 1.0},
                       {"kind": "bell", "hz": 300, "gain_db": -2, "q": 1.4, "channels": "mid"}]}
    eq = mg.MatchingEq.from_json(entry)
    assert eq == mg.MatchingEq(amount=0.5, phase="minimum", match_range=(60, 12000), range_octaves=0.5, side_amount=0,
                               mono_below_hz=120, mono_octaves=2, tilt_db_per_octave=-0.5, tilt_pivot_hz=800,
                               bands=(mg.ToneBand("high_shelf", 10000, 1.0), mg.ToneBand("bell", 300, -2, 1.4, "mid")))
    assert mg.MatchingEq.from_json(json.loads(json.dumps(eq.to_json()))) == eq
    assert mg.MatchingEq.from_json(json.loads(json.dumps(mg.MatchingEq().to_json()))) == mg.MatchingEq()
    assert mg.MatchingEq.from_json({"match_range": [None, 9000]}).match_range == (None, 9000)
    with pytest.raises(ValueError, match="unknown keys.*mono_below"):
        mg.MatchingEq.from_json({"mono_below": 120})
    with pytest.raises(ValueError, match="unknown keys.*gain"):
        mg.MatchingEq.from_json({"bands": [{"kind": "bell", "hz": 100, "gain": 2}]})
    with pytest.raises(ValueError, match="missing keys.*gain_db"):
        mg.MatchingEq.from_json({"bands": [{"kind": "bell", "hz": 100}]})
    with pytest.raises(ValueError, match="bands"):
        mg.MatchingEq.from_json({"bands": {"kind": "bell", "hz": 100, "gain_db": 1}})
    with pytest.raises(ValueError):
        mg.MatchingEq.from_json({"bands": ["bell"]})


def test_tone_native_and_struct_size():
    """tone_native() carries every field; sizeof(mgx_eq_tone) from the C compiler equals the ctypes size."""
    import eq_tone_emu
    import matchering_amd as mg
    from matchering_amd._native import MgxEqBand, MgxEqTone

    assert eq_tone_emu.library().emu_eq_tone_sizeof() == ctypes.sizeof(MgxEqTone) == 72 + 8 * ctypes.sizeof(MgxEqBand)
    eq = mg.MatchingEq(match_range=(60, None), range_octaves=0.5, side_amount=0.25, mono_below_hz=120, mono_octaves=2,
                       tilt_db_per_octave=-0.5, tilt_pivot_hz=800, bands=(mg.ToneBand("low_shelf", 90, 2.0, 0.9, "side"),))
    tone = eq.tone_native()
    want = tone_oracle.tone_of(low_hz=60.0, range_octaves=0.5, side_amount=0.25, mono_below_hz=120.0, mono_octaves=2.0,
                               tilt_db_per_octave=-0.5, tilt_pivot_hz=800.0, bands=((1, 2, 90.0, 2.0, 0.9),))
    assert bytes(tone) == bytes(tone_struct(want))


def test_curves_are_the_host_terms():
    import matchering_amd as mg

    eq = mg.MatchingEq(amount=0.8, match_range=(60, 12000), side_amount=0.0, mono_below_hz=120.0, tilt_db_per_octave=-0.5,
                       bands=(mg.ToneBand("high_shelf", 9000.0, 1.0),))
    curves = eq.curves(mg.Config())
    tone = tone_oracle.tone_of(low_hz=60.0, high_hz=12000.0, side_amount=0.0, mono_below_hz=120.0, tilt_db_per_octave=-0.5,
                               bands=((2, 3, 9000.0, 1.0, 0.7071),))
    assert np.array_equal(curves["hz"], tone_oracle.frequencies(4096, 44100))
    for channel, name in enumerate(("mid", "side")):
        want = tone_oracle.terms(4096, 44100, channel, tone, 0.8)
        for key, theirs in zip(("weight", "trim_db", "gate"), want):
            assert np.abs(curves[name][key] - theirs).max() <= BOUND
    assert not curves["side"]["weight"].any() and curves["mid"]["weight"].max() == 0.8
    neutral = mg.MatchingEq(amount=0.5).curves(mg.Config(fft_size=64))
    assert np.all(neutral["mid"]["weight"][1:] == 0.5) and not neutral["side"]["trim_db"].any() and np.all(neutral["side"]["gate"][1:] == 1.0)
    with pytest.raises(ValueError, match="mono_below_hz"):
        mg.MatchingEq(mono_below_hz=5000.0).curves(mg.Config(internal_sample_rate=8000, fft_size=512))


# ---- the stand-alone program under the sanitizers ------------------------------------------------------------------------
def test_standalone_driver_under_sanitizers(tmp_path):
    """mgx_eq_tone_check, mgx_eq_tone_curve and mgx_tone_fir (csrc/mgx_policy.cpp) and the emulated stage over exactly
    sized buffers, built with AddressSanitizer and UBSan and run as a program of its own: ``ok`` and exit status 0."""
    import emu_build
    import eq_tone_emu

    out = str(tmp_path / "emu_eq_tone_driver")
    emu_build.build_driver(eq_tone_emu.NAME, out, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    done = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip() == "ok", done.stdout + done.stderr
