"""Noise-shaped deliveries without a GPU (include/mgx.h: mgx_noise_shaper_preset, mgx_delivery_gain_shaped,
mgx_delivery_limit_step_shaped; csrc/deliver_shaped_kernel.h on the CPU): the kernel's phase functions against the numpy
definition byte for byte, the policy against its formula, the presets against the published landmarks of their noise
transfer functions, the ceiling as a theorem about the decoded file, the error's spectrum against 0.25 |H|^2, and the
Python surface."""

import ctypes
import json
import math
import os

import numpy as np
import pytest

import deliver_shaped_emu as emu
import deliver_shaped_oracle as oracle
import delivery_oracle
import emu_build
import loudness_oracle
import matchering_amd as mg
from matchering_amd import _native
from matchering_amd.delivery import Delivered, Delivery, DeliveryRequest, NoiseShaper, delivery_gain, limit_step
from matchering_amd.loudness import Loudness

B, W = oracle.SEGMENT, oracle.WARMUP
N_SPECTRUM, POINTS, AVERAGES, RATE = 1 << 17, 256, 512, 44100       # the spectrum test's analysis
SEED = 2 ** 40 + 3                                                   # above 2^32: both key words matter
K1 = (0.7,)
K16 = tuple((-1.0) ** k * 0.9 / (k + 1) for k in range(16))
SHAPERS = {"lipshitz5": oracle.LIPSHITZ5, "wannamaker9": oracle.WANNAMAKER9, "K1": K1, "K16": K16}


def frames_of(n, seed):
    """(n, 2) float32 over the whole range and beyond it (they clip after the gain too), a few within an LSB of zero."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1.6, 1.6, (n, 2)).astype(np.float32)
    x[::5] *= np.float32(1e-4)
    x[0, 0] = 3.0
    return x


# ---- the kernel's body on the CPU ---------------------------------------------------------------------------------------

def test_constants_are_the_headers():
    k = emu.constants()
    assert (k["B"], k["W"]) == (B, W) == (_native.SHAPER_SEGMENT, _native.SHAPER_WARMUP)
    assert B % k["step"] == 0 and W % k["step"] == 0 and k["step"] % 2 == 0 and k["chains"] == 2 * k["tile"] == 64
    assert k["threads"] % k["chains"] == 0 and (k["tile"] * k["step"] // 2) % k["threads"] == 0
    assert k["lds_bytes"] <= 64 * 1024


def edge_sizes():
    tile = emu.constants()["tile"]
    return [1, 2, W - 1, W, W + 1, B - 1, B, B + 1, B + W - 1, B + W, B + W + 1, 2 * B, 3 * B + 7, tile * B + B + 1]


@pytest.mark.parametrize("name", sorted(SHAPERS))
@pytest.mark.parametrize("bits", [16, 24])
def test_emulated_kernel_is_the_oracle_byte_for_byte(bits, name):
    for n in edge_sizes():
        x = frames_of(n, n % 1000)
        gain = 0.77                                                  # 1.6 * 0.77 > 1: samples clip after the gain
        want = oracle.deliver_shaped(x, gain, bits, SHAPERS[name], SEED)
        assert emu.deliver_shaped(x, gain, bits, SHAPERS[name], SEED) == oracle.packed(want, bits), (n, bits, name)
        if n > 8:
            assert want.max() == 2 ** (bits - 1) - 1 and want.min() == -2 ** (bits - 1)


def test_no_taps_is_the_tpdf_delivery():
    deliver = emu_build.load("deliver")
    deliver.emu_deliver.restype = ctypes.c_longlong
    deliver.emu_deliver.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_longlong]
    for n in (1, 2, 511, B + 1, 3 * B + 7):
        x = frames_of(n, 5)
        raw = np.zeros((2 * n * 4 + 64) // 16 * 16 + 16, dtype=np.uint8)
        offset = (-raw.ctypes.data) % 16
        xin = raw[offset:offset + 8 * n].view(np.float32)
        xin[:] = x.reshape(-1)
        for bits in (16, 24):
            out = np.zeros(2 * n * 3 + 32, dtype=np.uint8)
            skip = (-out.ctypes.data) % 16
            deliver.emu_deliver(xin.ctypes.data, 2 * n, 0.77, bits, 1, SEED, out.ctypes.data + skip, 0)
            plain = out[skip:skip + 2 * n * bits // 8].tobytes()
            assert plain == oracle.packed(delivery_oracle.deliver(x, 0.77, bits, 1, SEED), bits)
            assert emu.deliver_shaped(x, 0.77, bits, (), SEED) == plain, (n, bits)


def test_one_segment_over_the_track_is_the_sequential_filter():
    """The oracle with B >= n and the emulation with one chain per channel over the whole track are the textbook
    error-feedback quantiser, frame after frame in plain Python."""
    x = frames_of(300, 9)
    for coefficients in (oracle.LIPSHITZ5, K16):
        plain = oracle.sequential_reference(x, 0.5, 16, coefficients, 7)
        assert np.array_equal(oracle.deliver_shaped(x, 0.5, 16, coefficients, 7, segment=4096, warmup=0), plain)
        assert emu.deliver_shaped(x, 0.5, 16, coefficients, 7, segment=4096, warmup=0) == oracle.packed(plain, 16)
    # ... and the segments matter: the same track cut at 64 frames differs (the definition is the segmented one)
    assert not np.array_equal(oracle.deliver_shaped(x, 0.5, 16, oracle.LIPSHITZ5, 7, segment=64, warmup=0),
                              oracle.sequential_reference(x, 0.5, 16, oracle.LIPSHITZ5, 7))


# ---- the presets and the policy -----------------------------------------------------------------------------------------

def preset(identifier, rate=44100):
    out = _native.MgxNoiseShaper()
    rc = _native.library().mgx_noise_shaper_preset(identifier, rate, ctypes.byref(out))
    return rc, out, _native.library().mgx_last_error().decode()


def native_shaper(coefficients, taps=None):
    out = _native.MgxNoiseShaper()
    out.taps = len(coefficients) if taps is None else taps
    for k, value in enumerate(coefficients[:16]):
        out.c[k] = value
    return out


def test_preset_tables():
    for identifier, want in oracle.PRESETS.items():
        for rate in (44100, 47999, 48000):
            rc, out, text = preset(identifier, rate)
            assert rc == 0, text
            assert out.taps == len(want) and tuple(out.c[:out.taps]) == want and out.reserved == 0
            assert all(v == 0.0 for v in out.c[out.taps:])
    assert NoiseShaper.lipshitz5().coefficients == oracle.LIPSHITZ5 and NoiseShaper.lipshitz5().preset == "lipshitz5"
    assert NoiseShaper.wannamaker9().coefficients == oracle.WANNAMAKER9


# |H|^2 at DC, in the notch (dB, at Hz) and at 22 050 Hz, and sum |c|: computed from the published numbers
LANDMARKS = {1: (-16.6, -26.9, 3962.0, 19.4, 8.3619), 2: (-12.0, -24.7, 3445.0, 27.0, 21.3857)}


@pytest.mark.parametrize("identifier", [1, 2])
def test_noise_transfer_function_landmarks(identifier):
    """Known answers that a wrong sign or a typo in the table would move: to the 0.1 dB, the 1 Hz and the 1e-4 they are
    stated to (half a unit of the last place each)."""
    rc, out, _ = preset(identifier)
    assert rc == 0
    c = tuple(out.c[:out.taps])
    dc, notch_db, notch_hz, nyquist, total = LANDMARKS[identifier]
    db = lambda f: 10.0 * np.log10(oracle.ntf_power(c, f, 44100))
    assert abs(float(db([0.0])[0]) - dc) <= 0.05
    assert abs(float(db([22050.0])[0]) - nyquist) <= 0.05
    # the notch landmark is |H|^2 AT the stated frequency, a bin of the 256-point analysis (5 taps: the lowest bin; 9 taps:
    # two bins above the lowest, 3101 Hz at -25.2 dB); the curve's minimum lies in the 2-5 kHz region and no higher
    assert abs(float(db([notch_hz])[0]) - notch_db) <= 0.05
    grid = np.arange(POINTS // 2 + 1) * RATE / POINTS
    curve = db(grid)
    assert abs(grid - notch_hz).min() <= 0.5
    assert 2000.0 <= float(grid[np.argmin(curve)]) <= 5000.0 and float(curve.min()) <= notch_db + 0.05
    assert abs(sum(abs(v) for v in c) - total) <= 0.5e-4


def test_preset_refusals_name_their_field():
    for rate in (44099, 48001, 96000, 22050, 0, -1):
        rc, _, text = preset(1, rate)
        assert rc == _native.ERR_UNSUPPORTED and "sample_rate" in text and str(rate) in text, text
    for identifier in (0, 3, -1):
        rc, _, text = preset(identifier)
        assert rc == _native.ERR_ARGUMENT and "id" in text
    assert _native.library().mgx_noise_shaper_preset(1, 44100, None) == _native.ERR_ARGUMENT
    assert "out" in _native.library().mgx_last_error().decode()


def native_gain(target, ceiling, bits, coefficients, integrated, true_peak, dither=1, shaper="given"):
    lib = _native.library()
    spec = _native.MgxDelivery(math.nan if target is None else target, math.nan if ceiling is None else ceiling, bits, dither, 0)
    report = _native.MgxLoudnessReport()
    report.integrated, report.true_peak = integrated, true_peak
    out = _native.MgxDeliveryResult()
    given = native_shaper(coefficients) if shaper == "given" else shaper
    rc = lib.mgx_delivery_gain_shaped(ctypes.byref(spec), None if given is None else ctypes.byref(given), ctypes.byref(report),
                                      ctypes.byref(out))
    return rc, out, lib.mgx_last_error().decode()


def close(a, b):
    return a == b or abs(a - b) <= 1e-12 * abs(b)


def test_head_room_is_the_stated_one():
    assert oracle.error_lsb(()) == 1.5 * (1.0 + 2.0 ** -20)
    assert close(oracle.error_lsb(oracle.LIPSHITZ5), 1.5 * 9.3619 * (1.0 + 2.0 ** -20))
    # the library's own, read back from a ceiling of -60 dBTP at 24 bit
    rc, out, text = native_gain(None, -60.0, 24, oracle.WANNAMAKER9, -20.0, 1.0)
    assert rc == 0, text
    assert close(out.gain, 1e-3 - delivery_oracle.interpolator_gain() * oracle.error_lsb(oracle.WANNAMAKER9) / 2.0 ** 23)


def test_gain_rule_against_the_oracle():
    seen = set()
    for bits in (16, 24):
        for coefficients in SHAPERS.values():
            for target in (None, -14.0, -9.5):
                for ceiling in (None, 0.0, -1.0, -3.25):
                    for integrated in (-math.inf, -30.0, -12.3, -8.0):
                        for peak in (0.0, 0.2, 0.9981, 1.31):
                            case = (target, ceiling, bits, coefficients, integrated, peak)
                            want = oracle.delivery_gain(*case)
                            rc, got, text = native_gain(*case)
                            assert rc == 0, (case, text)
                            for field in ("gain", "achieved_lufs", "achieved_true_peak", "shortfall_lu"):
                                assert close(getattr(got, field), getattr(want, field)), (case, field)
                            assert got.limited_by == want.limited_by and got.shortfall_lu >= 0.0, case
                            seen.add(got.limited_by)
    assert seen == {0, 1, 2}
    # the shaper costs head-room: under the same ceiling the shaped gain is the smaller one
    plain = delivery_oracle.delivery_gain(None, -1.0, 16, 1, -9.0, 1.2).gain
    rc, got, _ = native_gain(None, -1.0, 16, oracle.WANNAMAKER9, -9.0, 1.2)
    assert rc == 0 and got.gain < plain and got.gain > 0.99 * plain


NAN_TAP = (1.0, math.nan, 0.5)
INF_TAP = (1.0, 0.5, math.inf)


@pytest.mark.parametrize("kwargs,field", [
    (dict(shaper=None), "shaper"),
    (dict(shaper=native_shaper((), taps=17)), "taps"),
    (dict(shaper=native_shaper((), taps=-1)), "taps"),
    (dict(coefficients=NAN_TAP), "c[2]"),
    (dict(coefficients=INF_TAP), "c[3]"),
    (dict(dither=0), "dither"),
    (dict(dither=2), "dither"),
    (dict(dither=3), "dither"),
    (dict(bits=0, dither=0), "bits"),
    (dict(bits=32, dither=0), "bits"),
    (dict(bits=8), "bits"),
    (dict(ceiling=0.5), "ceiling_dbtp"),
    (dict(ceiling=-56.0), "ceiling_dbtp"),                       # 1.6e-3 of full scale: under wannamaker9's 1.8e-3 at 16 bit
    (dict(ceiling=-math.inf), "ceiling_dbtp"),
    (dict(target=math.inf), "target_lufs"),
    (dict(true_peak=math.nan), "true_peak"),
    (dict(integrated=math.nan), "integrated"),
])
def test_every_policy_refusal_names_its_field(kwargs, field):
    case = dict(target=-14.0, ceiling=-1.0, bits=16, coefficients=oracle.WANNAMAKER9, integrated=-14.0, true_peak=0.5)
    case.update(kwargs)
    rc, _, text = native_gain(**case)
    assert rc == _native.ERR_ARGUMENT and field in text, text
    # the limiter's step refuses the same
    lib = _native.library()
    spec = _native.MgxDelivery(case["target"], case["ceiling"], case["bits"], case.get("dither", 1), 0)
    report = _native.MgxLoudnessReport()
    report.integrated, report.true_peak = case["integrated"], case["true_peak"]
    given = case.get("shaper", "given")
    given = native_shaper(case["coefficients"]) if given == "given" else given
    plan = _native.MgxDeliveryLimitPlan()
    rc = lib.mgx_delivery_limit_step_shaped(ctypes.byref(spec), None if given is None else ctypes.byref(given), ctypes.byref(report),
                                            0, None, None, 4, 0.1, ctypes.byref(plan))
    assert rc == _native.ERR_ARGUMENT and field in lib.mgx_last_error().decode()


def test_null_arguments_are_refused():
    lib = _native.library()
    assert lib.mgx_delivery_gain_shaped(None, None, None, None) == _native.ERR_ARGUMENT
    assert lib.mgx_delivery_limit_step_shaped(None, None, None, 0, None, None, 4, 0.1, None) == _native.ERR_ARGUMENT
    assert "null" in lib.mgx_last_error().decode()


def as_loudness(integrated, true_peak):
    return Loudness(integrated, 0.0, integrated, integrated, true_peak, true_peak, 44100, 44100, 10, 4410)


def test_limit_step_is_the_plain_rule_with_the_shapers_ceiling():
    """mgx_delivery_limit_step_shaped: the plan's ceiling is the oracle's room, and the search is mgx_delivery_limit_step's
    (its run and pre-gains depend on the loudness alone)."""
    measured = as_loudness(-12.0, 1.2)
    for bits in (16, 24):
        for name in ("lipshitz5", "wannamaker9"):
            shaped = Delivery(loudness=-8.0, true_peak=-1.0, dither=name, limiter=mg.TruePeakLimiter())
            plain = Delivery(loudness=-8.0, true_peak=-1.0, dither="tpdf", limiter=mg.TruePeakLimiter())
            for pre, loud in (((), ()), ((4.0,), (-9.0,)), ((4.0, 5.0), (-9.0, -8.5)), ((4.0, 5.0), (-9.0, -8.95))):
                run, pre_gain, ceiling = limit_step(shaped, bits, measured, pre, loud)
                assert close(ceiling, oracle.room(-1.0, bits, SHAPERS[name]))
                assert (run, pre_gain) == limit_step(plain, bits, measured, pre, loud)[:2]
            assert ceiling < limit_step(plain, bits, measured)[2]
    # where the linear policy reaches the target nothing runs
    assert limit_step(shaped, 16, as_loudness(-12.0, 0.2))[0] is False


# ---- the ceiling ----------------------------------------------------------------------------------------------------------

def theorem_signals():
    """DESIGN.md section 3.11's inputs."""
    n = 2048
    square = np.ones((n, 2), dtype=np.float32)
    square[(np.arange(n) // 5) % 2 == 1] = -1.0                                       # full scale, period 10 frames
    alternating = np.empty((n, 2), dtype=np.float32)
    alternating[0::2], alternating[1::2] = 0.998, -0.998
    rng = np.random.RandomState(11)
    noise = (rng.randn(n, 2) * 0.3).astype(np.float32)
    burst = np.zeros((n, 2), dtype=np.float32)
    burst[100:1100, 0] = np.sign(rng.randn(1000)).astype(np.float32)                  # random signs: the interpolator's own worst
    return {"square": square, "alternating": alternating, "noise": noise, "random signs": burst}


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("name", ["lipshitz5", "wannamaker9"])
def test_the_ceiling_is_a_theorem_about_the_decoded_file(bits, name):
    for label, x in theorem_signals().items():
        true_peak, _ = loudness_oracle.peaks(x)
        for ceiling_db in (0.0, -1.0):
            rule = oracle.delivery_gain(0.0, ceiling_db, bits, SHAPERS[name], -20.0, true_peak)
            assert rule.limited_by == 2
            for seed in (0, SEED):
                values = oracle.deliver_shaped(x, rule.gain, bits, SHAPERS[name], seed)
                assert values.max() < 2 ** (bits - 1) - 1 or ceiling_db == 0.0      # nothing clips under a ceiling
                got, _ = loudness_oracle.peaks(oracle.decoded(values, bits))
                ceiling = 10.0 ** (ceiling_db / 20.0)
                print(label, ceiling_db, seed, got / ceiling)
                assert got <= ceiling * (1.0 + 1e-12), (label, ceiling_db, seed, got)
                assert got > ceiling * 0.99                                          # ... and not by giving the level away


# ---- the spectrum -----------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def prototype_input():
    """2^17 frames of a 997 Hz sine at 1000.3 LSB plus a 0.37 LSB offset, both channels."""
    t = np.arange(N_SPECTRUM)
    lsb = 1000.3 * np.sin(2.0 * np.pi * 997.0 * t / RATE) + 0.37
    return np.repeat((lsb / 32767.0).astype(np.float32)[:, None], 2, axis=1)


def expected_periodogram(coefficients):
    """E of a Hann-windowed periodogram (normalised by sum w^2) of noise with spectrum 0.25 |H|^2: the spectrum smoothed
    by the window's own power response, evaluated exactly from the error's autocorrelation."""
    h = np.concatenate([[1.0], -np.asarray(coefficients, dtype=np.float64)])
    window = np.hanning(POINTS + 1)[:POINTS]
    lags = np.arange(-(len(h) - 1), len(h))
    r = 0.25 * np.correlate(h, h, mode="full")                                      # R[l], l = -(K) .. K
    ww = np.array([np.dot(window[:POINTS - abs(l)], window[abs(l):]) for l in lags]) / np.dot(window, window)
    k = np.arange(POINTS // 2 + 1)
    return np.real(np.exp(-2j * np.pi * np.outer(k, lags) / POINTS) @ (r * ww))


def averaged_periodogram(error):
    window = np.hanning(POINTS + 1)[:POINTS]
    blocks = error.reshape(AVERAGES, POINTS) * window
    return (np.abs(np.fft.rfft(blocks, axis=1)) ** 2).mean(axis=0) / np.dot(window, window)


@pytest.mark.parametrize("name", ["lipshitz5", "wannamaker9"])
def test_error_spectrum_is_the_noise_transfer_function(prototype_input, name):
    """Segmented (the definition, on the oracle) and purely sequential (one chain per channel, on the emulation): every bin
    of the averaged periodogram of file - a within 5 / sqrt(M) of 0.25 |H|^2 smoothed by the window, the mean over the
    2-5 kHz bins within 5 / sqrt(M bins) -- the spreads of an average of M (M bins) exponentially distributed values."""
    c = SHAPERS[name]
    a, _, _ = oracle.scaled_and_dither(prototype_input, 1.0, 16, SEED)
    segmented = oracle.deliver_shaped(prototype_input, 1.0, 16, c, SEED).astype(np.float64)
    raw = emu.deliver_shaped(prototype_input, 1.0, 16, c, SEED, segment=N_SPECTRUM, warmup=0)
    sequential = delivery_oracle.unpacked(raw, 16, 2 * N_SPECTRUM).reshape(-1, 2).astype(np.float64)
    assert emu.deliver_shaped(prototype_input, 1.0, 16, c, SEED) == oracle.packed(segmented, 16)
    want = expected_periodogram(c)
    assert np.allclose(want[[0, -1]], 0.25 * oracle.ntf_power(c, [0.0, RATE / 2.0], RATE), rtol=0.5)   # (smoothing aside)
    band = [k for k in range(POINTS // 2 + 1) if 2000.0 <= k * RATE / POINTS <= 5000.0]
    assert len(band) == 18
    flat_band = 0.25
    for label, values in (("segmented", segmented), ("sequential", sequential)):
        assert not np.array_equal(values, np.clip(np.rint(a), -32768, 32767)) and np.abs(values).max() < 1100
        for ch in range(2):
            got = averaged_periodogram(values[:, ch] - a[:, ch])
            worst = np.abs(got / want - 1.0).max()
            in_band = got[band].mean() / want[band].mean() - 1.0
            print(name, label, ch, "worst bin", worst, "band", in_band, "dB under flat", 10 * np.log10(got[band].mean() / flat_band))
            assert worst <= 5.0 / math.sqrt(AVERAGES), (label, ch, worst)
            assert abs(in_band) <= 5.0 / math.sqrt(AVERAGES * len(band)), (label, ch, in_band)
            assert got[band].mean() < flat_band / 30.0                               # ~ -18 / -22 dB: the noise has left the band


# ---- the Python surface -------------------------------------------------------------------------------------------------

def test_noise_shaper_validates():
    assert NoiseShaper([1, -0.5]).coefficients == (1.0, -0.5) and NoiseShaper(()).coefficients == ()
    assert NoiseShaper((1.0,)) == NoiseShaper([1.0]) and NoiseShaper((1.0,)).preset is None
    for bad in ([math.nan], [math.inf], ["1"], [True], [0.0] * 17, 3.0, None):
        with pytest.raises(ValueError):
            NoiseShaper(bad)
    with pytest.raises(TypeError):                                                    # the name is the library's to give
        NoiseShaper((1.0,), preset="lipshitz5")
    assert NoiseShaper(oracle.LIPSHITZ5).preset is None and NoiseShaper(oracle.LIPSHITZ5) != NoiseShaper.lipshitz5()
    assert NoiseShaper.lipshitz5() is NoiseShaper.lipshitz5()                         # read from the library once
    with pytest.raises(Exception):
        NoiseShaper((1.0,)).coefficients = ()                                         # frozen
    native = NoiseShaper(K16).native()
    assert native.taps == 16 and tuple(native.c) == K16
    assert str(NoiseShaper.wannamaker9()) == "wannamaker9" and str(NoiseShaper((1.0, 2.0))) == "noise-shaped, 2 taps"


def test_delivery_takes_a_shaper():
    for dither in ("lipshitz5", "wannamaker9", NoiseShaper(K1), NoiseShaper.lipshitz5()):
        spec = Delivery(true_peak=-1.0, dither=dither, seed=5)
        assert spec.shaped and spec.native(16).dither == 1 and spec.native(24).seed == 5
        spec.check_subtype("PCM_16"), spec.check_subtype("PCM_24")
        for subtype in ("PCM_32", "FLOAT", "DOUBLE"):
            with pytest.raises(ValueError, match="dither"):
                spec.check_subtype(subtype)
            with pytest.raises(ValueError, match="dither"):
                mg.Result("a.wav", subtype, delivery=spec)
    assert Delivery(dither="lipshitz5").shaper == NoiseShaper.lipshitz5()
    assert Delivery(dither=NoiseShaper(K1)).shaper.coefficients == K1
    assert Delivery(dither="tpdf").shaper is None and not Delivery().shaped and not Delivery(dither="tpdf_hp").shaped
    for bad in ("noise", "shibata", 1, [1.0, 2.0], (1.0,), {"coefficients": [1.0]}):
        with pytest.raises(ValueError, match="dither"):
            Delivery(dither=bad)
    # the unshaped names keep their codes
    assert [Delivery(dither=d).native(16).dither for d in (None, "tpdf", "tpdf_hp")] == [0, 1, 2]


def test_from_json_takes_the_names_and_coefficients():
    assert Delivery.from_json({"dither": "lipshitz5", "true_peak": -1}) == Delivery(true_peak=-1, dither="lipshitz5")
    assert Delivery.from_json({"dither": "wannamaker9"}).shaper == NoiseShaper.wannamaker9()
    assert Delivery.from_json({"dither": {"coefficients": [1.0, -0.5]}, "seed": 3}) == Delivery(dither=NoiseShaper((1.0, -0.5)), seed=3)
    own = NoiseShaper((0.5,))
    assert Delivery.from_json({"dither": own}).dither is own and Delivery.from_json({"dither": NoiseShaper.lipshitz5()}).shaped
    for bad in ({"dither": "noise"}, {"dither": {"taps": [1.0]}}, {"dither": {"coefficients": 1.0}}, {"dither": [1.0]},
                {"dither": {"coefficients": [1.0], "preset": "lipshitz5"}}, {"dither": {"coefficients": ["a"]}}):
        with pytest.raises(ValueError):
            Delivery.from_json(bad)


def test_batch_jobs_parse_shaped_deliveries(tmp_path):
    from matchering_amd.batch import jobs_from_json

    path = tmp_path / "jobs.json"
    path.write_text(json.dumps([{"target": "t.wav", "reference": "r.wav", "results": [
        {"file": "a.wav", "delivery": {"true_peak": -1, "dither": "wannamaker9", "seed": 7}},
        {"file": "b.wav", "subtype": "PCM_24", "delivery": {"dither": {"coefficients": [0.5, -0.25]}}}]}]))
    (job,) = jobs_from_json(str(path))
    a, b = job["results"]
    assert a.delivery == Delivery(true_peak=-1, dither="wannamaker9", seed=7) and a.subtype == "PCM_16"
    assert b.delivery.shaper == NoiseShaper((0.5, -0.25)) and b.subtype == "PCM_24"
    path.write_text(json.dumps([{"target": "t.wav", "reference": "r.wav", "results": [
        {"file": "a.wav", "subtype": "PCM_32", "delivery": {"dither": "lipshitz5"}}]}]))
    with pytest.raises(ValueError, match="dither"):
        jobs_from_json(str(path))


def test_delivery_gain_and_the_record_name_the_shaper():
    measured = as_loudness(-9.0, 1.2)
    record = delivery_gain(Delivery(true_peak=-1.0, dither="wannamaker9"), 16, measured)
    want = oracle.delivery_gain(None, -1.0, 16, oracle.WANNAMAKER9, -9.0, 1.2)
    assert isinstance(record, Delivered) and close(record.gain, want.gain) and record.limited_by == "true_peak"
    assert "16 bit, wannamaker9" in str(record)
    custom = delivery_gain(Delivery(true_peak=-1.0, dither=NoiseShaper(K1)), 24, measured)
    assert close(custom.gain, oracle.delivery_gain(None, -1.0, 24, K1, -9.0, 1.2).gain) and "noise-shaped, 1 taps" in str(custom)
    assert "tpdf_hp" in str(delivery_gain(Delivery(true_peak=-1.0, dither="tpdf_hp"), 16, measured))


def test_a_refused_preset_rate_is_a_value_error_before_a_file_is_opened(tmp_path):
    """A preset at a file rate outside 44.1-48 kHz: ``process``, ``process_batch`` and ``stages.main`` raise ValueError from
    mgx_noise_shaper_preset's refusal before a file is opened or a device asked for (the files named here do not exist)."""
    from matchering_amd import stages
    from matchering_amd.batch import process_batch

    missing = str(tmp_path / "missing.wav")
    for spec, config in ((Delivery(true_peak=-1.0, dither="lipshitz5", sample_rate=96000), mg.Config()),
                         (Delivery(dither=NoiseShaper.wannamaker9(), sample_rate=32000), mg.Config()),
                         (Delivery(dither="wannamaker9"), mg.Config(internal_sample_rate=96000))):
        results = [mg.pcm16(str(tmp_path / "out.wav"), delivery=spec)]
        for run in (lambda: mg.process(missing, missing, results, config=config),
                    lambda: process_batch([{"target": missing, "reference": missing, "results": results}], config=config,
                                          rank=0, world_size=1),
                    lambda: stages.main(np.zeros((10, 2), np.float32), np.zeros((10, 2), np.float32), config,
                                        device=object(), deliveries=DeliveryRequest([("k", 0, "PCM_16", spec)]))):
            with pytest.raises(ValueError) as refused:
                run()
            assert str(spec.rate(config.internal_sample_rate)) in str(refused.value) and "44100" in str(refused.value)
    assert not os.listdir(tmp_path)
    # what the library hands out, and coefficients of one's own at any rate: no refusal, no device
    request = DeliveryRequest([("a", 0, "PCM_16", Delivery(dither="lipshitz5", sample_rate=48000)),
                               ("b", 0, "PCM_24", Delivery(dither="wannamaker9")),
                               ("c", 0, "PCM_16", Delivery(dither=NoiseShaper(oracle.LIPSHITZ5), sample_rate=96000))])
    assert request.check_rates(44100, 44100) == {48000: 48000, 96000: 96000}
