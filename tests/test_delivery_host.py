"""Delivery renditions without a GPU: the Philox known answers, the gain rule of ``mgx_delivery_gain`` (the real libmgx.so
through ctypes against tests/delivery_oracle.py), the ceiling theorem and the dither's properties on the oracle, the
kernel's per-thread body (deliver_kernel.h) driven on the CPU by tests/emu/libmgx_emu_deliver.so bit for bit against the
oracle, and the Python plumbing: ``Delivery`` / ``Result`` validation, batch job parsing, ``core.process`` and
``process_batch`` with a stand-in behind ``main``.
"""

import ctypes
import json
import math
import os

import numpy as np
import pytest

import delivery_oracle as oracle
import emu_build
import loudness_oracle
import matchering_amd as mg
from matchering_amd import _native, audio_io
from matchering_amd.delivery import Delivered, Delivery, DeliveryRequest, delivery_gain
from matchering_amd.loudness import Loudness

P = ctypes.c_void_p
FORMATS = [(0, 0), (16, 0), (16, 1), (16, 2), (24, 0), (24, 1), (24, 2), (32, 0)]      # (bits, dither) that exist
GRID_MAX = 2048                                                                      # DELIVER_GRID_MAX (deliver_kernel.h)


@pytest.fixture(scope="module")
def emu():
    lib = emu_build.load("deliver")
    lib.emu_philox.argtypes = [P, P, P]
    lib.emu_deliver_grid.restype = ctypes.c_longlong
    lib.emu_deliver_grid.argtypes = [ctypes.c_longlong]
    lib.emu_deliver.restype = ctypes.c_longlong
    lib.emu_deliver.argtypes = [P, ctypes.c_longlong, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong, P,
                                ctypes.c_longlong]
    return lib


def aligned(nbytes, dtype=np.uint8):
    """A zeroed array of ``nbytes`` bytes on a 16-byte boundary, as device memory is."""
    raw = np.zeros(nbytes + 16, dtype=np.uint8)
    skip = (-raw.ctypes.data) % 16
    return raw[skip:skip + nbytes].view(dtype)


def signal(samples, seed):
    """Interleaved float32 samples that use the whole range and leave it: values that clip at gain 1 are among them."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1.3, 1.3, samples).astype(np.float32)
    x[::7] *= np.float32(1e-4)                                    # ... and a few within an LSB or two of zero
    if samples > 5:
        x[1], x[2], x[3], x[5] = 1.0, -1.0, 0.0, 2.5
    return x


KNOWN_ANSWERS = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                 ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                 ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                  (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers(emu):
    for counter, key, want in KNOWN_ANSWERS:
        assert oracle.philox(counter, key) == want
        out = (ctypes.c_uint32 * 4)()
        emu.emu_philox((ctypes.c_uint32 * 4)(*counter), (ctypes.c_uint32 * 2)(*key), out)
        assert tuple(out) == want
    # the vectorised form is the scalar one, block by block, for a key with both words set
    seed = (0x299f31d0 << 32) | 0xa4093822
    blocks = oracle.philox_blocks(6, 1, seed)
    for q in range(6):
        assert tuple(int(v) for v in blocks[q]) == oracle.philox((q, 0, 1, 0), (0xa4093822, 0x299f31d0))
    u = oracle.uniform(4096, 0, 5)
    assert u.min() > -0.5 and u.max() < 0.5 and np.all(u * 2.0 ** 25 == np.rint(u * 2.0 ** 25))


# ---- the policy -----------------------------------------------------------------------------------------------------

def native_gain(target, ceiling, bits, dither, integrated, true_peak, seed=0):
    lib = _native.library()
    spec = _native.MgxDelivery(math.nan if target is None else target, math.nan if ceiling is None else ceiling, bits, dither, seed)
    report = _native.MgxLoudnessReport()
    report.integrated, report.true_peak = integrated, true_peak
    out = _native.MgxDeliveryResult()
    rc = lib.mgx_delivery_gain(ctypes.byref(spec), ctypes.byref(report), ctypes.byref(out))
    return rc, out, lib.mgx_last_error().decode()


def close(a, b):
    return a == b or abs(a - b) <= 1e-12 * abs(b)


def test_version():
    assert _native.library().mgx_version() >= 105


def test_interpolator_gain_is_computed_from_the_taps():
    a = oracle.interpolator_gain()
    assert abs(a - 1.7629445505) < 1e-9                                              # phase 2 of sinc(k/4) kaiser(49, 8.0)
    taps = np.abs(loudness_oracle.true_peak_taps())
    assert a == taps[2::4].sum() and taps[0::4].sum() == 1.0
    # the library's own, read back from a ceiling of -80 dBTP, where the head-room 1.5 A / 2^15 is most of the ceiling
    # (no cancellation: the difference below is exact to 1e-20 of 8e-5)
    rc, out, _ = native_gain(None, -80.0, 16, 1, -20.0, 1.0)
    assert rc == 0 and abs((10.0 ** -4.0 - out.gain) * 2.0 ** 15 / 1.5 - a) <= 1e-12


def test_gain_rule_against_the_oracle():
    inf = math.inf
    cases = []
    for bits, dither in FORMATS:
        for target in (None, -14.0, -23.0, -9.5):
            for ceiling in (None, 0.0, -1.0, -3.25):
                for integrated in (-inf, -30.0, -12.3, -8.0):
                    for peak in (0.0, 0.2, 0.9981, 1.31):
                        cases.append((target, ceiling, bits, dither, integrated, peak))
    seen = set()
    for case in cases:
        want = oracle.delivery_gain(*case)
        rc, got, text = native_gain(*case)
        assert rc == 0, (case, text)
        for field in ("gain", "achieved_lufs", "achieved_true_peak", "shortfall_lu"):
            assert close(getattr(got, field), getattr(want, field)), (case, field, getattr(got, field), getattr(want, field))
        assert got.limited_by == want.limited_by and got.shortfall_lu >= 0.0, case
        seen.add(got.limited_by)
    assert seen == {0, 1, 2}


def test_gain_rule_by_hand():
    # target only: plain R 128 normalisation
    rc, out, _ = native_gain(-14.0, None, 24, 0, -20.0, 0.5)
    assert rc == 0 and close(out.gain, 10.0 ** 0.3) and out.limited_by == 1 and out.shortfall_lu == 0.0
    assert close(out.achieved_lufs, -14.0) and close(out.achieved_true_peak, 0.5 * 10.0 ** 0.3)
    # ceiling only, binding: the peak comes down to the ceiling less the head-room; not binding: nothing changes
    margin = oracle.interpolator_gain() * 1.5 / 2.0 ** 15
    rc, out, _ = native_gain(None, -1.0, 16, 1, -9.0, 1.2)
    assert rc == 0 and close(out.gain, (10.0 ** -0.05 - margin) / 1.2) and out.limited_by == 2 and out.shortfall_lu == 0.0
    rc, out, _ = native_gain(None, -1.0, 16, 1, -9.0, 0.3)
    assert rc == 0 and out.gain == 1.0 and out.limited_by == 0 and out.achieved_lufs == -9.0
    # both, the loudness binding
    rc, out, _ = native_gain(-16.0, -1.0, 24, 2, -12.0, 0.9)
    assert rc == 0 and close(out.gain, 10.0 ** -0.2) and out.limited_by == 1 and out.shortfall_lu == 0.0
    # both, the ceiling binding: the shortfall is what is missing to the target
    rc, out, _ = native_gain(-9.0, -1.0, 24, 0, -14.0, 0.8)
    g_peak = (10.0 ** -0.05 - oracle.interpolator_gain() * 0.5 / 2.0 ** 23) / 0.8
    assert rc == 0 and close(out.gain, g_peak) and out.limited_by == 2
    assert close(out.shortfall_lu, -9.0 - out.achieved_lufs) and out.shortfall_lu > 3.0
    # float output has no quantiser: no head-room
    rc, out, _ = native_gain(None, -2.0, 0, 0, -14.0, 1.0)
    assert rc == 0 and close(out.gain, 10.0 ** -0.1)
    # silence: no loudness to move; a zero peak: no ceiling to hold
    rc, out, _ = native_gain(-14.0, -1.0, 16, 0, -math.inf, 0.0)
    assert rc == 0 and out.gain == 1.0 and out.achieved_lufs == -math.inf and out.limited_by == 0 and out.shortfall_lu == 0.0
    rc, out, _ = native_gain(-14.0, -1.0, 16, 0, -math.inf, 0.5)                      # less than 400 ms, but it peaks
    assert rc == 0 and out.gain == 1.0 and out.limited_by == 0
    rc, out, _ = native_gain(-14.0, -1.0, 16, 0, -math.inf, 1.5)
    assert rc == 0 and out.gain < 1.0 and out.limited_by == 2 and out.shortfall_lu == 0.0
    rc, out, _ = native_gain(None, None, 16, 0, -14.0, 0.5)                           # nothing asked for
    assert rc == 0 and out.gain == 1.0 and out.limited_by == 0


@pytest.mark.parametrize("case,field", [
    ((None, 0.5, 16, 0, -14.0, 0.5), "ceiling_dbtp"),            # above 0 dBTP
    ((None, -100.0, 16, 1, -14.0, 0.5), "ceiling_dbtp"),         # 1e-5 of full scale: under the head-room of 8e-5
    ((None, -math.inf, 16, 0, -14.0, 0.5), "ceiling_dbtp"),
    ((math.inf, None, 16, 0, -14.0, 0.5), "target_lufs"),
    ((-14.0, None, 8, 0, -14.0, 0.5), "bits"),
    ((-14.0, None, 20, 0, -14.0, 0.5), "bits"),
    ((-14.0, None, 0, 1, -14.0, 0.5), "dither"),
    ((-14.0, None, 32, 2, -14.0, 0.5), "dither"),
    ((-14.0, None, 16, 3, -14.0, 0.5), "dither"),
    ((-14.0, None, 16, 0, -14.0, math.inf), "true_peak"),
    ((-14.0, None, 16, 0, -14.0, math.nan), "true_peak"),
    ((-14.0, None, 16, 0, math.nan, 0.5), "integrated"),
])
def test_every_refusal_names_its_field(case, field):
    rc, _, text = native_gain(*case)
    assert rc == _native.ERR_ARGUMENT and field in text, text
    with pytest.raises(ValueError, match=field):
        oracle.delivery_gain(*case)
    lib = _native.library()
    assert lib.mgx_delivery_gain(None, None, None) == _native.ERR_ARGUMENT


# ---- the theorem and the dither, on the oracle --------------------------------------------------------------------------

def theorem_signals():
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
@pytest.mark.parametrize("kind", [None, "tpdf", "tpdf_hp"])
def test_the_ceiling_is_a_theorem_about_the_decoded_file(bits, kind):
    for name, x in theorem_signals().items():
        true_peak, _ = loudness_oracle.peaks(x)
        for ceiling_db in (0.0, -1.0):
            # (a target far above: the ceiling binds, which is the case the theorem is about)
            rule = oracle.delivery_gain(0.0, ceiling_db, bits, kind, -20.0, true_peak)
            assert rule.limited_by == 2
            for seed in (0, 2 ** 40 + 3):
                values = oracle.deliver(x, rule.gain, bits, kind, seed)
                got, _ = loudness_oracle.peaks(oracle.decoded(values, bits))
                ceiling = 10.0 ** (ceiling_db / 20.0)
                assert got <= ceiling * (1.0 + 1e-12), (name, ceiling_db, seed, got)
                assert got > ceiling * 0.99                                          # ... and not by giving the level away

def test_dither_makes_the_quantiser_linear_and_its_noise_constant():
    n = 1 << 18
    top = 32767.0
    rounded = []
    for a_lsb in (0.1, 0.3, 0.5, 0.77, 2.25):
        x = np.full(n, a_lsb / top, dtype=np.float32)
        a = float(x[0]) * 1.0 * top                                                   # what the quantiser sees, in LSB
        for kind in ("tpdf", "tpdf_hp"):
            v = oracle.deliver(x, 1.0, 16, kind, seed=9).astype(np.float64)
            standard_error = v.std() / math.sqrt(n)
            assert abs(v.mean() - a) <= 5.0 * standard_error, (a_lsb, kind, v.mean(), a)
            # mean square error 1/4 LSB^2 whatever a is (1/6 of triangular dither + 1/12 of rounding); its estimate from
            # 2^18 samples of magnitude < 1.5 scatters by < 1.5^2 / 512 = 0.0044: 0.02 is 4.5 of those
            assert abs(np.mean((v - a) ** 2) - 0.25) <= 0.02, (a_lsb, kind)
        v = oracle.deliver(x, 1.0, 16, None).astype(np.float64)                       # rounding alone fails both
        assert v.std() == 0.0 and abs(v.mean() - a) > 0.09
        rounded.append(float(np.mean((v - a) ** 2)))
    assert max(rounded) - min(rounded) > 0.2                                          # ... its error depends on the input


def test_high_passed_dither_has_less_noise_at_low_frequencies():
    n = 1 << 18
    x = np.full(n, 0.3 / 32767.0, dtype=np.float32)
    low = {}
    for kind in ("tpdf", "tpdf_hp"):
        error = oracle.deliver(x, 1.0, 16, kind, seed=3).astype(np.float64)[0::2]     # one channel
        spectrum = np.abs(np.fft.rfft(error - error.mean())) ** 2
        low[kind] = spectrum[1:len(error) // 8].sum()                                 # below fs / 8
        total = spectrum[1:].sum()
        assert abs(total / (len(error) ** 2 / 2.0) - 0.25) < 0.02                     # the same total power: 1/4 LSB^2
    assert low["tpdf_hp"] < 0.5 * low["tpdf"]


# ---- the kernel's body on the CPU ---------------------------------------------------------------------------------------

def emulated(emu, x, gain, bits, dither, seed, grid=0):
    samples = x.size
    source = aligned(4 * samples, np.float32)
    source[:] = x
    nbytes = samples * (bits // 8 if bits else 4)
    out = aligned(nbytes + 16)                                                        # 16 guard bytes behind the output
    out[:] = 0xA5
    used = emu.emu_deliver(source.ctypes.data_as(P), samples, gain, bits, dither, seed, out.ctypes.data_as(P), grid)
    assert np.all(out[nbytes:] == 0xA5), "the kernel wrote behind its output"
    return bytes(out[:nbytes]), used


@pytest.mark.parametrize("samples", [2, 4, 6, 1022, 1024, 1026, 200006])
def test_emulated_kernel_is_the_oracle_bit_for_bit(emu, samples):
    x = signal(samples, samples)
    for seed in (0, 1, 2 ** 40 + 3):
        for gain in (1.0, 0.3701):
            for bits, dither in FORMATS:
                want = oracle.packed(oracle.deliver(x, gain, bits, dither, seed), bits)
                got, grid = emulated(emu, x, gain, bits, dither, seed)
                assert got == want, (samples, seed, gain, bits, dither)
                assert grid == emu.emu_deliver_grid(samples) == min(GRID_MAX, max(1, -(-(samples // 4) // 256)))
    # the same launch with three workgroups: every thread wraps around the grid
    if samples > 4096:
        for bits, dither in FORMATS:
            want = oracle.packed(oracle.deliver(x, 0.3701, bits, dither, 7), bits)
            assert emulated(emu, x, 0.3701, bits, dither, 7, grid=3)[0] == want


def test_emulated_kernel_clips_and_matches_the_plain_encoder(emu):
    """At gain 1 without dither the values are the host codec's (audio_io._quantise: what mgx_pcm_encode reproduces), the
    clipped ones included."""
    x = signal(1026, 4)
    assert np.abs(x).max() > 1.0
    for bits in (16, 24, 32):
        got = oracle.unpacked(emulated(emu, x, 1.0, bits, 0, 0)[0], bits, x.size)
        assert np.array_equal(got, audio_io._quantise(x, bits).astype(np.int64))
        assert got.max() == 2 ** (bits - 1) - 1 and got.min() == -2 ** (bits - 1)
    assert emu.emu_deliver_grid(4 * 256 * GRID_MAX + 4) == GRID_MAX                    # longer tracks wrap


# ---- Python: validation, parsing, process ----------------------------------------------------------------------------------

def test_delivery_validates_like_the_library():
    assert Delivery() == Delivery(None, None, None, 0)
    for bad in (dict(true_peak=0.1), dict(loudness=math.inf), dict(true_peak=math.nan), dict(dither="noise"),
                dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5), dict(loudness="loud")):
        with pytest.raises(ValueError):
            Delivery(**bad)
    with pytest.raises(Exception):
        Delivery().loudness = -3.0                                                    # frozen
    spec = Delivery(-14.0, -1.0, "tpdf_hp", 2 ** 40 + 3).native(16)
    assert (spec.target_lufs, spec.ceiling_dbtp, spec.bits, spec.dither, spec.seed) == (-14.0, -1.0, 16, 2, 2 ** 40 + 3)
    assert math.isnan(Delivery().native(0).target_lufs) and math.isnan(Delivery().native(0).ceiling_dbtp)


def test_result_takes_a_delivery_and_is_unchanged_without_one():
    plain = mg.Result("a.wav", "PCM_16")
    assert plain.delivery is None and repr(plain) == "Result('a.wav', 'PCM_16', use_limiter=True, normalize=True)"
    assert repr(mg.pcm24("b.wav")) == "Result('b.wav', 'PCM_24', use_limiter=True, normalize=True)"
    spec = Delivery(loudness=-14.0, true_peak=-1.0, dither="tpdf")
    assert mg.pcm16("a.wav", delivery=spec).delivery is spec and mg.pcm24("a.wav", delivery=spec).delivery is spec
    assert "delivery=Delivery(loudness=-14.0" in repr(mg.pcm16("a.wav", delivery=spec))
    assert mg.Result("a.aiff", "FLOAT", delivery=Delivery(loudness=-14.0)).delivery.loudness == -14.0
    for subtype in ("PCM_32", "FLOAT", "DOUBLE", "PCM_U8"):
        with pytest.raises(ValueError, match="dither"):
            mg.Result("a.wav", subtype, delivery=spec)
        with pytest.raises(ValueError, match="dither"):
            DeliveryRequest([("a.wav", 0, subtype, spec)])
    with pytest.raises(ValueError, match="WAVE"):
        mg.Result("a.aiff", "PCM_16", delivery=Delivery(loudness=-14.0))
    with pytest.raises(TypeError):
        mg.Result("a.wav", "PCM_16", delivery={"loudness": -14.0})
    with pytest.raises(TypeError):                                                    # the reference's own errors come first
        mg.Result("a.xyz", "PCM_16", delivery=spec)


def test_batch_jobs_parse_deliveries(tmp_path):
    from matchering_amd.batch import jobs_from_json

    path = tmp_path / "jobs.json"
    path.write_text(json.dumps([{"target": "t.wav", "reference": "r.wav", "results": [
        {"file": "a.wav", "subtype": "PCM_24", "delivery": {"loudness": -14, "true_peak": -1}},
        {"file": "b.wav", "delivery": {"dither": "tpdf_hp", "seed": 7}},
        {"file": "c.wav", "subtype": "FLOAT", "use_limiter": False}]}]))
    (job,) = jobs_from_json(str(path))
    a, b, c = job["results"]
    assert a.delivery == Delivery(loudness=-14, true_peak=-1) and a.subtype == "PCM_24"
    assert b.delivery == Delivery(dither="tpdf_hp", seed=7) and b.subtype == "PCM_16" and c.delivery is None
    path.write_text(json.dumps([{"target": "t.wav", "reference": "r.wav", "results": [
        {"file": "a.wav", "delivery": {"lufs": -14}}]}]))
    with pytest.raises(ValueError, match="lufs"):
        jobs_from_json(str(path))
    path.write_text(json.dumps([{"target": "t.wav", "reference": "r.wav", "results": [
        {"file": "a.wav", "subtype": "FLOAT", "delivery": {"dither": "tpdf"}}]}]))
    with pytest.raises(ValueError, match="dither"):
        jobs_from_json(str(path))


def as_loudness(measured, rate, frames):
    return Loudness(measured.integrated, measured.range, measured.momentary_max, measured.short_term_max, measured.true_peak,
                    measured.sample_peak, rate, frames, len(measured.sub_energy), loudness_oracle.sub_block_frames(rate))


def stand_in_main(calls):
    """``stages.main`` for the CPU suite: the renderings are the target at three levels; the deliveries are cut from them
    by the oracle, with the library's own ``mgx_delivery_gain``."""
    def main(target, reference, config, need_default=True, need_no_limiter=False, need_no_limiter_normalized=False,
             encodings=None, deliveries=None, **_):
        target = audio_io.pcm_to_float(np.asarray(target), np.float32)
        renderings = [np.ascontiguousarray(target * np.float32(g)) for g in (0.9, 1.4, 0.7)]
        calls.append({"needs": (need_default, need_no_limiter, need_no_limiter_normalized), "encodings": encodings,
                      "deliveries": deliveries})
        if deliveries:
            for key, slot, subtype, spec in deliveries.items:
                measured = as_loudness(loudness_oracle.measure(renderings[slot], 44100), 44100, target.shape[0])
                bits = {"PCM_16": 16, "PCM_24": 24, "PCM_32": 32}.get(subtype, 0)
                record = delivery_gain(spec, bits, measured)
                values = oracle.deliver(renderings[slot], record.gain, bits, spec.dither, spec.seed)
                deliveries.delivered[key] = record
                deliveries.arrays[key] = (values if bits == 0 else values.astype(np.int16) if bits == 16 else
                                          values.astype(np.int32) if bits == 32 else
                                          np.frombuffer(oracle.packed(values, 24), dtype=np.uint8).reshape(-1, 6))
        return tuple(r if need else None for r, need in zip(renderings, calls[-1]["needs"]))
    return main


def pair_files(tmp_path):
    from matchering_amd.synth import make_pair

    t, r = make_pair(5.0, 44100, pair=3, reference_seconds=4.0)
    audio_io.write_wav(str(tmp_path / "t.wav"), t, 44100, "FLOAT")
    audio_io.write_wav(str(tmp_path / "r.wav"), r, 44100, "FLOAT")
    return t.astype(np.float32)


def check_written(tmp_path, target, records):
    """The three delivered files of the two tests below hold what the oracle makes of the stand-in's renderings."""
    streaming, cd, loud = (records[str(tmp_path / name)] for name in ("streaming.wav", "cd.wav", "loud.wav"))
    assert isinstance(streaming, Delivered) and streaming.bits == 24 and cd.bits == 16 and loud.bits == 0
    assert cd.gain == 1.0 and cd.limited_by is None
    for name, record, slot_gain in (("streaming.wav", streaming, 0.9), ("cd.wav", cd, 0.9), ("loud.wav", loud, 1.4)):
        rendering = np.ascontiguousarray(target * np.float32(slot_gain))
        spec = record.delivery
        want = oracle.decoded(oracle.deliver(rendering, record.gain, record.bits, spec.dither, spec.seed), record.bits)
        got, rate = audio_io.read_wav(str(tmp_path / name))
        assert rate == 44100 and np.array_equal(np.asarray(got, dtype=np.float64), want), name
        measured = loudness_oracle.measure(want, 44100)
        assert abs(measured.integrated - record.achieved_lufs) <= 0.01
        if spec.true_peak is not None:
            # (float32 frames are rounded once more, by at most 2^-25 of a sample each: A 2^-25 of the ceiling)
            slack = 1e-12 if record.bits else oracle.interpolator_gain() * 2.0 ** -25
            assert measured.true_peak <= 10.0 ** (spec.true_peak / 20.0) * (1.0 + slack)
    assert streaming.limited_by == "loudness" and abs(streaming.achieved_lufs + 23.0) < 1e-9
    assert loud.limited_by == "true_peak" and loud.shortfall_lu > 0.0 and "under the -3 LUFS target" in str(loud)


def results_for(tmp_path):
    return [mg.pcm24(str(tmp_path / "streaming.wav"), delivery=Delivery(loudness=-23.0, true_peak=-1.0)),
            mg.pcm16(str(tmp_path / "cd.wav"), delivery=Delivery(dither="tpdf_hp", seed=2 ** 40 + 3)),
            mg.Result(str(tmp_path / "loud.wav"), "FLOAT", use_limiter=False, normalize=False,
                      delivery=Delivery(loudness=-3.0, true_peak=-0.5)),
            mg.pcm16(str(tmp_path / "plain16.wav")),
            mg.Result(str(tmp_path / "normalized.wav"), "FLOAT", use_limiter=False)]


def test_process_hands_deliveries_to_main_and_writes_them(tmp_path, monkeypatch):
    from matchering_amd import core

    target = pair_files(tmp_path)
    calls, seen, lines = [], [], []
    monkeypatch.setattr(core, "main", stand_in_main(calls))
    monkeypatch.setattr(core, "_gpu", lambda: None)
    mg.log(debug_handler=lines.append)
    try:
        mg.process(str(tmp_path / "t.wav"), str(tmp_path / "r.wav"), results_for(tmp_path), config=mg.Config(max_piece_size=2))
    finally:
        mg.log()
    (call,) = calls
    # the ordinary results alone decide what main returns and how it is encoded; the deliveries ride in the request
    assert call["needs"] == (True, False, True) and call["encodings"] == ("PCM_16", None, None)
    request = call["deliveries"]
    assert [(os.path.basename(k), slot, subtype) for k, slot, subtype, _ in request.items] == [
        ("streaming.wav", 0, "PCM_24"), ("cd.wav", 0, "PCM_16"), ("loud.wav", 1, "FLOAT")]
    assert request.needs() == (True, True, False)
    check_written(tmp_path, target, request.delivered)
    got, _ = audio_io.read_wav(str(tmp_path / "plain16.wav"))                          # today's route, untouched
    assert np.array_equal(got, audio_io._quantise(target * np.float32(0.9), 16).reshape(-1, 2) / 32768.0)
    got, _ = audio_io.read_wav(str(tmp_path / "normalized.wav"))
    assert np.array_equal(got, target * np.float32(0.7))
    said = [line for line in lines if "delivery '" in str(line)]
    assert len(said) == 3 and any("LU under the -3 LUFS target" in str(line) for line in said)
    assert all("LUFS" in str(line) and "dBTP" in str(line) and "gain" in str(line) for line in said)
    # without deliveries main is called exactly as before: no such keyword at all
    calls.clear()
    monkeypatch.setattr(core, "main", lambda *a, **k: calls.append(k) or stand_in_main([])(*a, **k))
    mg.process(str(tmp_path / "t.wav"), str(tmp_path / "r.wav"), [mg.pcm16(str(tmp_path / "again.wav"))],
               config=mg.Config(max_piece_size=2))
    assert "deliveries" not in calls[0] and calls[0]["encodings"] == ("PCM_16", None, None)


def test_process_batch_hands_deliveries_to_main_and_writes_them(tmp_path):
    target = pair_files(tmp_path)
    calls = []
    job = {"target": str(tmp_path / "t.wav"), "reference": str(tmp_path / "r.wav"), "results": results_for(tmp_path)}
    done = mg.process_batch([job], config=mg.Config(max_piece_size=2), rank=0, world_size=1, lanes=1,
                            master=stand_in_main(calls))
    assert done == [0] and calls[0]["needs"] == (True, False, True)
    check_written(tmp_path, target, calls[0]["deliveries"].delivered)
    assert os.path.exists(tmp_path / "plain16.wav") and os.path.exists(tmp_path / "normalized.wav")
