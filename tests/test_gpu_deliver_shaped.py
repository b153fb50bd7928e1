"""Noise-shaped deliveries on the GPU: mgx_deliver_shaped against tests/deliver_shaped_oracle.py byte for byte at the
sizes around a warm-up, a segment and a workgroup's tile, and a shaped delivery -- linear and limited -- through
stages.main, process and process_batch, its file read back under the ceiling.
"""

import ctypes
import os

import numpy as np
import pytest

import deliver_shaped_oracle as oracle
import delivery_oracle
import loudness_oracle
import matchering_amd as mg
from matchering_amd import _native, audio_io, stages
from matchering_amd.delivery import Delivery, DeliveryRequest, NoiseShaper, TruePeakLimiter
from matchering_amd.synth import make_pair

pytestmark = pytest.mark.gpu
B, W, TILE = oracle.SEGMENT, oracle.WARMUP, 32          # SHAPED_SEGMENTS (deliver_shaped_kernel.h; the CPU suite checks it)
SIZES = [1, 2, W - 1, W, W + 1, B - 1, B, B + 1, B + W - 1, B + W, B + W + 1, 2 * B, 3 * B + 7, TILE * B + B + 1]
SEED = 2 ** 40 + 3
RATE = 44100
PRESETS = {"lipshitz5": oracle.LIPSHITZ5, "wannamaker9": oracle.WANNAMAKER9}


@pytest.fixture(scope="module")
def dev():
    from matchering_amd.device import default_device

    return default_device()


def frames_of(n, seed):
    """(n, 2) float32 over the whole range and beyond it (they clip after the gain too), a few within an LSB of zero."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1.6, 1.6, (n, 2)).astype(np.float32)
    x[::5] *= np.float32(1e-4)
    x[0, 0] = 3.0
    return x


@pytest.fixture(scope="module")
def expected():
    """Per size: the frames, and per (bits, preset) the oracle's bytes -- computed once, read by every test."""
    table = {}
    for n in SIZES:
        x = frames_of(n, n % 1000)
        table[n] = (x, {(bits, name): oracle.packed(oracle.deliver_shaped(x, 0.77, bits, c, SEED), bits)
                        for bits in (16, 24) for name, c in PRESETS.items()})
    return table


@pytest.mark.parametrize("n", SIZES)
def test_deliver_shaped_is_the_oracle_byte_for_byte(dev, expected, n):
    x, want = expected[n]
    with dev.lock:
        buf = dev.upload(x)
        try:
            for (bits, name), raw in want.items():
                shaper = getattr(NoiseShaper, name)()
                got = dev.deliver_shaped(buf, n, 0.77, bits, shaper, SEED)
                assert got.tobytes() == raw, (n, bits, name)
                assert dev.deliver_shaped(buf, n, 0.77, bits, shaper, SEED).tobytes() == raw     # two calls, the same bytes
        finally:
            buf.release()


def test_custom_taps_and_no_taps(dev):
    n = 3 * B + 7
    x = frames_of(n, 4)
    k16 = tuple((-1.0) ** k * 0.9 / (k + 1) for k in range(16))
    with dev.lock:
        buf = dev.upload(x)
        try:
            for bits in (16, 24):
                for c in ((0.7,), k16):
                    got = dev.deliver_shaped(buf, n, 0.77, bits, NoiseShaper(c), SEED)
                    assert got.tobytes() == oracle.packed(oracle.deliver_shaped(x, 0.77, bits, c, SEED), bits), (bits, len(c))
                plain = dev.deliver(buf, n, 2, 0.77, bits, 1, SEED)
                assert dev.deliver_shaped(buf, n, 0.77, bits, NoiseShaper(()), SEED).tobytes() == plain.tobytes()
        finally:
            buf.release()


def test_refusals_leave_the_handle_usable(dev):
    lib = _native.library()
    x = frames_of(64, 3)
    good = NoiseShaper.lipshitz5().native()

    def shaper(taps, value=0.5):
        s = _native.MgxNoiseShaper()
        s.taps = taps
        for k in range(16):
            s.c[k] = value
        return s

    with dev.lock:
        buf, out = dev.upload(x), dev.alloc(64 * 2 * 3)
        try:
            def call(x_ptr=buf.ptr, frames=64, gain=0.5, bits=16, s=good, out_ptr=out.ptr, handle=dev.handle):
                rc = lib.mgx_deliver_shaped(handle, ctypes.c_void_p(x_ptr), frames, gain, bits, None if s is None else ctypes.byref(s),
                                            5, ctypes.c_void_p(out_ptr))
                return rc, lib.mgx_last_error().decode()

            refused = {"h": call(handle=None), "x_dev": call(x_ptr=None), "out_dev": call(out_ptr=None), "shaper": call(s=None),
                       "n_frames": call(frames=-1), "bits": call(bits=8), "taps": call(s=shaper(17)), "c[1]": call(s=shaper(3, np.nan)),
                       "gain": call(gain=float("nan"))}
            for field, (rc, text) in refused.items():
                assert rc == _native.ERR_ARGUMENT and field in text, (field, rc, text)
            for rc, text in (call(bits=0), call(bits=32), call(s=shaper(-1)), call(s=shaper(2, np.inf)), call(gain=float("inf"))):
                assert rc == _native.ERR_ARGUMENT
            assert "x_dev" in call(x_ptr=buf.ptr + 4)[1] and "out_dev" in call(out_ptr=out.ptr + 8)[1]
            assert call(frames=0)[0] == 0                                              # nothing to do: a success
            assert call()[0] == 0
            got = dev.download(out, (64, 2), np.int16)
            assert np.array_equal(got, oracle.deliver_shaped(x, 0.5, 16, oracle.LIPSHITZ5, 5))
        finally:
            buf.release()
            out.release()


# ---- a shaped delivery through stages.main, process and process_batch --------------------------------------------------------
CEILING_DB = -1.0
LINEAR = Delivery(true_peak=CEILING_DB, dither="wannamaker9", seed=SEED)


@pytest.fixture(scope="module")
def pair():
    return make_pair(4.0)


def read_back(array, bits):
    values = delivery_oracle.unpacked(np.ascontiguousarray(array).tobytes(), bits, array.nbytes * 8 // bits).reshape(-1, 2)
    return values, loudness_oracle.measure(delivery_oracle.decoded(values, bits), RATE)


def last_pass(dev, rendering, record, bits, coefficients, limiter):
    """The record's last limiter pass again, by hand: mgx_tp_limit of the rendering at the record's pre-gain under the
    ceiling the shaped policy hands the limiter (the oracle's ``room``).  mgx_tp_limit gives the same bytes twice."""
    n = rendering.shape[0]
    with dev.lock:
        buf = dev.upload(np.ascontiguousarray(rendering, dtype=np.float32))
        frames, _ = dev.tp_limit(buf, n, 10.0 ** (record.pre_gain_db / 20.0), oracle.room(CEILING_DB, bits, coefficients),
                                 *limiter.frames(RATE))
        limited = dev.download(frames, (n, 2), np.float32)
        buf.release(), frames.release()
    return limited


def test_main_delivers_shaped_linear_and_limited(dev, pair):
    target, reference = pair
    config = mg.Config()
    first = DeliveryRequest([("linear", 1, "PCM_16", LINEAR)])
    renderings = stages.main(target, reference, config, False, True, False, device=dev, deliveries=first)
    unlimited = renderings[1]
    plain = stages.main(target, reference, config, False, True, False, device=dev)
    assert np.array_equal(plain[1], unlimited)                                        # the rendering is not touched
    record = first.delivered["linear"]
    # the policy: the oracle's formula on the oracle's own measurement of the rendering (the meter agrees to 1e-6)
    measured = loudness_oracle.measure(unlimited.astype(np.float64), RATE)
    want = oracle.delivery_gain(None, CEILING_DB, 16, oracle.WANNAMAKER9, measured.integrated, measured.true_peak)
    assert record.limited_by == "true_peak" and abs(record.gain - want.gain) <= 1e-6 * want.gain
    assert "wannamaker9" in str(record)
    # the file: the oracle's bytes for that gain, under the ceiling when read back
    values, reading = read_back(first.arrays["linear"], 16)
    assert np.array_equal(values, oracle.deliver_shaped(unlimited, record.gain, 16, oracle.WANNAMAKER9, SEED))
    print("linear:", record, "| read back", reading.integrated, "LUFS, true peak", reading.true_peak)
    assert reading.true_peak <= 10.0 ** (CEILING_DB / 20.0) * (1.0 + 1e-9)
    assert abs(reading.integrated - record.achieved_lufs) <= 0.01

    # three LU above what linear gain reaches: the limiter runs, with the shaper's ceiling
    for bits, name in ((16, "wannamaker9"), (24, "lipshitz5")):
        spec = Delivery(loudness=record.achieved_lufs + 3.0, true_peak=CEILING_DB, dither=name, seed=7, limiter=TruePeakLimiter())
        request = DeliveryRequest([("limited", 1, f"PCM_{bits}", spec)])
        stages.main(target, reference, config, False, True, False, device=dev, deliveries=request)
        made = request.delivered["limited"]
        assert made.limiter_passes >= 1 and made.shortfall_lu < 3.0 and name in str(made) and "limited in" in str(made)
        want = oracle.delivery_gain(spec.loudness, CEILING_DB, bits, PRESETS[name], made.limited.integrated, made.limited.true_peak)
        assert abs(made.gain - want.gain) <= 1e-12 * want.gain
        # the last pass again, by hand: the file is the oracle's bytes of exactly those frames (mgx_tp_limit gives the same
        # bytes twice), with the ceiling the shaped policy hands the limiter
        limited = last_pass(dev, unlimited, made, bits, PRESETS[name], spec.limiter)
        values, reading = read_back(request.arrays["limited"], bits)
        assert np.array_equal(values, oracle.deliver_shaped(limited, made.gain, bits, PRESETS[name], 7)), name
        print(name, made, "| read back", reading.integrated, "LUFS, true peak", reading.true_peak)
        assert reading.true_peak <= 10.0 ** (CEILING_DB / 20.0) * (1.0 + 1e-9)
        assert abs(reading.integrated - made.achieved_lufs) <= 0.01


def test_process_and_a_batch_job_write_the_same_shaped_files(dev, pair, tmp_path):
    """What ``process`` and a batch job write IS the noise-shaped file: the integer samples of each file equal the oracle's
    for the rendering ``stages.main`` makes of the same pair, at the record's gain, with the delivery's shaper and seed --
    a file that lost its shaper on the way, or took another delivery's array, differs in nearly every sample."""
    import json

    from matchering_amd import batch

    target, reference = pair
    audio_io.save(str(tmp_path / "target.wav"), target, RATE, "FLOAT")
    audio_io.save(str(tmp_path / "reference.wav"), reference, RATE, "FLOAT")
    one, two = str(tmp_path / "process"), str(tmp_path / "batch")
    os.makedirs(one), os.makedirs(two)
    loud = Delivery(loudness=-9.0, true_peak=CEILING_DB, dither="wannamaker9", seed=7, limiter=TruePeakLimiter())
    records = {}
    mg.process(str(tmp_path / "target.wav"), str(tmp_path / "reference.wav"),
               [mg.pcm16(os.path.join(one, "cd.wav"), delivery=LINEAR),
                mg.Result(os.path.join(one, "loud.wav"), "PCM_16", use_limiter=False, normalize=False, delivery=loud)],
               loudness=lambda name, value: records.__setitem__(name, value))
    # the renderings of the same pair (FLOAT files hold the float32 frames as they are): cd.wav is cut from the limited
    # one (pcm16's default), loud.wav from the unlimited one
    result, unlimited, _ = stages.main(target, reference, mg.Config(), True, True, False, device=dev)
    cd, hot = (records["delivered:" + os.path.join(one, name)] for name in ("cd.wav", "loud.wav"))
    assert cd.delivery == LINEAR and cd.limiter_passes == 0 and "16 bit, wannamaker9" in str(cd)
    assert hot.delivery == loud and hot.limiter_passes >= 1 and "16 bit, wannamaker9" in str(hot) and "limited in" in str(hot)
    want = {"cd.wav": oracle.deliver_shaped(result, cd.gain, 16, oracle.WANNAMAKER9, SEED),
            "loud.wav": oracle.deliver_shaped(last_pass(dev, unlimited, hot, 16, oracle.WANNAMAKER9, loud.limiter), hot.gain, 16,
                                              oracle.WANNAMAKER9, 7)}
    for name, record in (("cd.wav", cd), ("loud.wav", hot)):
        samples, rate = audio_io.read_wav(os.path.join(one, name), pcm=True)
        assert rate == RATE and samples.dtype == np.int16
        assert np.array_equal(samples, want[name]), name
        got, _ = audio_io.read_wav(os.path.join(one, name))
        reading = loudness_oracle.measure(np.asarray(got, dtype=np.float64), RATE)
        print(name, record, "| read back", reading.integrated, "LUFS, true peak", reading.true_peak)
        assert reading.true_peak <= 10.0 ** (CEILING_DB / 20.0) * (1.0 + 1e-9)
        assert abs(reading.integrated - record.achieved_lufs) <= 0.01
    # ... which is not the TPDF file of the same gain and seed: the shaper is in the bytes
    assert np.mean(want["cd.wav"] != delivery_oracle.deliver(result, cd.gain, 16, 1, SEED)) > 0.5
    job = {"target": str(tmp_path / "target.wav"), "reference": str(tmp_path / "reference.wav"), "results": [
        {"file": os.path.join(two, "cd.wav"), "delivery": {"true_peak": CEILING_DB, "dither": "wannamaker9", "seed": SEED}},
        {"file": os.path.join(two, "loud.wav"), "subtype": "PCM_16", "use_limiter": False, "normalize": False,
         "delivery": {"loudness": -9.0, "true_peak": CEILING_DB, "dither": "wannamaker9", "seed": 7, "limiter": True}}]}
    with open(tmp_path / "jobs.json", "w") as fh:
        json.dump([job], fh)
    jobs = batch.jobs_from_json(str(tmp_path / "jobs.json"))
    assert [r.delivery for r in jobs[0]["results"]] == [LINEAR, loud]
    assert mg.process_batch(jobs, rank=0, world_size=1, lanes=1) == [0]
    for name in ("cd.wav", "loud.wav"):
        assert open(os.path.join(one, name), "rb").read() == open(os.path.join(two, name), "rb").read(), name
