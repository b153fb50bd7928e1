"""Delivery renditions on the MI355X: ``mgx_deliver`` against tests/delivery_oracle.py bit for bit (everything is float64 on
exact operands: there is no tolerance), against ``mgx_pcm_encode`` at gain 1, its refusals, and the deliveries of
``stages.main`` / ``process`` / ``process_batch`` on a 3-second synthetic pair: each written rendition holds its ceiling
and its predicted loudness as the oracle's meter reads it back.
"""

import ctypes
import os

import numpy as np
import pytest

import delivery_oracle as oracle
import loudness_oracle
import matchering_amd as mg
from matchering_amd import _native, audio_io, stages
from matchering_amd.delivery import Delivery, DeliveryRequest
from matchering_amd.synth import make_pair

pytestmark = pytest.mark.gpu

FORMATS = [(0, 0), (16, 0), (16, 1), (16, 2), (24, 0), (24, 1), (24, 2), (32, 0)]      # (bits, dither) that exist
SEEDS = (1, 2 ** 40 + 3)
GRID_THREADS = 2048 * 256           # DELIVER_GRID_MAX workgroups of 256 threads (deliver_kernel.h; the CPU suite checks it)
WRAPPING = GRID_THREADS * 2 + 515   # frames: 4 samples a thread -- 257 threads take a second quad, two samples are ragged
RATE = 44100


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
    if n > 2:
        x[1], x[2] = (1.0, -1.0), (0.0, -3.0)
    return x


def delivered(dev, buf, n, gain, bits, dither, seed):
    with dev.lock:
        return dev.deliver(buf, n, 2, gain, bits, dither, seed)


@pytest.mark.parametrize("n", [1, 2, 3, 511, 512, 513, 100003, WRAPPING])
def test_deliver_is_the_oracle_bit_for_bit(dev, n):
    x = frames_of(n, n % 1000)
    assert n != WRAPPING or 2 * n // 4 > GRID_THREADS                  # the grid really wraps at the launch's grid size
    with dev.lock:
        buf = dev.upload(x)
    try:
        for seed in (SEEDS if n != WRAPPING else SEEDS[1:]):           # (the long one once: the seed changes no path)
            for bits, dither in FORMATS:
                gain = 0.3701 if (bits + dither) % 2 else 0.77         # 3 * 0.3701 > 1: samples clip after the gain too
                got = delivered(dev, buf, n, gain, bits, dither, seed)
                want = oracle.deliver(x, gain, bits, dither, seed)
                assert got.tobytes() == oracle.packed(want, bits), (n, seed, bits, dither)
                if bits:
                    assert want.max() == 2 ** (bits - 1) - 1
    finally:
        buf.release()


def test_no_dither_at_unit_gain_is_the_plain_encoder(dev):
    x = frames_of(513, 2)
    with dev.lock:
        buf = dev.upload(x)
        try:
            for bits in (16, 24, 32):
                plain = dev.download_pcm(buf, 513, 2, bits)
                assert delivered(dev, buf, 513, 1.0, bits, 0, 99).tobytes() == plain.tobytes()
            assert np.array_equal(delivered(dev, buf, 513, 1.0, 0, 0, 0), x)
        finally:
            buf.release()


def test_refusals_leave_the_handle_usable(dev):
    lib = _native.library()
    x = frames_of(64, 3)
    with dev.lock:
        buf, out = dev.upload(x), dev.alloc(64 * 2 * 4)
        try:
            def call(x_ptr=buf.ptr, samples=128, gain=0.5, bits=16, dither=0, out_ptr=out.ptr, handle=dev.handle):
                return lib.mgx_deliver(handle, ctypes.c_void_p(x_ptr), samples, gain, bits, dither, 5, ctypes.c_void_p(out_ptr))

            refused = [call(handle=None), call(x_ptr=None), call(out_ptr=None), call(samples=-1), call(bits=8), call(bits=20),
                       call(bits=0, dither=1), call(bits=32, dither=2), call(dither=3), call(dither=-1),
                       call(gain=float("nan")), call(gain=float("inf")), call(x_ptr=buf.ptr + 4), call(out_ptr=out.ptr + 8)]
            assert refused == [_native.ERR_ARGUMENT] * len(refused)
            assert lib.mgx_last_error()
            assert call(samples=0) == 0                                                # nothing to do: a success
            assert call(dither=2) == 0
            got = dev.download(out, (64, 2), np.int16)
            assert np.array_equal(got, oracle.deliver(x, 0.5, 16, 2, 5))
        finally:
            buf.release()
            out.release()


# ---- the deliveries of stages.main, process and process_batch ----------------------------------------------------------
# The 3-second pair's limited rendering measures -6.4 LUFS with a true peak of 1.004 (+0.04 dBTP: above full scale, as a
# sample-peak limiter leaves it), the unlimited one -6.0 LUFS and 1.76 (tests/loudness_oracle.py on oracle/mastering_oracle.py's
# renderings).  So -14 LUFS / -1 dBTP is bound by the loudness (-7.6 dB puts the peak at 0.42), -5 LUFS / -1 dBTP by the
# ceiling (+1.4 dB is not there: the gain is -1.04 dB), and -0.5 dBTP alone on the unlimited rendering by the ceiling.
STREAMING = Delivery(loudness=-14.0, true_peak=-1.0)
LOUD = Delivery(loudness=-5.0, true_peak=-1.0, dither="tpdf_hp", seed=2 ** 40 + 3)
UNLIMITED = Delivery(true_peak=-0.5, dither="tpdf", seed=7)
PLAN = {"streaming.wav": (0, "PCM_24", STREAMING, "loudness"), "loud.wav": (0, "PCM_16", LOUD, "true_peak"),
        "unlimited.wav": (1, "PCM_24", UNLIMITED, "true_peak")}


@pytest.fixture(scope="module")
def pair():
    return make_pair(3.0)


def check_rendition(name, array, record):
    """``array``: the integer samples as the device packed them, or float frames read back from a file."""
    slot, subtype, spec, bound_by = PLAN[name]
    bits = int(subtype[4:])
    if array.dtype.kind in "iu":
        array = oracle.decoded(oracle.unpacked(array.tobytes(), bits, array.nbytes * 8 // bits).reshape(-1, 2), bits)
    measured = loudness_oracle.measure(array, RATE)
    print(name, record, "| read back:", measured.integrated, "LUFS, true peak", measured.true_peak)
    assert record.limited_by == bound_by and record.bits == bits and record.delivery == spec
    assert measured.true_peak <= 10.0 ** (spec.true_peak / 20.0) * (1.0 + 1e-9), name
    assert abs(measured.integrated - record.achieved_lufs) <= 0.01, name
    if bound_by == "loudness":
        assert abs(record.achieved_lufs - spec.loudness) < 1e-9 and record.shortfall_lu == 0.0
    elif spec.loudness is not None:
        assert record.shortfall_lu > 0.5 and abs(spec.loudness - record.shortfall_lu - record.achieved_lufs) < 1e-9
    return measured


def test_main_cuts_deliveries_and_changes_nothing_else(dev, pair):
    target, reference = pair
    config = mg.Config()
    request = DeliveryRequest([(name, slot, subtype, spec) for name, (slot, subtype, spec, _) in PLAN.items()])
    seen = []
    with_them = stages.main(target, reference, config, True, True, True, device=dev, deliveries=request,
                            loudness=lambda name, value: seen.append(name))
    without = stages.main(target, reference, config, True, True, True, device=dev)
    for a, b in zip(with_them, without):
        assert a.dtype == np.float32 and np.array_equal(a, b)
    assert seen == ["target", "reference", "result", "result_no_limiter", "result_no_limiter_normalized",
                    "delivered:streaming.wav", "delivered:loud.wav", "delivered:unlimited.wav"]
    assert set(request.arrays) == set(request.delivered) == set(PLAN)
    assert request.arrays["loud.wav"].dtype == np.int16 and request.arrays["streaming.wav"].shape == (target.shape[0], 6)
    for name in PLAN:
        check_rendition(name, request.arrays[name], request.delivered[name])
    # the two deliveries of the limited rendering share ONE measurement, and it is the meter's own of that rendering
    assert request.delivered["streaming.wav"].measured is request.delivered["loud.wav"].measured
    limited = loudness_oracle.measure(with_them[0], RATE)
    assert abs(request.delivered["loud.wav"].measured.integrated - limited.integrated) < 1e-6
    assert limited.true_peak > 1.0                     # the sample-peak limiter's result is above 0 dBTP; the deliveries are not
    # the device's values are the oracle's for the same gain: nothing in the plumbing touches them
    record = request.delivered["loud.wav"]
    want = oracle.deliver(with_them[0], record.gain, 16, "tpdf_hp", LOUD.seed)
    assert np.array_equal(request.arrays["loud.wav"], want)
    # a rendering that only a delivery names is computed but not returned
    only = DeliveryRequest([("unlimited.wav", 1, "PCM_24", UNLIMITED)])
    triple = stages.main(target, reference, config, True, False, False, device=dev, deliveries=only)
    assert triple[1] is None and triple[2] is None and np.array_equal(triple[0], without[0])
    assert np.array_equal(only.arrays["unlimited.wav"], request.arrays["unlimited.wav"])


def results_in(folder):
    return [mg.Result(os.path.join(folder, name), subtype, use_limiter=slot == 0, normalize=False, delivery=spec)
            for name, (slot, subtype, spec, _) in PLAN.items()] + [mg.pcm16(os.path.join(folder, "plain16.wav"))]


def check_folder(folder, records, reference_folder=None):
    for name in PLAN:
        got, rate = audio_io.read_wav(os.path.join(folder, name))
        assert rate == RATE
        check_rendition(name, np.asarray(got, dtype=np.float64), records["delivered:" + os.path.join(folder, name)])
    if reference_folder is not None:
        for name in list(PLAN) + ["plain16.wav"]:
            assert open(os.path.join(folder, name), "rb").read() == open(os.path.join(reference_folder, name), "rb").read(), name


def test_process_and_a_batch_job_write_the_deliveries(dev, pair, tmp_path):
    target, reference = pair
    audio_io.save(str(tmp_path / "target.wav"), target, RATE, "FLOAT")
    audio_io.save(str(tmp_path / "reference.wav"), reference, RATE, "FLOAT")
    one, two, bare = (str(tmp_path / name) for name in ("process", "batch", "bare"))
    for folder in (one, two, bare):
        os.makedirs(folder)
    records, lines = {}, []
    mg.log(debug_handler=lines.append)
    try:
        mg.process(str(tmp_path / "target.wav"), str(tmp_path / "reference.wav"), results_in(one),
                   loudness=lambda name, value: records.__setitem__(name, value))
    finally:
        mg.log()
    check_folder(one, records)
    said = [str(line) for line in lines if "delivery '" in str(line)]
    assert len(said) == 3 and sum("LU under the -5 LUFS target" in line for line in said) == 1
    # the ordinary result beside them is the file a run without deliveries writes
    mg.process(str(tmp_path / "target.wav"), str(tmp_path / "reference.wav"), [mg.pcm16(os.path.join(bare, "plain16.wav"))])
    assert open(os.path.join(one, "plain16.wav"), "rb").read() == open(os.path.join(bare, "plain16.wav"), "rb").read()
    # one job of a batch: the same four files, byte for byte (the same seeds write the same dither)
    done = mg.process_batch([{"target": str(tmp_path / "target.wav"), "reference": str(tmp_path / "reference.wav"),
                              "results": results_in(two)}], rank=0, world_size=1, lanes=1)
    assert done == [0]
    check_folder(two, {key.replace(one, two): value for key, value in records.items()}, reference_folder=one)
