"""The deliveries' sample-rate converter on the MI355X (``mgx_convert_rate``): bit for bit ``mgx_resample`` of two channels
on the same frames -- its oracle on the device, no tolerance -- the host resampler under tests/test_gpu_resample.py's
acceptance rule, the plan cache both entry points share, the refusals, and deliveries at another rate than the internal
one through ``stages.main``, ``process`` and ``process_batch``: each written rendition holds its ceiling and its
predicted loudness as the oracle's meter reads it back AT THE FILE'S RATE.
"""

import ctypes
import os

import numpy as np
import pytest

import delivery_oracle
import loudness_oracle
import matchering_amd as mg
from matchering_amd import _native, audio_io, stages
from matchering_amd import device as device_module
from matchering_amd import resample as host
from matchering_amd.delivery import Delivery, DeliveryRequest, TruePeakLimiter
from matchering_amd.synth import make_pair

pytestmark = pytest.mark.gpu

PAIRS = [(44100, 48000), (48000, 44100), (44100, 96000), (96000, 44100), (44100, 88200), (96000, 48000), (192000, 44100),
         (44100, 8000)]
SPAN_MAX = 7680                     # RESAMPLE_SPAN_MAX
SPAN_SHARED = 5120                  # CONVERT_RATE_SPAN_MAX
RATE = 44100


@pytest.fixture(scope="module")
def dev():
    from matchering_amd.device import default_device

    return default_device()


def tiling(dev, sr, new):
    """(P, S, M) restated from the plan's L and W: S = L ceil(256 / L); P the largest of 8, 4, 2 whose span
    P (S / L) M + W fits 5120 frames, else 1."""
    _, L, W, _ = dev.resample_plan(sr, new)
    g = int(np.gcd(sr, new))
    assert L == new // g
    M = sr // g
    S = L * -(-256 // L)
    P = next(P for P in (8, 4, 2, 1) if P * (S // L) * M + W <= (SPAN_SHARED if P > 1 else SPAN_MAX))
    return P, S, M


def length(n, sr, new):
    return int(n * (float(new) / sr))


def inputs_for(n_out, sr, new):
    """The shortest input that gives n_out outputs -- or, where the ratio steps over n_out, the next count it gives."""
    n = max(0, int(n_out * sr / new) - 2)
    while length(n, sr, new) < n_out:
        n += 1
    return n


def both(dev, buf, n, sr, new):
    """(mgx_convert_rate, mgx_resample with two channels) of the first n frames of ``buf``."""
    with dev.lock:
        new_frames = dev.convert_rate(buf, n, sr, new)
        old_frames = dev.resample_frames(buf, n, 2, sr, new)
        try:
            assert new_frames.frames == old_frames.frames == length(n, sr, new)
            got = np.array(dev.download(new_frames.buf, (new_frames.frames, 2)))
            want = np.array(dev.download(old_frames.buf, (old_frames.frames, 2)))
        finally:
            new_frames.release()
            old_frames.release()
    return got, want


@pytest.mark.parametrize("sr,new", PAIRS)
def test_convert_rate_is_mgx_resample_bit_for_bit(dev, sr, new):
    with dev.lock:
        seed = dev.upload(np.zeros((64, 2), dtype=np.float32))
        dev.convert_rate(seed, 64, sr, new).release()                  # (the plan exists from here on)
        seed.release()
    P, S, M = tiling(dev, sr, new)
    tile = P * S
    lengths = sorted({1, 5, M - 1, M, M + 1, inputs_for(tile - 1, sr, new), inputs_for(tile, sr, new),
                      inputs_for(tile + 1, sr, new), inputs_for(2 * tile + 1, sr, new), inputs_for(3 * tile + 77, sr, new)})
    assert length(lengths[-1], sr, new) >= 3 * tile + 77
    x = (0.3 * np.random.RandomState(sr % 1013 + new % 101).randn(lengths[-1], 2)).astype(np.float32)
    with dev.lock:
        buf = dev.upload(x)
    try:
        for n in lengths:
            if n < 1:
                continue
            got, want = both(dev, buf, n, sr, new)
            assert np.array_equal(got, want), (sr, new, P, S, n, int(np.count_nonzero(got != want)))
            if n == lengths[-1]:
                assert float(np.abs(want).max()) > 0.1                 # (not two buffers of zeros)
    finally:
        buf.release()


def float64_bound(sr, new, peak):
    """max|x| (sum|w| W 2^-53 + W 2e-15), from the host plan of the same rates (tests/test_gpu_resample.py)."""
    plan = host._Plan(sr, new)
    g = int(np.gcd(sr, new))
    proto, _ = host._prototype(plan, new // g, sr // g)
    width = 2 * plan.taps
    row_sum = max(float(np.abs(proto[p::new // g]).sum()) for p in range(new // g))
    return peak * (row_sum * width * 2.0 ** -53 + width * 2e-15)


@pytest.mark.parametrize("sr,new", PAIRS)
def test_convert_rate_is_the_host_resampler(dev, sr, new):
    """The acceptance rule of tests/test_gpu_resample.py: each sample within one float32 spacing of float32(host) plus
    the float64 bound, at most 1 in 10 000 different from float32(host) at all."""
    n = sr // 2 + 77
    x = (0.3 * np.random.RandomState(new % 1009).randn(n, 2)).astype(np.float32)
    with dev.lock:
        buf = dev.upload(x)
        frames = dev.convert_rate(buf, n, sr, new)
        got = np.array(dev.download(frames.buf, (frames.frames, 2)))
        buf.release()
        frames.release()
    want64 = host.resample(x.astype(np.float64), sr, new)
    want = want64.astype(np.float32)
    assert got.shape == want.shape and want.shape[0] == length(n, sr, new)
    error = np.abs(got.astype(np.float64) - want.astype(np.float64))
    allowed = np.spacing(np.abs(want)).astype(np.float64) + float64_bound(sr, new, float(np.abs(x).max()))
    different = int(np.count_nonzero(got != want))
    print(f"{sr} -> {new}: max error {error.max():.3e}, {different} of {want.size} differ from float32(host)")
    assert np.all(error <= allowed), float((error - allowed).max())
    assert different * 10000 <= want.size, (different, want.size)


def test_both_entry_points_share_one_plan():
    from matchering_amd._native import MgxError
    from matchering_amd.device import Device

    own = Device(0)
    try:
        x = (0.3 * np.random.RandomState(1).randn(3000, 2)).astype(np.float32)
        with own.lock:
            buf = own.upload(x)
            with pytest.raises(MgxError):
                own.resample_plan(44100, 48000)                       # nothing converted on this handle yet
            first = own.convert_rate(buf, 3000, 44100, 48000)
            address, phases, width, designed = own.resample_plan(44100, 48000)
            assert address and (phases, width, designed) == (160, 130, 1)
            second = own.resample_frames(buf, 3000, 2, 44100, 48000)
            assert own.resample_plan(44100, 48000) == (address, 160, 130, 1)
            assert np.array_equal(own.download(first.buf, (first.frames, 2)), own.download(second.buf, (second.frames, 2)))
            # ... and the other way round, for another pair
            third = own.resample_frames(buf, 3000, 2, 48000, 44100)
            assert own.resample_plan(48000, 44100)[1:] == (147, 140, 2)
            fourth = own.convert_rate(buf, 3000, 48000, 44100)
            assert own.resample_plan(48000, 44100)[1:] == (147, 140, 2)
            assert np.array_equal(own.download(third.buf, (third.frames, 2)), own.download(fourth.buf, (fourth.frames, 2)))
            for b in (buf, first, second, third, fourth):
                b.release()
    finally:
        own.close()


def test_refusals_leave_the_handle_usable(dev):
    from matchering_amd._native import ERR_UNSUPPORTED, MgxError

    lib = device_module.library()
    x = (0.3 * np.random.RandomState(2).randn(1000, 2)).astype(np.float32)
    with dev.lock:
        buf = dev.upload(x)
        small = dev.alloc(8 * 100)
        try:
            with pytest.raises(MgxError) as refused:
                dev.convert_rate(buf, 1000, 44100, 44056)                 # 11014 phases
            assert refused.value.code == ERR_UNSUPPORTED and "44100 -> 44056" in str(refused.value)
            with pytest.raises(MgxError) as equal:
                dev.convert_rate(buf, 1000, 44100, 44100)
            assert equal.value.code == _native.ERR_ARGUMENT
            n_out = ctypes.c_int64()
            rc = lib.mgx_convert_rate(dev.handle, ctypes.c_void_p(buf.ptr), 1000, 48000, 44100, ctypes.c_void_p(small.ptr),
                                      100, ctypes.byref(n_out))
            assert rc == _native.ERR_ARGUMENT and n_out.value == 918      # capacity too small, the length reported
            empty = dev.convert_rate(buf, 1, 48000, 44100)                # n_out == 0: a success that launches nothing
            assert empty.frames == 0
            empty.release()
            got, want = both(dev, buf, 1000, 48000, 44100)                # the handle works as before
            assert got.shape == (918, 2) and np.array_equal(got, want)
        finally:
            buf.release()
            small.release()
    with pytest.raises(ValueError, match="44056"):
        device_module.delivery_length(1000, 44100, 44056)


# ---- deliveries at another rate through stages.main, process and process_batch ---------------------------------------------
STREAMING = Delivery(loudness=-14.0, true_peak=-1.0, sample_rate=48000)
CD_48 = Delivery(true_peak=-0.5, dither="tpdf_hp", seed=2 ** 40 + 3, sample_rate=48000)
HIRES = Delivery(true_peak=-1.0, sample_rate=96000)
HOME = Delivery(true_peak=-1.0, dither="tpdf", seed=7, sample_rate=RATE)
PLAN = {"streaming48.wav": ("PCM_24", STREAMING), "cd48.wav": ("PCM_16", CD_48), "hires96.wav": ("FLOAT", HIRES),
        "home.wav": ("PCM_16", HOME)}


@pytest.fixture(scope="module")
def pair():
    return make_pair(3.0)


def read_back(array, subtype, rate):
    if array.dtype.kind in "iu":
        bits = int(subtype[4:])
        array = delivery_oracle.decoded(delivery_oracle.unpacked(array.tobytes(), bits, array.nbytes * 8 // bits).reshape(-1, 2), bits)
    return loudness_oracle.measure(np.asarray(array, dtype=np.float64), rate)


def check_rendition(name, array, record, frames):
    """test_gpu_delivery.py's ``check_rendition`` bounds, read back at the delivery's own rate."""
    subtype, spec = PLAN[name]
    rate = spec.sample_rate
    assert record.sample_rate == rate and record.frames == int(frames * (rate / RATE)), name
    assert record.delivery == spec and record.measured.sample_rate == rate
    assert array.shape[0] == record.frames, name                       # (packed 24-bit: (frames, 6) bytes)
    measured = read_back(array, subtype, rate)
    print(name, record, "| read back:", measured.integrated, "LUFS, true peak", measured.true_peak)
    assert measured.true_peak <= 10.0 ** (spec.true_peak / 20.0) * (1.0 + 1e-9), name
    assert abs(measured.integrated - record.achieved_lufs) <= 0.01, name
    assert (" at %d Hz" % rate in str(record)) == (rate != RATE)


def test_main_delivers_at_other_rates_and_changes_nothing_else(dev, pair, monkeypatch):
    from matchering_amd.device import Device

    target, reference = pair
    n = target.shape[0]
    config = mg.Config()
    calls, kept = [], {}
    plain = Device.convert_rate

    def spy(self, buf, frames, rate_in, rate_out):
        made = plain(self, buf, frames, rate_in, rate_out)
        calls.append((frames, rate_in, rate_out))
        kept[rate_out] = np.array(self.download(made.buf, (made.frames, 2)))
        return made

    monkeypatch.setattr(Device, "convert_rate", spy)
    request = DeliveryRequest([(name, 0, subtype, spec) for name, (subtype, spec) in PLAN.items()])
    with_them = stages.main(target, reference, config, True, True, False, device=dev, deliveries=request)
    monkeypatch.setattr(Device, "convert_rate", plain)
    without = stages.main(target, reference, config, True, True, False, device=dev)
    for a, b in zip(with_them[:2], without[:2]):
        assert a.dtype == np.float32 and a.tobytes() == b.tobytes()
    # one conversion per (rendering, rate), none for the internal rate
    assert calls == [(n, RATE, 48000), (n, RATE, 96000)]
    assert request.arrays["streaming48.wav"].shape == (int(n * (48000 / 44100)), 6)
    assert request.arrays["cd48.wav"].shape == (int(n * (48000 / 44100)), 2) and request.arrays["cd48.wav"].dtype == np.int16
    assert request.arrays["hires96.wav"].shape == (int(n * (96000 / 44100)), 2) and request.arrays["hires96.wav"].dtype == np.float32
    assert request.arrays["home.wav"].shape == (n, 2)
    for name in PLAN:
        check_rendition(name, request.arrays[name], request.delivered[name], n)
    # ... and one measurement, taken at 48 kHz on the converted frames
    assert request.delivered["streaming48.wav"].measured is request.delivered["cd48.wav"].measured
    at_48 = loudness_oracle.measure(kept[48000].astype(np.float64), 48000)
    assert abs(request.delivered["cd48.wav"].measured.integrated - at_48.integrated) < 1e-6
    assert request.delivered["streaming48.wav"].limited_by == "loudness"
    # the converted frames are mgx_resample's of the rendering, and the file's values the oracle's of those frames
    with dev.lock:
        buf = dev.upload(without[0])
        old = dev.resample_frames(buf, n, 2, RATE, 48000)
        assert np.array_equal(dev.download(old.buf, (old.frames, 2)), kept[48000])
        buf.release()
        old.release()
    record = request.delivered["cd48.wav"]
    assert np.array_equal(request.arrays["cd48.wav"], delivery_oracle.deliver(kept[48000], record.gain, 16, "tpdf_hp", CD_48.seed))
    # the delivery at the internal rate is the one a request without the field produces, and shares the rendering's measurement
    bare = DeliveryRequest([("home.wav", 0, "PCM_16", Delivery(true_peak=-1.0, dither="tpdf", seed=7))])
    stages.main(target, reference, config, True, True, False, device=dev, deliveries=bare)
    assert request.arrays["home.wav"].tobytes() == bare.arrays["home.wav"].tobytes()
    assert request.delivered["home.wav"].gain == bare.delivered["home.wav"].gain
    assert request.delivered["home.wav"].measured.sample_rate == RATE


def test_a_binding_ceiling_is_limited_at_the_delivery_rate(dev, pair):
    """-9 LUFS under -1 dBTP from the unlimited rendering (about -6 LUFS with a true peak of 1.76: 3 dB down still peaks
    at 1.25): the delivery's limiter runs on the frames converted to 48 kHz, with its look-ahead in 48 kHz frames."""
    target, reference = pair
    spec = Delivery(loudness=-9.0, true_peak=-1.0, dither="tpdf_hp", seed=11, limiter=TruePeakLimiter(), sample_rate=48000)
    request = DeliveryRequest([("club.wav", 1, "PCM_16", spec)])
    stages.main(target, reference, mg.Config(), True, True, False, device=dev, deliveries=request)
    record = request.delivered["club.wav"]
    assert record.limiter_passes > 0 and record.sample_rate == 48000
    assert record.measured.sample_rate == record.limited.sample_rate == 48000
    assert record.frames == request.arrays["club.wav"].shape[0] == int(target.shape[0] * (48000 / 44100))
    measured = read_back(request.arrays["club.wav"], "PCM_16", 48000)
    print(record, "| read back:", measured.integrated, "LUFS, true peak", measured.true_peak)
    assert measured.true_peak <= 10.0 ** (-1.0 / 20.0) * (1.0 + 1e-9)
    assert abs(measured.integrated - record.achieved_lufs) <= 0.01


def results_in(folder):
    return [mg.Result(os.path.join(folder, name), subtype, delivery=spec) for name, (subtype, spec) in PLAN.items()] \
        + [mg.pcm16(os.path.join(folder, "plain16.wav"))]


def test_process_and_a_batch_job_write_each_file_at_its_rate(dev, pair, tmp_path):
    target, reference = pair
    audio_io.save(str(tmp_path / "target.wav"), target, RATE, "FLOAT")
    audio_io.save(str(tmp_path / "reference.wav"), reference, RATE, "FLOAT")
    one, two = str(tmp_path / "process"), str(tmp_path / "batch")
    os.makedirs(one)
    os.makedirs(two)
    lines = []
    mg.log(debug_handler=lines.append)
    try:
        mg.process(str(tmp_path / "target.wav"), str(tmp_path / "reference.wav"), results_in(one))
    finally:
        mg.log()
    said = [str(line) for line in lines if "delivery '" in str(line)]
    assert len(said) == 4 and sum(" at 48000 Hz" in line for line in said) == 2 and sum(" at 96000 Hz" in line for line in said) == 1
    done = mg.process_batch([{"target": str(tmp_path / "target.wav"), "reference": str(tmp_path / "reference.wav"),
                              "results": results_in(two)}], rank=0, world_size=1, lanes=1)
    assert done == [0]
    n = target.shape[0]
    for name, (subtype, spec) in list(PLAN.items()) + [("plain16.wav", ("PCM_16", Delivery()))]:
        got, rate = audio_io.read_wav(os.path.join(one, name))
        assert rate == spec.rate(RATE), name                            # the header carries the file's own rate
        assert got.shape[0] == int(n * (float(rate) / RATE)), name
        assert open(os.path.join(one, name), "rb").read() == open(os.path.join(two, name), "rb").read(), name
