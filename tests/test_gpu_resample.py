"""The sample-rate converter on the MI355X (``mgx_resample``): ``Device.resample_frames`` against the host resampler
it restates, the plan cache, and ``process`` / ``process_batch`` with off-rate and mono files taking the resident
route.  The host form ``matchering_amd.resample.resample`` in float64 is the reference throughout.
"""

import ctypes
import os

import numpy as np
import pytest

import matchering_amd as mg
from conftest import rms_error
from matchering_amd import audio_io, batch, checker, core, stages
from matchering_amd import device as device_module
from matchering_amd import resample as host
from matchering_amd.log import Code, ModuleError
from matchering_amd.synth import synth

pytestmark = pytest.mark.gpu

PAIRS = [(48000, 44100), (44100, 48000), (96000, 44100), (192000, 44100), (8000, 44100), (32000, 44100),
         (22050, 44100), (88200, 44100)]


def as_encoding(values, encoding):
    """Noise in [-1, 1) as a file of that encoding holds it (audio_io.PCM_DTYPES): (array, its float64 values)."""
    if encoding == "float32":
        array = values.astype(np.float32)
    elif encoding == "int16":
        array = np.clip(np.rint(values * 32768.0), -32768, 32767).astype(np.int16)
    else:                                                                      # packed little-endian 24-bit
        whole = np.clip(np.rint(values * 8388608.0), -8388608, 8388607).astype("<i4")
        n, channels = whole.shape
        array = np.ascontiguousarray(whole.view(np.uint8).reshape(n, channels, 4)[:, :, :3]).reshape(n, channels * 3)
    return array, np.asarray(audio_io.pcm_to_float(array, np.float64), dtype=np.float64)


def float64_bound(sr, new, peak):
    """max|x| (sum|w| W 2^-53 + W 2e-15): W float64 accumulations of terms bounded by the largest row sum, plus the
    plan's tolerance carried through the sum -- from the host plan of the same rates."""
    plan = host._Plan(sr, new)
    g = int(np.gcd(sr, new))
    proto, _ = host._prototype(plan, new // g, sr // g)
    width = 2 * plan.taps
    # a phase's row is every L-th tap of the prototype
    row_sum = max(float(np.abs(proto[p::new // g]).sum()) for p in range(new // g))
    return peak * (row_sum * width * 2.0 ** -53 + width * 2e-15)


def compare(got, want64, bound, what):
    """Each sample within one float32 spacing of float32(host) plus the float64 bound; at most 1 in 10 000 different
    from float32(host) at all (only sums on a rounding boundary may flip; a systematic offset may not hide in the band)."""
    want = want64.astype(np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.size == 0:
        return
    error = np.abs(got.astype(np.float64) - want.astype(np.float64))
    allowed = np.spacing(np.abs(want)).astype(np.float64) + bound
    different = int(np.count_nonzero(got != want))
    print(f"{what}: max error {error.max():.3e}, {different} of {want.size} differ from float32(host)")
    assert np.all(error <= allowed), (what, float((error - allowed).max()))
    assert different * 10000 <= want.size, (what, different, want.size)


def convert(dev, array, sr, new):
    channels = audio_io.pcm_channels(array)
    with dev.lock:
        decoded = dev.upload_frames(array)
        frames = dev.resample_frames(decoded, array.shape[0], channels, sr, new)
        out = np.array(dev.download(frames.buf, (frames.frames, 2)))
        decoded.release()
        frames.release()
    return out


@pytest.fixture(scope="module")
def dev():
    from matchering_amd.device import default_device

    return default_device()


@pytest.mark.parametrize("encoding", ["float32", "int16", "pcm24"])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("sr,new", PAIRS)
def test_device_resampler_is_the_host_resampler(dev, sr, new, channels, encoding):
    lengths = [5, 3000]
    if encoding == "float32" or (sr, new) == (48000, 44100):
        lengths.append(20 * sr + 77)
    for n in lengths:
        rng = np.random.RandomState((sr + new + n + channels) % 100003)
        array, values = as_encoding(np.clip(0.3 * rng.randn(n, channels), -1, 1), encoding)
        got = convert(dev, array, sr, new)
        want = host.resample(np.repeat(values, 2, axis=1) if channels == 1 else values, sr, new)
        assert got.shape[0] == int(n * (float(new) / sr))
        compare(got, want, float64_bound(sr, new, float(np.abs(values).max())), f"{sr}->{new} {encoding} x{channels} n={n}")
        if channels == 1:
            assert np.array_equal(got[:, 0], got[:, 1])


def test_exact_phases_far_into_a_file(dev):
    """Twenty-one minutes of 48 kHz int16 stereo: the last outputs' phases come from t M / L in 64-bit integers.  The
    reference is the host resampler on the file's tail, cut at a multiple of M = 160 frames so that its phases are the
    file's; compared on a window at the very end, away from the cut."""
    sr, new, minutes = 48000, 44100, 21
    n = sr * 60 * minutes + 1234
    rng = np.random.default_rng(77)
    array = rng.integers(-9000, 9000, size=(n, 2), dtype=np.int16)
    got = convert(dev, array, sr, new)
    assert got.shape[0] == int(n * (float(new) / sr))
    cut = (n - 8 * sr) // 160 * 160
    tail = host.resample(audio_io.pcm_to_float(array[cut:], np.float64), sr, new)
    first = cut // 160 * 147                                          # the output that sits exactly on frame `cut`
    assert first + tail.shape[0] == got.shape[0]
    window = 4 * new
    compare(got[-window:], tail[-window:], float64_bound(sr, new, 9000 / 32768.0), "21 minutes in")


@pytest.mark.parametrize("sr,new", [(48000, 44100), (44100, 48000), (96000, 44100), (32000, 44100)])
def test_a_sine_stays_the_same_sine_on_the_device(dev, sr, new):
    n = sr // 4
    t_old = np.arange(n) / sr
    x = np.stack([np.sin(2 * np.pi * 1000 * t_old), 0.5 * np.cos(2 * np.pi * 9000 * t_old)], axis=1).astype(np.float32)
    y = convert(dev, x, sr, new)
    t_new = np.arange(y.shape[0]) / new
    want = np.stack([np.sin(2 * np.pi * 1000 * t_new), 0.5 * np.cos(2 * np.pi * 9000 * t_new)], axis=1)
    edge = 200
    assert np.abs(y[edge:-edge] - want[edge:-edge]).max() <= 5e-4


def test_a_second_conversion_designs_and_uploads_nothing():
    from matchering_amd._native import MgxError
    from matchering_amd.device import Device

    own = Device(0)
    try:
        x = (0.3 * np.random.RandomState(1).randn(3000, 2)).astype(np.float32)
        with pytest.raises(MgxError):
            own.resample_plan(48000, 44100)                           # nothing converted on this handle yet
        first = convert(own, x, 48000, 44100)
        address, phases, width, designed = own.resample_plan(48000, 44100)
        assert address and (phases, width, designed) == (147, 140, 1)
        second = convert(own, x, 48000, 44100)
        assert own.resample_plan(48000, 44100) == (address, 147, 140, 1)
        assert np.array_equal(first, second)
        convert(own, x, 44100, 48000)
        assert own.resample_plan(44100, 48000)[1:] == (160, 130, 2)
        assert own.resample_plan(48000, 44100) == (address, 147, 140, 2)
    finally:
        own.close()


def test_mgx_resample_refuses_on_a_live_handle(dev):
    from matchering_amd._native import ERR_UNSUPPORTED, MgxError

    with dev.lock:
        buf = dev.upload(np.zeros((1000, 2), dtype=np.float32))
        with pytest.raises(MgxError) as refused:
            dev.resample_frames(buf, 1000, 2, 44100, 44101)
        assert refused.value.code == ERR_UNSUPPORTED
        n_out = ctypes.c_int64()
        small = dev.alloc(8 * 100)
        rc = device_module.library().mgx_resample(dev.handle, ctypes.c_void_p(buf.ptr), 1000, 2, 48000, 44100,
                                                  ctypes.c_void_p(small.ptr), 100, ctypes.byref(n_out))
        assert rc == -1 and n_out.value == 918                        # MGX_ERR_ARGUMENT: capacity too small
        empty = dev.resample_frames(buf, 1, 2, 48000, 44100)          # n_out == 0: a success that launches nothing
        assert empty.frames == 0
        for b in (buf, small, empty):
            b.release()
    assert device_module.converted_length(1000, 2, 44100, 44101) is None


# ---- end to end ------------------------------------------------------------------------------------------------------
def _files(tmp_path, target_subtype):
    target = 0.5 * synth(9.0, 48000, 31)
    reference = np.clip(2.5 * synth(8.0, 22050, 32, corner=3500.0), -1.0, 1.0)[:, :1]
    t_path, r_path = str(tmp_path / f"target_{target_subtype}.wav"), str(tmp_path / "reference_mono.wav")
    audio_io.write_wav(t_path, target, 48000, target_subtype)
    audio_io.write_wav(r_path, reference, 22050, "PCM_16")
    return t_path, r_path


def _process_codes(target, reference, results, config):
    seen = []
    mg.log(warning_handler=seen.append, info_handler=seen.append, show_codes=True)
    try:
        mg.process(target, reference, results, config)
    finally:
        mg.log()
    return seen


@pytest.mark.parametrize("subtype", ["PCM_16", "PCM_24"])
def test_process_takes_off_rate_and_mono_files_resident(tmp_path, monkeypatch, subtype):
    config = mg.Config()
    t_path, r_path = _files(tmp_path, subtype)
    out = str(tmp_path / "device.wav")
    taken = []
    real = device_module.Device.track_frames

    def spy(self, audio, rate, internal):
        taken.append((rate, audio_io.pcm_channels(audio)))
        return real(self, audio, rate, internal)

    monkeypatch.setattr(device_module.Device, "track_frames", spy)
    codes = _process_codes(t_path, r_path, [mg.Result(out, subtype="FLOAT")], config)
    assert taken == [(48000, 2), (22050, 1)]                          # both converted on the device

    # the host path for the same files: the loader's rule of the tracks that need no conversion
    def on_rate_stereo_only(audio, rate, internal):
        return (audio.dtype.kind in "iu" or audio.dtype == np.float32) and audio_io.pcm_channels(audio) == 2 \
            and rate == internal and audio.shape[0] > 0

    monkeypatch.setattr(device_module, "takes_resident", on_rate_stereo_only)
    host_out = str(tmp_path / "host.wav")
    host_codes = _process_codes(t_path, r_path, [mg.Result(host_out, subtype="FLOAT")], config)
    assert len(taken) == 2                                            # (nothing went resident this time)
    assert codes == host_codes
    assert any(str(int(Code.WARNING_TARGET_IS_RESAMPLED)) in c for c in codes)
    assert any(str(int(Code.INFO_REFERENCE_IS_MONO)) in c for c in codes)
    assert any(str(int(Code.INFO_REFERENCE_IS_RESAMPLED)) in c for c in codes)

    # stages.main on the host-resampled arrays
    tracks = []
    for path, role in ((t_path, "target"), (r_path, "reference")):
        audio, rate = audio_io.load(path, role, str(tmp_path), pcm=True)
        tracks.append(checker.check(audio, rate, config, role)[0])
    want = stages.main(tracks[0], tracks[1], config)[0]
    got, rate = audio_io.load(out, "result", str(tmp_path))
    assert rate == config.internal_sample_rate and got.shape == want.shape
    error = rms_error(got, want)
    print(f"process, {subtype} target: rms error against stages.main on host-resampled arrays {error:.3e}")
    assert error <= 1e-5
    assert rms_error(audio_io.load(host_out, "result", str(tmp_path))[0], want) <= 1e-5


@pytest.mark.parametrize("subtype", ["PCM_16", "PCM_24"])
def test_batch_writes_the_files_process_writes(tmp_path, subtype):
    config = mg.Config()
    t_path, r_path = _files(tmp_path, subtype)
    single, many = str(tmp_path / "single.wav"), str(tmp_path / "batch.wav")
    mg.process(t_path, r_path, [mg.pcm24(single)], config)
    done = batch.process_batch([{"target": t_path, "reference": r_path, "results": [mg.pcm24(many)]}], config,
                               lanes=1, io_threads=1)
    assert done == [0]
    with open(single, "rb") as a, open(many, "rb") as b:
        assert a.read() == b.read()


def test_a_file_as_its_own_reference_at_an_off_rate(tmp_path):
    t_path, _ = _files(tmp_path, "PCM_16")
    with pytest.raises(ModuleError) as same:
        mg.process(t_path, t_path, [mg.pcm16(str(tmp_path / "never.wav"))], mg.Config())
    assert same.value.code == Code.ERROR_TARGET_EQUALS_REFERENCE
    with pytest.raises(ModuleError) as same:
        batch.process_batch([{"target": t_path, "reference": t_path, "results": [mg.pcm16(str(tmp_path / "never.wav"))]}],
                            mg.Config(), lanes=1, io_threads=1)
    assert same.value.code == Code.ERROR_TARGET_EQUALS_REFERENCE
    assert not os.path.exists(str(tmp_path / "never.wav"))


# ---- process and process_batch on one intake: the same files from every kind of file -----------------------------------
# (byte identity and equal codes held for every case at the commit before intake.py, where the two had loaders of their own)
KINDS = {   # case -> (target, reference), each (subtype, rate, channels, clipped)
    "A": (("PCM_24", 44100, 1, True), ("FLOAT", 44100, 2, False)),     # on-rate mono column fill; float32 as it is
    "B": (("PCM_32", 48000, 2, False), ("PCM_16", 22050, 1, False)),   # the host's float64 resampler beside the device's
    "C": (("FLOAT", 48000, 2, False), ("PCM_24", 44100, 2, False)),    # a converted target, a resident unchanged reference
}


def _kind_file(tmp_path, name, kind, seed):
    subtype, rate, channels, clipped = kind
    audio = synth(0.5, rate, seed)
    audio = np.clip(8.0 * audio, -1.0, 1.0) if clipped else 0.5 * audio
    path = str(tmp_path / f"{name}.wav")
    audio_io.write_wav(path, audio[:, :channels], rate, subtype)
    return path


def _codes_of(call):
    seen = []
    mg.log(warning_handler=seen.append, info_handler=seen.append, show_codes=True)
    try:
        call()
    finally:
        mg.log()
    # (loading, exporting and completed are lines of ``process`` alone)
    return sorted(code for code in (str(line).split(":")[0] for line in seen) if code not in ("2003", "2008", "2010"))


def _same_files_and_codes(tmp_path, config, target, reference, job_reference):
    single, many = str(tmp_path / "single.wav"), str(tmp_path / "batch.wav")
    codes = _codes_of(lambda: mg.process(target, reference, [mg.pcm24(single)], config))
    job = {"target": target, "results": [mg.pcm24(many)], **job_reference}
    batch_codes = _codes_of(lambda: batch.process_batch([job], config, lanes=1, io_threads=1))
    print(f"process: {codes}\nprocess_batch: {batch_codes}")
    with open(single, "rb") as a, open(many, "rb") as b:
        assert a.read() == b.read()
    assert codes == batch_codes and codes


@pytest.mark.parametrize("case", sorted(KINDS))
def test_batch_writes_the_files_process_writes_from_every_kind(tmp_path, case):
    target = _kind_file(tmp_path, "target", KINDS[case][0], 41)
    reference = _kind_file(tmp_path, "reference", KINDS[case][1], 42)
    _same_files_and_codes(tmp_path, mg.Config(), target, reference, {"reference": reference})


def test_batch_writes_the_files_process_writes_against_a_profile(tmp_path):
    from matchering_amd.profile import ReferenceProfile

    config = mg.Config()
    target = _kind_file(tmp_path, "target", KINDS["B"][0], 41)
    reference = _kind_file(tmp_path, "reference", KINDS["B"][1], 42)
    saved = str(tmp_path / "reference.profile")
    ReferenceProfile.analyze(reference, config).save(saved)
    _same_files_and_codes(tmp_path, config, target, saved, {"reference_profile": saved})


def test_measure_hears_a_file_as_process_does(tmp_path, dev):
    """``loudness.measure(path)``: a file the device takes goes through ``Device.track_frames``, any other through the
    host conversion ``checker.check`` makes."""
    config = mg.Config()
    internal = config.internal_sample_rate
    target = _kind_file(tmp_path, "target", KINDS["B"][0], 41)
    reference = _kind_file(tmp_path, "reference", KINDS["B"][1], 42)
    audio, rate = audio_io.load(reference, "reference", str(tmp_path), pcm=True)
    with dev.lock:
        frames = dev.track_frames(audio, rate, internal)
    try:
        assert mg.measure(reference, config=config) == mg.measure(frames, internal, config)
    finally:
        frames.release()
    audio, rate = audio_io.load(target, "target", str(tmp_path), pcm=True)
    assert mg.measure(target, config=config) == mg.measure(checker.check(audio, rate, config, "target")[0], internal, config)
