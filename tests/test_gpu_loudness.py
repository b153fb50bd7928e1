"""The loudness meter on the MI355X: ``mgx_loudness`` through the C ABI against tests/loudness_oracle.py at the bounds
tests/loudness_cases.py states (the same shapes the CPU emulation runs in tests/test_loudness_host.py), its edges, and
``process(..., loudness=handler)`` / ``measure`` on the 30 s example pair.
"""

import ctypes
import hashlib
import math
import os

import numpy as np
import pytest

import loudness_cases as cases
import loudness_oracle as oracle
import matchering_amd as mg
from matchering_amd import _native, audio_io
from matchering_amd.synth import make_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from matchering_amd.device import default_device

    return default_device()


def measured(dev, x, rate):
    """(Loudness, sub-block energies) of float32 frames through ``mgx_loudness``."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with dev.lock:
        buf = dev.upload(x)
        try:
            return dev.loudness(buf, x.shape[0], rate, sub_energy=True)
        finally:
            buf.release()


def check(dev, x, rate, label):
    value, energy = measured(dev, x, rate)
    assert value.sub_blocks == energy.shape[0] and value.sub_block_frames == oracle.sub_block_frames(rate)
    fields = (value.integrated, value.range, value.momentary_max, value.short_term_max)
    return cases.assert_measured(x, rate, energy, fields, value.true_peak, value.sample_peak, label), value


@pytest.mark.parametrize("rate", cases.RATES)
def test_every_rate_and_length(dev, rate):
    for n in cases.lengths(rate):
        check(dev, cases.noise(n, rate % 1000 + n % 97, dc=0.05), rate, f"{rate} Hz, {n} frames")


@pytest.mark.parametrize("rate,subs", [(44100, 1), (44100, 2), (44100, 3), (44100, 50), (8000, 401), (8000, 801),
                                        (8000, 4801), (8000, 4813)])
def test_workgroup_counts(dev, rate, subs):
    """One workgroup, two, two and one sub-block more, about fifty; then two, three and twelve sub-blocks per workgroup."""
    n = subs * oracle.sub_block_frames(rate) + 7
    _, _, _, own, workgroups = cases.geometry(rate, n)
    check(dev, cases.noise(n, subs, dc=-0.1), rate, f"{rate} Hz, {subs} sub-blocks in {workgroups} workgroups of {own}")


def test_second_workgroup_with_a_clipped_warmup(dev):
    assert cases.workgroup_start(192000, 2 * 19200 + 1, 1) == 0 and cases.geometry(192000, 2 * 19200 + 1)[3:] == (1, 2)
    check(dev, cases.noise(2 * 19200 + 1, 5, dc=0.2), 192000, "clipped warm-up")


@pytest.mark.parametrize("rate", [44100, 192000])
def test_noise_dc_and_a_60_db_step(dev, rate):
    size = oracle.sub_block_frames(rate)
    n = 40 * size + 11
    check(dev, cases.noise_dc_step(rate, n, 17 * size), rate, f"{rate} Hz, step on an ownership boundary")
    on_tile = cases.workgroup_start(rate, n, 20) + 2 * cases.TILE
    check(dev, cases.noise_dc_step(rate, n, on_tile), rate, f"{rate} Hz, step on a tile boundary")


@pytest.mark.parametrize("rate", [44100, 48000, 76050, 192000])
def test_step_ahead_of_a_warmup_with_nothing_to_spare(dev, rate):
    """A length at which the last workgroup's tiles begin exactly H frames ahead of its sub-blocks (at 76050 Hz every
    workgroup's do), the 60 dB step 0.1 to 0.4 sub-blocks ahead of them: H alone holds the bound."""
    n, begin = cases.zero_slack_length(rate, 40)
    size = oracle.sub_block_frames(rate)
    for back in (size * k // 20 for k in (2, 3, 4, 5, 6, 8)):
        check(dev, cases.noise_dc_step(rate, n, begin - back), rate, f"{rate} Hz, {n} frames, step {back} frames ahead of {begin}")


def test_impulses(dev):
    rate, size = 44100, 4410
    n = 6 * size + 100
    for at in ([0], [n - 1], [3 * size - 1], [3 * size], [0, n - 1, 3 * size - 1, 3 * size]):
        want, _ = check(dev, cases.impulses(n, at), rate, f"impulses at {at}")
        assert want.true_peak == 1.0 == want.sample_peak
    x = np.zeros((n, 2), dtype=np.float32)
    x[3 * size - 1, 0] = x[3 * size, 0] = 0.5
    want, value = check(dev, x, rate, "a pair across the boundary")
    assert value.true_peak > 0.6 and value.sample_peak == 0.5


def test_silence(dev):
    for n in (1, 4409, 5 * 4410, 40 * 4410 + 3):
        value, energy = measured(dev, np.zeros((n, 2), dtype=np.float32), 44100)
        assert not energy.any() and value.true_peak == 0.0 == value.sample_peak
        assert value.integrated == value.momentary_max == value.short_term_max == -math.inf and value.range == 0.0
        assert value.true_peak_db == -math.inf


def test_no_frames_at_all(dev):
    report, count = _native.MgxLoudnessReport(), ctypes.c_int64(-1)
    rc = _native.library().mgx_loudness(dev.handle, None, 0, 44100, ctypes.byref(report), None, 0, ctypes.byref(count))
    assert rc == 0 and count.value == 0 and report.integrated == -math.inf and report.true_peak == 0.0


def test_non_finite_input_fails_and_the_handle_works_on(dev):
    x = cases.noise(7 * 4410 + 300, 1)
    good, _ = measured(dev, x, 44100)
    for at, value in ((0, np.nan), (7 * 4410 + 299, np.inf), (3 * 4410 + 17, -np.inf)):
        bad = x.copy()
        bad[at, 1] = value
        with pytest.raises(_native.MgxError) as refused:
            measured(dev, bad, 44100)
        assert refused.value.code == _native.ERR_ARGUMENT and "the frames to measure" in str(refused.value)
        again, _ = measured(dev, x, 44100)
        assert again == good


def test_edge_arguments(dev):
    lib = _native.library()
    x = cases.noise(5 * 4410 + 9, 2)
    with dev.lock:
        buf = dev.upload(x)
        try:
            plain = dev.loudness(buf, x.shape[0], 44100)                             # sub_energy = NULL
            with_energy, energy = dev.loudness(buf, x.shape[0], 44100, sub_energy=True)
            assert plain == with_energy and energy.shape == (5, 2)
            report, count = _native.MgxLoudnessReport(), ctypes.c_int64()
            small = (ctypes.c_double * 8)()
            rc = lib.mgx_loudness(dev.handle, ctypes.c_void_p(buf.ptr), x.shape[0], 44100, ctypes.byref(report), small, 4,
                                  ctypes.byref(count))
            assert rc == _native.ERR_ARGUMENT and count.value == 5
            assert lib.mgx_loudness(dev.handle, ctypes.c_void_p(buf.ptr), x.shape[0], 7999, ctypes.byref(report), None, 0,
                                    None) == _native.ERR_ARGUMENT
            assert lib.mgx_loudness(dev.handle, None, x.shape[0], 44100, ctypes.byref(report), None, 0, None) == _native.ERR_ARGUMENT
            assert lib.mgx_loudness(dev.handle, ctypes.c_void_p(buf.ptr), x.shape[0], 44100, None, None, 0, None) == _native.ERR_ARGUMENT
            assert lib.mgx_loudness(dev.handle, ctypes.c_void_p(buf.ptr), x.shape[0], 44100, ctypes.byref(report), None, 0,
                                    None) == 0                                       # count = NULL too
            assert report.integrated == plain.integrated
        finally:
            buf.release()


def test_two_calls_agree_bit_for_bit(dev):
    x = cases.noise_dc_step(44100, 60 * 4410 + 3, 31 * 4410)
    first, second = measured(dev, x, 44100), measured(dev, x, 44100)
    assert first[0] == second[0] and np.array_equal(first[1], second[1])


def test_the_80_second_known_answer_at_48_khz(dev):
    """EBU Tech 3341 case 3: 10 s at -36 dBFS, 60 s at -23, 10 s at -36 -> -23.0 +- 0.1 LUFS, end to end."""
    x = cases.segments(48000, [(10, -36), (60, -23), (10, -36)])
    value, _ = measured(dev, x, 48000)
    print(value)
    assert -23.1 <= value.integrated <= -22.9
    assert abs(value.sample_peak_db + 23.0) < 0.01 and value.true_peak_db >= value.sample_peak_db


def test_true_peak_catches_what_the_sample_peak_misses(dev):
    x = cases.faded_sine(48000, 12000.0, 45.0, 0.5)
    value, _ = measured(dev, x, 48000)
    assert -6.4 <= value.true_peak_db <= -5.8 and abs(value.sample_peak_db + 9.03) < 0.01


def test_process_reports_loudness_and_changes_nothing_else(dev, tmp_path):
    """``process(..., loudness=handler)`` on the 30 s example pair: the handler sees the target, the reference and each
    rendering; every value is ``measure()`` of the written float file; and the log lines and the files of that run are
    compared, byte for byte, with those of a run of THIS commit's ``process`` without the argument.  (A test cannot run
    the parent commit: that the run without the argument equals the parent's was checked once by hand, both packages
    side by side on one GPU, same log lines and same seven files.)  ``measure`` leaves no upload pinned behind it."""
    target, reference = make_pair(30.0)
    audio_io.save(str(tmp_path / "target.wav"), target, 44100, "FLOAT")
    audio_io.save(str(tmp_path / "reference.wav"), reference, 44100, "FLOAT")
    names = {"result": "limited.wav", "result_no_limiter": "plain.wav", "result_no_limiter_normalized": "normalized.wav"}

    def run(folder, **extra):
        os.makedirs(folder)
        lines = []
        mg.log(lines.append, show_codes=True)
        try:
            mg.process(str(tmp_path / "target.wav"), str(tmp_path / "reference.wav"),
                       [mg.Result(os.path.join(folder, names["result"]), "FLOAT"),
                        mg.Result(os.path.join(folder, names["result_no_limiter"]), "FLOAT", use_limiter=False, normalize=False),
                        mg.Result(os.path.join(folder, names["result_no_limiter_normalized"]), "FLOAT", use_limiter=False),
                        mg.pcm16(os.path.join(folder, "limited16.wav"))], **extra)
        finally:
            mg.log()
        digests = {f: hashlib.sha256(open(os.path.join(folder, f), "rb").read()).hexdigest() for f in sorted(os.listdir(folder))}
        return [line.replace(folder, "<folder>") for line in lines], digests

    seen = []
    with_lines, with_files = run(str(tmp_path / "with"), loudness=lambda name, value: seen.append((name, value)))
    without_lines, without_files = run(str(tmp_path / "without"))
    assert with_lines == without_lines and with_files == without_files and len(with_files) == 4
    assert [name for name, _ in seen] == ["target", "reference", *names]
    files = {"target": str(tmp_path / "target.wav"), "reference": str(tmp_path / "reference.wav"),
             **{name: str(tmp_path / "with" / f) for name, f in names.items()}}
    for name, value in seen:
        again = mg.measure(files[name])
        print(name, value)
        assert value.frames == again.frames == 30 * 44100 and math.isfinite(value.integrated)
        for field in ("integrated", "range", "momentary_max", "short_term_max"):
            assert abs(getattr(value, field) - getattr(again, field)) <= 1e-8, (name, field)
        assert abs(value.true_peak - again.true_peak) <= 1e-12 * again.true_peak and value.sample_peak == again.sample_peak
    assert not dev._keep_until_sync                  # (measure() waited: no track-sized pinned block per call stays)
    # ... and the array form, at the array's own rate, against the oracle
    value = mg.measure(target, 44100)
    want = oracle.measure(target, 44100)
    assert abs(value.integrated - want.integrated) <= 1e-8 and abs(value.true_peak - want.true_peak) <= 1e-12 * want.true_peak
    loud = dict(seen)
    assert loud["result"].integrated > loud["target"].integrated + 3.0            # the master is louder than the quiet target
    assert loud["result"].sample_peak <= 1.0
