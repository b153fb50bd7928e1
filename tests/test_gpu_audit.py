"""The audit on the MI355X: ``mgx_audit`` through the C ABI against tests/audit_oracle.py -- every integer field and the
peaks equal, every sum within the first-order bound of float64 summation -- at the lengths where a segment or a sub-block
begins, on rail runs, silences and non-finite samples placed around the segment borders, on integer PCM of every width,
at its argument edges, and through ``mg.audit``, ``process(..., audit=handler)``, a batch job and the example.

Shapes: a segment is S = 4096 frames and a sub-block B = rate / 10, so a few segments (16 K frames) reach every path; no
index can leave 32 bits below the 500 million frames ``mgx_audit`` accepts, the global offsets are 64-bit.
Bounds: a sum of n exact terms, added in any order in float64, lies within n 2^-52 sum|terms| of the exact sum (first
order); the terms are exact for float32 and 16 / 24-bit input (a product of two 24-bit significands fits 53 bits) and are
the oracle's own rounded products for 32-bit input (the kernel multiplies and adds separately, as numpy does).  The
derived ratios are compared at 1e-12 relative on signals that condition them well (correlated channels, a DC offset).
"""

import ctypes
import math
import os
import runpy

import numpy as np
import pytest

import audit_oracle as oracle
import matchering_amd as mg
from matchering_amd import _native, audio_io
from matchering_amd.delivery import Delivery
from matchering_amd.qc import AuditLimits
from matchering_amd.synth import make_pair

pytestmark = pytest.mark.gpu

S = 4096
INTS = ("frames", "bits", "nonfinite", "clip_events", "clip_samples", "clip_longest", "clip_first", "head_silence",
        "tail_silence", "gap_longest", "gap_at", "sub_blocks", "sub_block_frames", "correlation_min_at")
RATIOS = ("balance_db", "correlation", "mono_loss_db", "correlation_min")


@pytest.fixture(scope="module")
def dev():
    from matchering_amd.device import default_device

    return default_device()


def audited(dev, x, bits, rate, limits=None):
    """(Audit, sub-block sums) of float32 frames or file PCM through ``mgx_audit``."""
    x = np.ascontiguousarray(x, dtype=np.float32) if bits == 0 else np.ascontiguousarray(x)
    with dev.lock:
        buf = dev.upload(x, dtype=None)
        try:
            return dev.audit(buf, x.shape[0], rate, bits, limits, sub_sums=True)
        finally:
            buf.release()


def close(a, b, rel=1e-12):
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= rel * abs(b)


def assert_audit(got, sums, want, label):
    """Every integer field and the peaks equal; sums within n 2^-52 sum|terms|; ratios at 1e-12 or both NaN."""
    for name in INTS:
        assert getattr(got, name) == want[name], (label, name, getattr(got, name), want[name])
    assert got.peak == want["peak"], (label, got.peak, want["peak"])
    eps = 2.0 ** -52
    figures = {"sum0": got.sum[0], "sum1": got.sum[1], "sumsq0": got.sumsq[0], "sumsq1": got.sumsq[1], "sum_lr": got.sum_lr}
    exact = {"sum0": want["sum"][0], "sum1": want["sum"][1], "sumsq0": want["sumsq"][0], "sumsq1": want["sumsq"][1],
             "sum_lr": want["sum_lr"]}
    for name, value in figures.items():
        terms, magnitude = want["terms"][name]
        print(label, name, value, exact[name], "bound", terms * eps * magnitude)
        assert abs(value - exact[name]) <= terms * eps * magnitude, (label, name, value, exact[name])
    if sums is not None:
        assert sums.shape == want["sub_sums"].shape, (label, sums.shape)
        B, n = want["sub_block_frames"], want["frames"]
        for k in range(sums.shape[0]):
            terms = min(n, (k + 1) * B) - k * B
            for c in range(3):
                assert abs(sums[k, c] - want["sub_sums"][k, c]) <= terms * eps * want["sub_terms"][k, c], (label, k, c)
    for name in RATIOS:
        assert close(getattr(got, name), want[name]), (label, name, getattr(got, name), want[name])
    for c in range(2):
        assert close(got.dc[c], want["dc"][c]) and close(got.rms[c], want["rms"][c]), (label, "dc / rms", c)


def check(dev, x, bits, rate, label, limits=None):
    limits = AuditLimits() if limits is None else limits
    got, sums = audited(dev, x, bits, rate, limits)
    want = oracle.audit(x, bits, rate, limits.clip_level, limits.clip_run, limits.silence_level)
    assert_audit(got, sums, want, label)
    return got


def noise(n, seed, level=0.1, dc=0.01):
    """Noise at -20 dBFS, the right channel half the left and half its own (so that no ratio is a difference of nearly
    equal numbers), a small DC offset; float32, under the rail."""
    rng = np.random.default_rng(seed)
    left = level * rng.standard_normal(n)
    right = 0.5 * left + 0.5 * level * rng.standard_normal(n)
    return np.clip(np.stack([left, right], axis=1) + dc, -0.99, 0.99).astype(np.float32)


def loud(n, seed):
    """Frames that are never silent and never at the rail: magnitudes in [0.05, 0.15], random signs."""
    rng = np.random.default_rng(seed)
    return ((0.05 + 0.1 * rng.random((n, 2))) * rng.choice([-1.0, 1.0], size=(n, 2))).astype(np.float32)


# ---- lengths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [44100, 48000])
def test_lengths_around_segments_and_sub_blocks(dev, rate):
    B = rate // 10
    for n in (1, 2, S - 1, S, S + 1, 3 * S + 17, B, B + 1, 2 * B - 1):
        x = noise(n, rate % 1000 + n)
        first = check(dev, x, 0, rate, f"{rate} Hz, {n} frames")
        assert first.sub_blocks == -(-n // B) and first.frames == n
        again, sums = audited(dev, x, 0, rate)
        assert repr(again) == repr(first)                           # bit for bit: a float's repr is the float
        assert sums.tobytes() == audited(dev, x, 0, rate)[1].tobytes()


def test_a_track_of_many_sub_blocks_has_its_least_correlation_found(dev):
    """41 sub-blocks at 8000 Hz (the most sub-blocks a segment meets: 7), all but the first quarter in anti-phase: the
    last of the twelve windows is the first that lies wholly there."""
    n = 40 * 800 + 123
    x = noise(n, 5)
    x[n // 4:, 1] = -x[n // 4:, 0]
    got = check(dev, x, 0, 8000, "8000 Hz, anti-phase from the first quarter on")
    assert got.correlation_min == -1.0 and got.correlation_min_at == -(-(n // 4) // 800) == 11
    assert [f[0] for f in got.findings()] == ["dc_offset", "out_of_phase"]


# ---- rail runs ----------------------------------------------------------------------------------------------------------
N_RUNS = 4 * S + 100
# name -> [(channel, first frame, length, alternate the sign)], and what clip_run 3 must find: events, samples, longest, first
RAIL_CASES = {
    "inside one segment": ([(0, 1000, 5, False)], ((1, 0), (5, 0), (5, 0), (1000, -1))),
    "ending on the last sample of a segment": ([(0, S - 4, 4, False)], ((1, 0), (4, 0), (4, 0), (S - 4, -1))),
    "starting on the first sample of a segment": ([(1, 2 * S, 4, False)], ((0, 1), (0, 4), (0, 4), (-1, 2 * S))),
    "straddling a border with 1 + 2 samples": ([(0, S - 1, 3, False)], ((1, 0), (3, 0), (3, 0), (S - 1, -1))),
    "covering two whole segments": ([(1, S - 7, 2 * S + 20, False)], ((0, 1), (0, 2 * S + 20), (0, 2 * S + 20), (-1, S - 7))),
    "at frame 0": ([(0, 0, 3, False)], ((1, 0), (3, 0), (3, 0), (0, -1))),
    "ending at frame n - 1": ([(1, N_RUNS - 3, 3, False)], ((0, 1), (0, 3), (0, 3), (-1, N_RUNS - 3))),
    "the two channels with different runs": ([(0, 100, 2, False), (0, 300, 6, False), (1, 200, 4, False), (1, S + 5, 1, False)],
                                             ((1, 1), (6, 4), (6, 4), (300, 200))),
    "alternating-sign full scale": ([(0, 2 * S - 3, 7, True)], ((1, 0), (7, 0), (7, 0), (2 * S - 3, -1))),
}


@pytest.mark.parametrize("name", list(RAIL_CASES))
def test_rail_runs_placed_by_construction(dev, name):
    placed, expected = RAIL_CASES[name]
    x = loud(N_RUNS, len(name))
    for channel, first, length, alternate in placed:
        x[first:first + length, channel] = [(-1.0 if alternate and i % 2 else 1.0) for i in range(length)]
    for clip_run in (1, 3):
        got = check(dev, x, 0, 44100, f"{name}, clip_run {clip_run}", AuditLimits(clip_run=clip_run))
        if clip_run == 3:
            assert (got.clip_events, got.clip_samples, got.clip_longest, got.clip_first) == expected, name
        else:
            assert got.clip_events == tuple(sum(1 for c, *_ in placed if c == channel) for channel in range(2)), name
    assert "clipping" in [f[0] for f in got.findings()]


# ---- silence ------------------------------------------------------------------------------------------------------------
N_QUIET = 3 * S + 50


def test_silence_all_and_single_frames(dev):
    x = np.zeros((N_QUIET, 2), dtype=np.float32)
    got = check(dev, x, 0, 44100, "all silent")
    assert (got.head_silence, got.tail_silence, got.gap_longest, got.gap_at) == (N_QUIET, N_QUIET, 0, -1)
    assert math.isnan(got.correlation) and math.isnan(got.correlation_min) and got.peak == (0.0, 0.0)
    for at in (0, N_QUIET - 1, S + 17):
        x = np.zeros((N_QUIET, 2), dtype=np.float32)
        x[at] = (0.25, -0.25)
        got = check(dev, x, 0, 44100, f"one frame at {at}")
        assert (got.head_silence, got.tail_silence, got.gap_longest, got.gap_at) == (at, N_QUIET - 1 - at, 0, -1)


def test_silence_gaps(dev):
    x = loud(N_QUIET, 1)
    x[S - 10:2 * S + 10] = 0.0
    got = check(dev, x, 0, 44100, "a gap across two segment borders")
    assert (got.head_silence, got.tail_silence, got.gap_longest, got.gap_at) == (0, 0, S + 20, S - 10)
    assert ("dropout", (S + 20) / 44100, 0.05) in got.findings()
    x = loud(N_QUIET, 2)
    x[100:150] = 0.0
    x[S + 100:S + 150] = 0.0
    x[:7] = 0.0
    x[-9:] = 1e-6                                                   # under -90 dBFS: silent
    got = check(dev, x, 0, 44100, "two gaps of equal length")
    assert (got.head_silence, got.tail_silence, got.gap_longest, got.gap_at) == (7, 9, 50, 100)


def test_silence_exact_zeros_and_half_silent_frames(dev):
    exact = AuditLimits(silence_db=-math.inf)
    x = loud(N_QUIET, 3)
    x[200:260] = 1e-30                                              # not zero: not silent where only exact zeros are
    x[S - 3:S + 3] = 0.0
    x[:5] = 0.0
    got = check(dev, x, 0, 44100, "silence_db -inf against 1e-30", exact)
    assert (got.head_silence, got.gap_longest, got.gap_at) == (5, 6, S - 3)
    got = check(dev, x, 0, 44100, "the same at -90 dB")
    assert (got.head_silence, got.gap_longest, got.gap_at) == (5, 60, 200)
    x = loud(N_QUIET, 4)
    x[1000:1100, 0] = 0.0                                           # one channel silent, the other loud: not silent
    x[2 * S - 5:2 * S + 5, 1] = 0.0
    got = check(dev, x, 0, 44100, "half-silent frames")
    assert (got.head_silence, got.tail_silence, got.gap_longest, got.gap_at) == (0, 0, 0, -1)


# ---- non-finite ---------------------------------------------------------------------------------------------------------
def test_non_finite_samples(dev):
    n = 3 * S + 11
    x = loud(n, 6)
    x[500:510, 0] = 1.0
    x[505, 0] = -np.inf                                            # splits the run into 5 and 4
    x[2 * S - 2:2 * S + 2, 1] = -1.0
    x[2 * S, 1] = np.nan                                           # ... and this one, on a segment's first sample, into 2 and 1
    x[S - 1, 0] = np.nan                                           # the last sample of a segment
    x[S, 1] = np.inf                                               # the first
    x[3000:3010] = 0.0
    x[3004, 1] = np.nan                                            # makes its frame not silent
    got = check(dev, x, 0, 44100, "NaN and infinities", AuditLimits(clip_run=2))
    assert got.nonfinite == (2, 3)
    assert (got.clip_events, got.clip_longest, got.clip_first) == ((2, 1), (5, 2), (500, 2 * S - 2))
    assert got.peak == (1.0, 1.0) and all(math.isfinite(v) for v in got.sum + got.sumsq + (got.sum_lr,))
    assert (got.gap_longest, got.gap_at) == (5, 3005)
    assert got.findings()[0] == ("nonfinite", 5, 0)


# ---- integer PCM --------------------------------------------------------------------------------------------------------
def pcm(n, bits, seed):
    """Random samples of the full range with both extremes and a run at either rail; as a file holds them."""
    rng = np.random.default_rng(seed)
    low, high = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    v = rng.integers(low, high + 1, size=(n, 2), dtype=np.int64)
    v[0], v[n - 1] = (low, high), (high, low)
    if n > 40:
        v[10:14, 0], v[20:25, 1] = high, low
        v[30:33] = 0
    if bits == 16:
        return v.astype(np.int16)
    if bits == 32:
        return v.astype(np.int32)
    u = (v & 0xFFFFFF).astype(np.uint32)
    return np.stack([(u >> s) & 0xFF for s in (0, 8, 16)], axis=-1).astype(np.uint8).reshape(n, 6)


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_integer_pcm(dev, bits):
    """n odd and even, short and across segments: the packed 24-bit stream ends at every byte alignment (6 n mod 16)."""
    for n in (1, 2, 3, 5, 8, S + 1, S + 2, S + 3, S + 4, 2 * S + 7):
        got = check(dev, pcm(n, bits, n), bits, 48000, f"{bits} bits, {n} frames")
        assert got.bits == bits and (n == 1 or got.peak == (1.0, 1.0))
    if bits == 16:
        x = np.zeros((S + 9, 2), dtype=np.int16)
        x[S - 2:S + 2, 0], x[100:103, 1] = 32767, -32768             # both rails at the default clip_level 1 - 2^-15
        got = check(dev, x, 16, 44100, "16 bits, both rails")
        assert got.clip_events == (1, 1) and got.clip_first == (S - 2, 100) and got.clip_longest == (4, 3)
        x[:, 1] = np.where(x[:, 1] == -32768, -32767, x[:, 1])       # one step inside: still at the rail
        x[S - 2:S + 2, 0] = 32766                                    # two steps: not
        got = check(dev, x, 16, 44100, "16 bits, one and two steps inside")
        assert got.clip_events == (0, 1)


# ---- the C ABI's edges --------------------------------------------------------------------------------------------------
def test_no_frames_and_refused_arguments(dev):
    lib = _native.library()
    good = AuditLimits().native()
    report = _native.MgxAuditReport()
    count = ctypes.c_int64(-5)
    x = noise(S + 5, 1)
    with dev.lock:
        buf = dev.upload(x)
        try:
            call = lambda h, p, n, bits, rate, limits, rep, sums=None, capacity=0: lib.mgx_audit(      # noqa: E731
                h, ctypes.c_void_p(p) if p else None, n, bits, rate, None if limits is None else ctypes.byref(limits),
                None if rep is None else ctypes.byref(rep), sums, capacity, ctypes.byref(count))
            assert call(dev.handle, None, 0, 0, 44100, good, report) == 0, lib.mgx_last_error()
            assert count.value == 0 and report.frames == 0 and report.sub_blocks == 0 and report.sub_block_frames == 4410
            assert (report.head_silence, report.tail_silence, report.gap_longest, report.gap_at) == (0, 0, 0, -1)
            assert tuple(report.clip_first) == (-1, -1) and report.correlation_min_at == -1
            assert tuple(report.nonfinite) + tuple(report.clip_events) + tuple(report.clip_longest) == (0,) * 6
            assert tuple(report.sum) + tuple(report.sumsq) + tuple(report.peak) == (0.0,) * 6
            assert all(math.isnan(v) for v in (report.dc[0], report.dc[1], report.rms[0], report.rms[1], report.balance_db,
                                               report.correlation, report.mono_loss_db, report.correlation_min))

            def limits(**changes):
                value = AuditLimits().native()
                for name, v in changes.items():
                    setattr(value, name, v)
                return value

            room = (ctypes.c_double * 3)()
            n = x.shape[0]
            refused = [
                ((None, buf.ptr, n, 0, 44100, good, report), "h"),
                ((dev.handle, buf.ptr, n, 0, 44100, None, report), "limits"),
                ((dev.handle, buf.ptr, n, 0, 44100, good, None), "report"),
                ((dev.handle, None, n, 0, 44100, good, report), "x_dev"),
                ((dev.handle, buf.ptr + 8, n - 1, 0, 44100, good, report), "x_dev"),
                ((dev.handle, buf.ptr, -1, 0, 44100, good, report), "n_frames"),
                ((dev.handle, buf.ptr, n, 8, 44100, good, report), "bits"),
                ((dev.handle, buf.ptr, n, 0, 7999, good, report), "sample_rate"),
                ((dev.handle, buf.ptr, n, 0, 44100, limits(clip_level=0.0), report), "clip_level"),
                ((dev.handle, buf.ptr, n, 0, 44100, limits(clip_level=math.inf), report), "clip_level"),
                ((dev.handle, buf.ptr, n, 0, 44100, limits(clip_level=math.nan), report), "clip_level"),
                ((dev.handle, buf.ptr, n, 0, 44100, limits(clip_run=0), report), "clip_run"),
                ((dev.handle, buf.ptr, n, 0, 44100, limits(silence_level=-1e-9), report), "silence_level"),
                ((dev.handle, buf.ptr, n, 0, 44100, limits(silence_level=math.nan), report), "silence_level"),
                ((dev.handle, buf.ptr, n, 0, 44100, good, report, room, 0), "capacity"),
            ]
            for args, word in refused:
                assert call(*args) == _native.ERR_ARGUMENT, word
                assert lib.mgx_last_error().decode().startswith(word + ":"), (word, lib.mgx_last_error())
            assert call(dev.handle, buf.ptr, n, 0, 44100, good, report, room, 1) == 0, lib.mgx_last_error()
            assert count.value == 1 and report.frames == n and room[0] == report.sumsq[0] > 0.0
        finally:
            buf.release()
    check(dev, x, 0, 44100, "the handle after the refusals")


# ---- the Python surface -------------------------------------------------------------------------------------------------
def test_audit_takes_what_measure_takes(dev, tmp_path):
    from matchering_amd.device import DeviceFrames

    rate = 44100
    x = noise(2 * S + 100, 8)
    ints = np.round(x * 32767.0).astype(np.int16)
    ints[50:53, 0] = 32767
    want = oracle.audit(x, 0, rate)
    assert_audit(mg.audit(x, rate), None, want, "a float array")
    assert_audit(mg.audit(x.astype(np.float64), rate), None, want, "a float64 array")
    both = np.repeat(x[:, :1], 2, axis=1)
    for mono in (x[:, 0], x[:, :1]):
        got = mg.audit(mono)                                        # (the Config's internal rate: 44100)
        assert_audit(got, None, oracle.audit(both, 0, rate), "a mono float array")
        assert got.correlation == 1.0 and got.mono_loss_db == 0.0
    got = mg.audit(ints, 48000)
    assert_audit(got, None, oracle.audit(ints, 16, 48000), "an int16 array")
    assert got.bits == 16 and got.sample_rate == 48000 and got.clip_events == (1, 0)
    assert_audit(mg.audit(ints[:, :1], rate), None, oracle.audit(np.repeat(ints[:, :1], 2, axis=1), 16, rate), "a mono int16 array")
    with dev.lock:
        frames = DeviceFrames(dev.upload(x), x.shape[0])
    try:
        assert_audit(mg.audit(frames, rate, limits=AuditLimits(clip_level=0.2, clip_run=1)), None,
                     oracle.audit(x, 0, rate, clip_level=0.2, clip_run=1), "DeviceFrames")
    finally:
        frames.release()
    path = str(tmp_path / "track.wav")
    audio_io.write_wav(path, ints, rate, "PCM_16")
    got = mg.audit(path)
    assert_audit(got, None, oracle.audit(ints.astype(np.float32) / 32768.0, 0, rate), "a path")
    assert got.bits == 0 and len(str(got).splitlines()) == 3
    with pytest.raises(ValueError):
        mg.audit(np.zeros((10, 3), dtype=np.float32))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    folder = tmp_path_factory.mktemp("audit_pair")
    target, reference = make_pair(2.0, 44100, pair=81, reference_seconds=1.8)
    audio_io.save(str(folder / "target.wav"), target, 44100, "FLOAT")
    audio_io.save(str(folder / "reference.wav"), reference, 44100, "FLOAT")
    return folder, target, reference


def results_in(folder):
    os.makedirs(folder, exist_ok=True)
    return [mg.pcm16(os.path.join(folder, "plain.wav")),
            mg.Result(os.path.join(folder, "delivered.wav"), "PCM_16", delivery=Delivery(loudness=-14.0, true_peak=-1.0, dither="tpdf", seed=3))]


def test_process_audits_tracks_renderings_and_the_file_as_written(dev, files, tmp_path):
    folder, target, reference = files
    seen = {}
    with_audit, without = str(tmp_path / "with"), str(tmp_path / "without")
    mg.process(str(folder / "target.wav"), str(folder / "reference.wav"), results_in(with_audit),
               audit=lambda name, value: seen.__setitem__(name, value))
    written = os.path.join(with_audit, "delivered.wav")
    assert list(seen) == ["target", "reference", "result", "delivered:" + written]
    assert_audit(seen["target"], None, oracle.audit(target, 0, 44100), "target")
    assert_audit(seen["reference"], None, oracle.audit(reference, 0, 44100), "reference")
    assert seen["reference"].clip_events[0] > 0                      # (the synthetic reference is clipped)
    assert seen["result"].frames == target.shape[0] and seen["result"].bits == 0
    samples, rate = audio_io.read_wav(written, pcm=True)
    assert rate == 44100 and samples.dtype == np.int16
    assert_audit(seen["delivered:" + written], None, oracle.audit(samples, 16, 44100), "the file as written")
    assert seen["delivered:" + written].bits == 16
    mg.process(str(folder / "target.wav"), str(folder / "reference.wav"), results_in(without))
    for name in ("plain.wav", "delivered.wav"):
        assert open(os.path.join(with_audit, name), "rb").read() == open(os.path.join(without, name), "rb").read(), name


def test_a_batch_job_carries_its_audits(dev, files, tmp_path):
    folder, target, reference = files
    jobs = [{"target": str(folder / "target.wav"), "reference": str(folder / "reference.wav"),
             "results": results_in(str(tmp_path / "a")), "audit": True},
            {"target": str(folder / "target.wav"), "reference": str(folder / "reference.wav"),
             "results": results_in(str(tmp_path / "b"))}]
    assert mg.process_batch(jobs, rank=0, world_size=1, lanes=1) == [0, 1]
    carried = jobs[0]["audit"]
    written = os.path.join(str(tmp_path / "a"), "delivered.wav")
    assert list(carried) == ["target", "reference", "result", "delivered:" + written]
    assert all(type(value) is dict for value in carried.values()) and "audit" not in jobs[1]
    samples, _ = audio_io.read_wav(written, pcm=True)
    want = oracle.audit(samples, 16, 44100)
    for name in ("frames", "bits", "head_silence", "gap_longest"):
        assert carried["delivered:" + written][name] == want[name]
    assert carried["delivered:" + written]["peak"] == list(want["peak"]) and carried["target"]["frames"] == target.shape[0]
    for name in ("plain.wav", "delivered.wav"):
        assert open(os.path.join(str(tmp_path / "a"), name), "rb").read() == open(os.path.join(str(tmp_path / "b"), name), "rb").read()


def test_audit_report_example_runs(files, tmp_path, monkeypatch):
    from conftest import ROOT

    folder, target, reference = files
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr("sys.argv", ["audit_report.py", str(folder / "target.wav"), str(folder / "reference.wav")])
    lines = []
    monkeypatch.setattr("builtins.print", lambda *a, **k: lines.append(" ".join(str(v) for v in a)))
    try:
        runpy.run_path(os.path.join(ROOT, "examples", "audit_report.py"), run_name="__main__")
    finally:
        mg.log()                                    # the example installs handlers: put the defaults back
    assert os.path.exists(tmp_path / "my_song_master_16bit.wav")
    assert any(line.lstrip().startswith("target:") for line in lines) and any("delivered:" in line for line in lines)
    assert any("clipping" in line for line in lines)                 # the clipped reference is found out
