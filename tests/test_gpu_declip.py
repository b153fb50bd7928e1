"""Clip repair on the MI355X: ``mgx_declip`` through the C ABI against tests/declip_oracle.py -- output bytes and every
field of the report equal -- at the lengths where a segment begins, on runs placed around the segment borders and the
track's ends, on samples that are not finite, on whole-track cases and at its argument edges; then through
``repair_clipping``, ``process(..., repair=)``, a batch job and the example.

Shapes: a segment is 4096 frames with a halo of 514, so three segments reach every path; the global offsets are 64-bit and
no index leaves 32 bits below the 500 million frames ``mgx_declip`` accepts.  Everything is an equality: the definition
fixes every bit."""

import ctypes
import os
import runpy

import numpy as np
import pytest

import declip_oracle as oracle
import matchering_amd as mg
from matchering_amd import _native, audio_io
from matchering_amd.synth import make_pair

pytestmark = pytest.mark.gpu

S = 4096
INTS = ("runs_repaired", "samples_repaired", "samples_raised", "longest_repaired", "first_repaired", "runs_short", "runs_long",
        "runs_edge")


@pytest.fixture(scope="module")
def dev():
    from matchering_amd.device import default_device

    return default_device()


def params_of(level, min_run=2, max_run=32, max_rise=2.0):
    return _native.MgxDeclipParams(float(level), float(max_rise), int(min_run), int(max_run))


def repaired(dev, x, level, **kw):
    """(out (n, 2) float32, report as the oracle's dict) of float32 frames through ``mgx_declip``."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 2)
    with dev.lock:
        buf = dev.upload(x)
        out = None
        try:
            out, report = dev.declip(buf, x.shape[0], params_of(level, **kw))
            got = np.array(dev.download(out, x.shape)) if x.shape[0] else x.copy()
        finally:
            buf.release()
            if out is not None:
                out.release()
    found = {name: tuple(int(v) for v in getattr(report, name)) for name in INTS}
    found["peak_before"], found["peak_after"] = tuple(report.peak_before), tuple(report.peak_after)
    return got, found


def assert_same(dev, x, level, label, **kw):
    want, want_report = oracle.declip(x, level, **kw)
    got, got_report = repaired(dev, x, level, **kw)
    assert got_report == want_report, (label, got_report, want_report)
    assert got.tobytes() == want.tobytes(), (label, int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32))))
    return got, want_report


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 517, 4 * 4096 + 1])
def test_lengths(dev, n):
    _, report = assert_same(dev, oracle.random_track(n, 100 + n % 97, nonfinite=2 if n > 8 else 0), 0.8, n)
    if n > 4096:
        assert min(report["runs_repaired"]) > 0 and min(report["samples_raised"]) > 0


@pytest.mark.parametrize("max_run", [32, 512])
def test_runs_around_a_segment_border_and_the_tracks_ends(dev, max_run):
    seen = {}
    for name, (n, runs) in oracle.border_cases(S, max_run).items():
        _, seen[name] = assert_same(dev, oracle.track_with(n, runs), 0.8, name, max_run=max_run)
    assert seen["max_run_across"]["longest_repaired"] == (max_run, max_run)
    assert seen["max_run_plus_one_across"]["runs_long"] == (1, 1)
    assert seen["min_run_less_one"]["runs_short"] == (2, 2) and seen["min_run"]["runs_repaired"] == (2, 2)
    assert seen["track_ends"]["runs_edge"] == (2, 2)


def test_nonfinite_anchors_and_a_nonfinite_sample_inside_a_run(dev):
    n = 2 * S + 9
    for bad in (np.nan, np.inf):
        for at in (S - 5, S - 4, S + 3, S + 4, S):               # the anchors of [S - 3, S + 3), and a sample inside it
            x = oracle.track_with(n, [(0, S - 3, 6, 1), (1, S - 3, 6, -1)])
            x[at, :] = bad
            _, report = assert_same(dev, x, 0.8, (bad, at))
            assert report["runs_edge"] == ((2, 2) if at == S else (1, 1)) and report["runs_repaired"] == (0, 0)


def test_a_clean_track_is_copied_and_a_track_at_the_rail_is_left(dev):
    x = oracle.quiet(3 * S + 77, 3)
    x[S + 5, 0], x[2 * S, 1] = np.nan, -np.inf                  # (copied bit for bit as well)
    got, report = assert_same(dev, x, 0.8, "clean")
    assert got.tobytes() == x.tobytes() and report["peak_after"] == report["peak_before"]
    rail = np.full((3 * S + 9, 2), 1.0, dtype=np.float32)
    rail[:, 1] = -1.0
    got, report = assert_same(dev, rail, 1.0, "rail", max_run=512)
    assert got.tobytes() == rail.tobytes() and report["runs_long"] == (1, 1)


def test_max_rise_binds(dev):
    x = oracle.quiet(S + 200, 5, 0.01)
    x[S - 6:S + 6, 0] = [-0.5, 0.75, 0.8, 0.8, 0.8, 0.8, 0.8, 0.8, 0.8, 0.8, 0.75, -0.5]
    x[S - 6:S + 6, 1] = -x[S - 6:S + 6, 0]
    _, capped = assert_same(dev, x, 0.8, "capped", max_rise=1.05)
    _, loose = assert_same(dev, x, 0.8, "loose", max_rise=4.0)
    assert capped["peak_after"] == (float(np.float32(1.05 * 0.8)),) * 2 and loose["peak_after"][0] > 1.5


def test_two_calls_give_equal_bytes(dev):
    x = oracle.random_track(3 * S + 11, 42)
    a, ra = repaired(dev, x, 0.8)
    b, rb = repaired(dev, x, 0.8)
    assert a.tobytes() == b.tobytes() and ra == rb


def test_a_queued_call_without_a_report(dev):
    x = oracle.random_track(2 * S + 3, 43)
    want, _ = oracle.declip(x, 0.8)
    with dev.lock:
        buf = dev.upload(x)
        out, report = dev.declip(buf, x.shape[0], params_of(0.8), report=False)
        got = np.array(dev.download(out, x.shape))
        buf.release(), out.release()
    assert report is None and got.tobytes() == want.tobytes()


def test_argument_refusals(dev):
    lib = _native.library()
    x = oracle.quiet(64, 1)
    with dev.lock:
        buf, out = dev.upload(x), dev.alloc(64 * 8)
        dev.synchronize()
        p, rep = params_of(0.8), _native.MgxDeclipReport()
        h, xp, op = dev.handle, ctypes.c_void_p(buf.ptr), ctypes.c_void_p(out.ptr)

        def refused(rc, word, code=_native.ERR_ARGUMENT):
            message = lib.mgx_last_error().decode()
            assert rc == code and word in message, (rc, message)

        refused(lib.mgx_declip(None, xp, 64, ctypes.byref(p), op, ctypes.byref(rep)), "h:")
        refused(lib.mgx_declip(h, None, 64, ctypes.byref(p), op, ctypes.byref(rep)), "x_dev")
        refused(lib.mgx_declip(h, xp, 64, ctypes.byref(p), None, ctypes.byref(rep)), "out_dev")
        refused(lib.mgx_declip(h, xp, 64, None, op, ctypes.byref(rep)), "params")
        refused(lib.mgx_declip(h, xp, -1, ctypes.byref(p), op, ctypes.byref(rep)), "n_frames")
        refused(lib.mgx_declip(h, xp, 64, ctypes.byref(p), xp, ctypes.byref(rep)), "overlaps")
        refused(lib.mgx_declip(h, xp, 32, ctypes.byref(p), ctypes.c_void_p(buf.ptr + 128), ctypes.byref(rep)), "overlaps")
        refused(lib.mgx_declip(h, ctypes.c_void_p(buf.ptr + 8), 32, ctypes.byref(p), op, ctypes.byref(rep)), "x_dev")
        refused(lib.mgx_declip(h, xp, 32, ctypes.byref(p), ctypes.c_void_p(out.ptr + 8), ctypes.byref(rep)), "out_dev")
        refused(lib.mgx_declip(h, xp, 500_000_001, ctypes.byref(p), op, ctypes.byref(rep)), "500 million", _native.ERR_UNSUPPORTED)
        refused(lib.mgx_declip(h, xp, 64, ctypes.byref(params_of(0.8, max_run=513)), op, ctypes.byref(rep)), "max_run")
        # n == 0 succeeds and launches nothing; the handle is good for the next call
        assert lib.mgx_declip(h, xp, 0, ctypes.byref(p), op, ctypes.byref(rep)) == 0 and tuple(rep.first_repaired) == (-1, -1)
        assert lib.mgx_declip(h, xp, 64, ctypes.byref(p), op, ctypes.byref(rep)) == 0
        assert np.array(dev.download(out, x.shape)).tobytes() == x.tobytes()
        buf.release(), out.release()


# ---- end to end ---------------------------------------------------------------------------------------------------------
MAX_RISE = 10.0 ** (6.0 / 20.0)                     # ClipRepair's default, 6 dB


def default_level(x):
    """ClipRepair()'s level on a track: its peak lowered by 0.1 dB."""
    return float(np.max(np.abs(x))) * 10.0 ** (-0.1 / 20.0)


def assert_found(found, want, level, frames):
    assert found.level == level and found.frames == frames
    for name in oracle.FIELDS:
        assert getattr(found, name) == want[name], (name, getattr(found, name), want[name])


def test_repair_clipping_of_a_16_bit_file_finds_both_rails(dev, tmp_path):
    t = np.arange(3 * S + 100) / 44100.0
    hot = 1.4 * np.stack([np.sin(2 * np.pi * 997.0 * t), np.sin(2 * np.pi * 1499.0 * t + 1.0)], axis=1)
    pcm = np.clip(np.rint(hot * 32768.0), -32768, 32767).astype(np.int16)
    path = str(tmp_path / "clipped16.wav")
    audio_io.save(path, pcm, 44100, "PCM_16")
    x = (pcm.astype(np.float64) / 32768.0).astype(np.float32)
    assert x.max() == np.float32(32767 / 32768) and x.min() == -1.0
    level = default_level(x)
    want, want_report = oracle.declip(x, level, 2, 32, MAX_RISE)
    frames, found = mg.repair_clipping(path)
    assert frames.dtype == np.float32 and frames.tobytes() == want.tobytes()
    assert_found(found, want_report, level, x.shape[0])
    assert min(found.runs_repaired) > 100 and max(found.peak_after) > 1.0
    # both rails: about as many high runs as low ones were rebuilt, so about half would be missing with one rail
    high_only = oracle.declip(np.where(x < 0, 0, x), level, 2, 32, MAX_RISE)[1]
    assert high_only["runs_repaired"][0] < 0.6 * found.runs_repaired[0]
    # an array gives the same, and a silent one comes back as it is
    again, found_again = mg.repair_clipping(x)
    assert again.tobytes() == want.tobytes() and found_again == found
    silent, nothing = mg.repair_clipping(np.zeros((100, 2), dtype=np.float32))
    assert not silent.any() and nothing.level == 0.0 and nothing.runs_repaired == (0, 0) and "silent" in nothing.describe()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    folder = tmp_path_factory.mktemp("declip_pair")
    target, reference = make_pair(2.0, 44100, pair=83, reference_seconds=1.8)
    ceiling = np.float32(0.45 * np.max(np.abs(target)))
    clipped = np.clip(target, -ceiling, ceiling).astype(np.float32)
    level = default_level(clipped)
    mended, report = oracle.declip(clipped, level, 2, 32, MAX_RISE)
    audio_io.save(str(folder / "target.wav"), clipped, 44100, "FLOAT")
    audio_io.save(str(folder / "mended.wav"), mended, 44100, "FLOAT")
    audio_io.save(str(folder / "reference.wav"), reference, 44100, "FLOAT")
    return folder, clipped, level, report


def results_in(folder):
    os.makedirs(folder, exist_ok=True)
    return [mg.pcm24(os.path.join(folder, "limited.wav")),
            mg.Result(os.path.join(folder, "plain.wav"), "PCM_16", use_limiter=False, normalize=False)]


def same_files(a, b):
    return all(open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read()
               for name in ("limited.wav", "plain.wav"))


def test_process_masters_the_repaired_target(dev, files, tmp_path):
    folder, clipped, level, report = files
    assert min(report["runs_repaired"]) > 10 and min(report["samples_raised"]) > 10
    seen, heard = {}, {}
    repaired, by_oracle, plain, none = (str(tmp_path / name) for name in ("repaired", "oracle", "plain", "none"))
    mg.process(str(folder / "target.wav"), str(folder / "reference.wav"), results_in(repaired),
               repair=(lambda name, value: seen.__setitem__(name, value), mg.ClipRepair()),
               audit=lambda name, value: heard.__setitem__(name, value))
    assert list(seen) == ["target"]
    assert_found(seen["target"], report, level, clipped.shape[0])
    assert heard["target"].peak == report["peak_after"]             # the "target" callbacks see the repaired frames
    mg.process(str(folder / "mended.wav"), str(folder / "reference.wav"), results_in(by_oracle))
    assert same_files(repaired, by_oracle)
    # without repair nothing changes, and the repair does change the master
    mg.process(str(folder / "target.wav"), str(folder / "reference.wav"), results_in(plain))
    mg.process(str(folder / "target.wav"), str(folder / "reference.wav"), results_in(none), repair=None)
    assert same_files(plain, none) and not same_files(plain, repaired)
    # the JSON forms take the same route
    as_json = str(tmp_path / "json")
    mg.process(str(folder / "target.wav"), str(folder / "reference.wav"), results_in(as_json), repair=True)
    assert same_files(as_json, repaired)


def test_a_batch_job_with_repair(dev, files, tmp_path):
    folder, clipped, level, report = files
    job = {"target": str(folder / "target.wav"), "reference": str(folder / "reference.wav")}
    jobs = [dict(job, results=results_in(str(tmp_path / "a")), repair=True),
            dict(job, results=results_in(str(tmp_path / "b"))),
            dict(job, target=str(folder / "mended.wav"), results=results_in(str(tmp_path / "c")))]
    assert mg.process_batch(jobs, rank=0, world_size=1, lanes=1) == [0, 1, 2]
    assert jobs[0]["repaired"]["runs_repaired"] == list(report["runs_repaired"]) and jobs[0]["repaired"]["level"] == level
    assert "repaired" not in jobs[1]
    assert same_files(str(tmp_path / "a"), str(tmp_path / "c")) and not same_files(str(tmp_path / "a"), str(tmp_path / "b"))


def test_clip_repair_example_runs(tmp_path, monkeypatch):
    from conftest import ROOT

    monkeypatch.setattr("sys.argv", ["clip_repair.py", str(tmp_path)])
    lines = []
    monkeypatch.setattr("builtins.print", lambda *a, **k: lines.append(" ".join(str(v) for v in a)))
    try:
        runpy.run_path(os.path.join(ROOT, "examples", "clip_repair.py"), run_name="__main__")
    finally:
        mg.log()
    described = [line for line in lines if "clip repair at" in line]
    assert len(described) == 2 and described[1].startswith("target:")
    assert os.path.exists(tmp_path / "master.wav") and os.path.exists(tmp_path / "master_repaired.wav")
    errors = [float(line.split("mix ")[1].split(" dB")[0]) for line in lines if "RMS error" in line]
    assert len(errors) == 2 and errors[1] <= errors[0]
