"""The visuals on the MI355X: ``mgx_spectrogram`` and ``mgx_overview`` through the C ABI against tests/visuals_oracle.py
-- every transform length in both channel modes, the hops that hang over either end of a track, the column and run
splits, closed forms -- and through ``mg.spectrogram``, ``mg.overview``, ``process(..., visuals=)``, a batch job and the
example.

Shapes: n is at most about 40 K frames (2.5 transforms of 16384 points); a run of a column is RUN_CAP = 32 hops, reached
with 256-point transforms one frame apart; a share of an overview column is 16384 frames.
Spectrogram bound (tests/stage_sweeps.py's form): the reference is the float64 oracle on the float32 input, the error is
max |got - want| / max(want) per channel and picture, and the bound is the analysis bound carried to power: 2e-6 of the
peak bin in magnitude (check_analysis) is 4e-6 in power to first order.  Beside it the yardstick -- scipy's float32
transform of the float32 windowed hops, pooled identically -- is printed, and eight times the yardstick must lie under
the bound: the inputs are ones an unrelated float32 transform passes with room.
Overview bound: the least and largest samples equal the oracle's; a float64 sum of `count` exact squares lies within
count 2^-52 sum|terms| of the exact sum, the audit's bound.
"""

import ctypes
import os
import runpy

import numpy as np
import pytest

import matchering_amd as mg
import visuals_oracle as oracle
from matchering_amd import _native, audio_io, visuals
from matchering_amd.synth import make_pair

pytestmark = pytest.mark.gpu

BOUND = 4e-6
RUN_CAP = 32          # csrc/visuals_plan.h SPECTRO_RUN_CAP (tests/test_visuals_emu.py holds the constant to this)
SHARE = 16384         # OVERVIEW_SHARE


@pytest.fixture(scope="module")
def dev():
    from matchering_amd.device import default_device

    return default_device()


def track(n, seed, fft_size, tone_bin=None):
    """Noise at -20 dB plus a tone per channel, on bin centres of the transform."""
    rng = np.random.default_rng(seed)
    x = 0.1 * rng.standard_normal((n, 2)).astype(np.float32)
    tone_bin = fft_size // 8 if tone_bin is None else tone_bin
    t = np.arange(n)
    x[:, 0] += (0.5 * np.sin(2 * np.pi * tone_bin * t / fft_size)).astype(np.float32)
    x[:, 1] += (0.25 * np.cos(2 * np.pi * (tone_bin + 3) * t / fft_size)).astype(np.float32)
    return x


def drawn(dev, x, fft_size, hop, columns, edges, mode="lr"):
    x = np.ascontiguousarray(x, dtype=np.float32)
    with dev.lock:
        buf = dev.upload(x)
        try:
            return dev.spectrogram(buf, x.shape[0], 44100, fft_size, hop, columns, edges, mode)
        finally:
            buf.release()


def surveyed(dev, x, columns):
    x = np.ascontiguousarray(x, dtype=np.float32)
    with dev.lock:
        buf = dev.upload(x)
        try:
            return dev.overview(buf, x.shape[0], 44100, columns)
        finally:
            buf.release()


def errors(values, want):
    return [float(np.max(np.abs(values[:, ch] - want[:, ch])) / np.max(want[:, ch])) for ch in range(2)]


def check(dev, x, fft_size, hop, columns, edges, mode, label, powers=None):
    """The picture of the GPU against the oracle's, with the yardstick beside it.  ``powers``: (float64, float32) hop
    powers of x where the caller has them already."""
    exact, single = powers if powers is not None else (oracle.hop_powers(x, fft_size, hop, mode),
                                                       oracle.hop_powers(x, fft_size, hop, mode, float32=True))
    width = oracle.plan(x.shape[0], hop, columns)[1]
    want, yard = oracle.pool(exact, width, edges), oracle.pool(single, width, edges)
    got = drawn(dev, x, fft_size, hop, columns, edges, mode)
    assert got.power.shape == want.shape and got.power.dtype == np.float32, (label, got.power.shape, want.shape)
    assert got.hops == exact.shape[0] and got.columns == width
    error, yardstick = errors(got.power.astype(np.float64), want), errors(yard, want)
    print(f"{label}: error {error[0]:.3e} {error[1]:.3e}, yardstick {yardstick[0]:.3e} {yardstick[1]:.3e}, bound {BOUND:.1e}")
    assert 8.0 * max(yardstick) <= BOUND, (label, yardstick)
    assert max(error) <= BOUND, (label, error)
    return got


# ---- every transform length ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["lr", "ms"])
@pytest.mark.parametrize("log2_fft", [8, 9, 10, 11, 12, 13, 14])
def test_every_length_in_both_modes(dev, log2_fft, mode):
    fft_size = 1 << log2_fft
    n, hop = 5 * fft_size // 2 + 3, fft_size // 4
    x = track(n, log2_fft, fft_size)
    powers = (oracle.hop_powers(x, fft_size, hop, mode), oracle.hop_powers(x, fft_size, hop, mode, float32=True))
    check(dev, x, fft_size, hop, 0, visuals.log_bands(fft_size, 44100, 48), mode, f"N {fft_size} {mode} log bands", powers)
    check(dev, x, fft_size, hop, 0, visuals.linear_bands(fft_size), mode, f"N {fft_size} {mode} every bin", powers)
    check(dev, x, fft_size, hop, 3, visuals.log_bands(fft_size, 44100, 48), mode, f"N {fft_size} {mode} pooled", powers)


# ---- edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 256, 257, 511, 512, 1025])
def test_short_tracks(dev, n):
    """n in {1, H, H + 1, N/2 - 1, N/2, N + 1}: every hop hangs over the start, the end or both."""
    x = track(n, n, 1024)
    check(dev, x, 1024, 256, 0, visuals.linear_bands(1024), "lr", f"n {n}")
    check(dev, x, 1024, 256, 1, visuals.log_bands(1024, 44100, 16), "ms", f"n {n} one column")


@pytest.mark.parametrize("fft_size, hop, n", [(1024, 1024, 3000), (256, 1, 300), (4096, 1000, 10240)])
def test_hops(dev, fft_size, hop, n):
    """No overlap; a hop of one frame; a hop that does not divide N."""
    check(dev, track(n, hop, fft_size), fft_size, hop, 0, visuals.linear_bands(fft_size), "lr", f"N {fft_size} hop {hop}")


def test_columns(dev):
    fft_size, hop, n = 512, 128, 5000
    x = track(n, 40, fft_size)
    powers = (oracle.hop_powers(x, fft_size, hop), oracle.hop_powers(x, fft_size, hop, float32=True))
    hops = powers[0].shape[0]
    assert hops == 40
    for columns in (hops, hops - 1, 2, 1):
        check(dev, x, fft_size, hop, columns, visuals.linear_bands(fft_size), "lr", f"{columns} columns of {hops} hops", powers)


@pytest.mark.parametrize("count", [RUN_CAP - 1, RUN_CAP, RUN_CAP + 1, 2 * RUN_CAP + 3])
def test_a_column_split_over_workgroups(dev, count):
    """One column of `count` hops: one run short of the cap, exactly the cap, the cap and one, two caps and three."""
    fft_size, hop = 256, 16
    n = (count - 1) * hop + 1
    x = track(n, count, fft_size)
    assert oracle.hops(n, hop) == count
    check(dev, x, fft_size, hop, 1, visuals.linear_bands(fft_size), "lr", f"{count} hops in one column")
    check(dev, x, fft_size, hop, 2, visuals.log_bands(fft_size, 44100, 12), "ms", f"{count} hops in two columns")


def test_one_band_and_every_bin(dev):
    fft_size = 256
    x = track(1000, 77, fft_size)
    check(dev, x, fft_size, 64, 0, np.array([0, fft_size // 2 + 1], dtype=np.int32), "lr", "one band of every bin")
    check(dev, x, fft_size, 64, 0, np.array([5, 9], dtype=np.int32), "lr", "one band of four bins")
    got = check(dev, x, fft_size, 64, 0, visuals.linear_bands(fft_size), "ms", "B = N/2 + 1")
    assert got.power.shape[2] == fft_size // 2 + 1


# ---- closed forms ------------------------------------------------------------------------------------------------------
def test_a_stretch_of_zeros_reads_exactly_zero(dev):
    """Exact zeros for N + H frames and more inside noise: the hops that lie inside it are exactly 0.0 in every bin, so
    nothing of an earlier hop is left in LDS or in an accumulator."""
    fft_size, hop = 1024, 256
    x = track(8000, 9, fft_size)
    x[3000:3000 + 2 * fft_size + hop] = 0.0
    got = drawn(dev, x, fft_size, hop, 0, visuals.linear_bands(fft_size)).power
    inside = [t for t in range(got.shape[0]) if t * hop - fft_size // 2 >= 3000 and t * hop + fft_size // 2 <= 3000 + 2 * fft_size + hop]
    assert len(inside) >= 4
    for t in range(got.shape[0]):
        assert (not got[t].any()) == (t in inside), t
    pooled = drawn(dev, x, fft_size, hop, 0, visuals.log_bands(fft_size, 44100, 20), "ms").power
    assert all(not pooled[t].any() for t in inside) and pooled[inside[0] - 1].all()


def test_an_impulse_at_either_end_reads_the_window(dev):
    fft_size, hop, n = 1024, 256, 3000
    w = oracle.window(fft_size).astype(np.float64)
    scale = (2.0 / w.sum()) ** 2
    for pos in (0, n - 1):
        x = np.zeros((n, 2), dtype=np.float32)
        x[pos, 0] = 1.0
        x[pos, 1] = -0.5
        got = drawn(dev, x, fft_size, hop, 0, visuals.linear_bands(fft_size)).power.astype(np.float64)
        holding = 0
        for t in range(got.shape[0]):
            inside = pos - (t * hop - fft_size // 2)
            want = w[inside] ** 2 * scale if 0 <= inside < fft_size else 0.0
            holding += want > 0.0
            # (the bound is taken of the largest value an impulse can read, the window's peak)
            assert np.max(np.abs(got[t, 0] - want)) <= BOUND * scale, (pos, t)
            assert np.max(np.abs(got[t, 1] - 0.25 * want)) <= BOUND * scale, (pos, t)
        assert holding >= 2, pos


@pytest.mark.parametrize("log2_fft", [8, 12, 14])
def test_a_full_scale_sine_on_a_bin_centre_reads_one(dev, log2_fft):
    fft_size = 1 << log2_fft
    n, k = 3 * fft_size, fft_size // 16 + 1
    t = np.arange(n)
    x = np.stack([np.sin(2 * np.pi * k * t / fft_size), np.cos(2 * np.pi * (2 * k) * t / fft_size)], axis=1).astype(np.float32)
    got = drawn(dev, x, fft_size, fft_size // 2, 0, visuals.linear_bands(fft_size)).power
    middle = got[2:-2]                                             # hops that lie inside the track
    assert middle.shape[0] >= 1
    assert np.max(np.abs(middle[:, 0, k] - 1.0)) <= BOUND and np.max(np.abs(middle[:, 1, 2 * k] - 1.0)) <= BOUND
    assert np.max(middle[:, 0, k + 2:]) <= BOUND and np.max(middle[:, 1, :2 * k - 1]) <= BOUND


# ---- overview --------------------------------------------------------------------------------------------------------------
def check_overview(dev, x, columns, label):
    got = surveyed(dev, x, columns)
    lo, hi, sq = oracle.overview(x, columns)
    assert got.lo.dtype == np.float32 and got.lo.shape == (columns, 2)
    assert np.array_equal(got.lo, lo) and np.array_equal(got.hi, hi), label
    frames = np.diff(oracle.column_bounds(x.shape[0], columns))
    assert np.array_equal(got.frames_per_column, frames)
    finite = np.isfinite(sq)
    assert np.array_equal(np.isnan(sq), np.isnan(got.sumsq)) and np.array_equal(finite, np.isfinite(got.sumsq)), label
    assert np.array_equal(got.sumsq[~finite & ~np.isnan(sq)], sq[~finite & ~np.isnan(sq)])
    bound = frames[:, None] * 2.0 ** -52 * sq                       # (squares: the terms are their own magnitudes)
    worst = np.abs(got.sumsq[finite] - sq[finite])
    print(f"{label}: worst sum error {worst.max():.3e}, bound there {bound[finite][np.argmax(worst)]:.3e}")
    assert np.all(worst <= bound[finite]), label
    return got


@pytest.mark.parametrize("n", [1, 255, 5000, 2 * SHARE + 1234])
def test_overview_columns(dev, n):
    x = track(n, n + 1, 256)
    for columns in sorted({1, min(2, n), n, max(n - 1, 1)}):
        if columns <= 65536:
            check_overview(dev, x, columns, f"n {n} in {columns} columns")


def test_overview_splits_a_long_column(dev):
    """Columns of more than a share of 16384 frames: two and three workgroups each, folded in order."""
    n = 5 * SHARE + 77
    x = track(n, 3, 256)
    check_overview(dev, x, 2, "two columns of three shares")
    check_overview(dev, x, 3, "three columns of two shares")
    check_overview(dev, x, 1, "one column of six shares")


def test_overview_with_samples_that_are_not_finite(dev):
    x = track(6000, 12, 256)
    x[100, 0], x[101, 0] = np.nan, 7.0
    x[2100, 1], x[4100, 1], x[4200, 0] = np.inf, -np.inf, np.nan
    got = check_overview(dev, x, 3, "NaN and infinities")
    assert got.hi[0, 0] == 7.0 and np.isnan(got.sumsq[0, 0])       # the NaN is skipped by the maximum and poisons the sum
    assert got.hi[1, 1] == np.inf and got.sumsq[1, 1] == np.inf and got.lo[2, 1] == -np.inf
    whole = np.full((10, 2), np.nan, dtype=np.float32)
    got = surveyed(dev, whole, 2)
    assert np.all(got.lo == np.inf) and np.all(got.hi == -np.inf) and np.all(np.isnan(got.sumsq))


# ---- determinism -----------------------------------------------------------------------------------------------------
def test_two_calls_agree_bit_for_bit(dev):
    x = track(20000, 21, 4096)
    for fft_size, hop, columns, edges in ((4096, 1024, 0, visuals.linear_bands(4096)), (256, 1, 3, visuals.log_bands(256, 44100, 24))):
        first = drawn(dev, x, fft_size, hop, columns, edges).power
        surveyed(dev, x[::-1].copy(), 7)                             # (other work on the scratch in between)
        second = drawn(dev, x, fft_size, hop, columns, edges).power
        assert first.tobytes() == second.tobytes()
    long = track(3 * SHARE + 5, 22, 256)
    first = surveyed(dev, long, 2)
    drawn(dev, x, 256, 64, 0, visuals.linear_bands(256))
    second = surveyed(dev, long, 2)
    assert first.lo.tobytes() == second.lo.tobytes() and first.hi.tobytes() == second.hi.tobytes()
    assert first.sumsq.tobytes() == second.sumsq.tobytes()


# ---- the ABI's refusals ----------------------------------------------------------------------------------------------
def test_no_frames_and_refused_arguments(dev):
    lib = _native.library()
    int_p, float_p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    x = track(2000, 1, 256)
    edges = visuals.linear_bands(256)
    power = np.full((40, 2, 129), -1.0, dtype=np.float32)
    minmax, sumsq = np.full((8, 2, 2), -1.0, dtype=np.float32), np.full((8, 2), -1.0)
    with dev.lock:
        buf = dev.upload(x)
        try:
            def spectro(n=2000, log2_fft=8, hop=64, columns=0, channels=0, bands=129, handle=dev.handle, ptr=buf.ptr, table=edges,
                        out=power, capacity=power.size, count=None):
                spec = _native.MgxSpectrogramSpec(log2_fft, hop, columns, channels, bands)
                rc = lib.mgx_spectrogram(handle, ctypes.c_void_p(ptr), n, ctypes.byref(spec),
                                         None if table is None else table.ctypes.data_as(int_p),
                                         None if out is None else out.ctypes.data_as(float_p), capacity, count)
                return rc, lib.mgx_last_error().decode()

            def over(n=2000, columns=8, handle=dev.handle, ptr=buf.ptr, a=minmax, b=sumsq):
                rc = lib.mgx_overview(handle, ctypes.c_void_p(ptr), n, columns, None if a is None else a.ctypes.data_as(float_p),
                                      None if b is None else b.ctypes.data_as(_native.c_double_p))
                return rc, lib.mgx_last_error().decode()

            count = ctypes.c_int64(-1)
            assert spectro(n=0, ptr=None, out=None, capacity=0, count=ctypes.byref(count))[0] == 0 and count.value == 0
            assert over(n=0, ptr=None, a=None, b=None, columns=0)[0] == 0
            assert np.all(power == -1.0) and np.all(minmax == -1.0)  # (nothing launched, nothing written)
            assert spectro(count=ctypes.byref(count))[0] == 0 and count.value == 32 and np.all(power[:32] >= 0.0)
            assert np.all(power[32:] == -1.0)
            for kwargs, code, word, value in (
                    (dict(n=-1), "ERR_ARGUMENT", "n_frames", "-1"),
                    (dict(n=500000001), "ERR_UNSUPPORTED", "n_frames", "500000001"),
                    (dict(log2_fft=7), "ERR_ARGUMENT", "log2_fft", "7"),
                    (dict(log2_fft=15), "ERR_ARGUMENT", "log2_fft", "15"),
                    (dict(hop=0), "ERR_ARGUMENT", "hop", "0"),
                    (dict(hop=257), "ERR_ARGUMENT", "hop", "257"),
                    (dict(channels=2), "ERR_ARGUMENT", "channels", "2"),
                    (dict(bands=0), "ERR_ARGUMENT", "bands", "0"),
                    (dict(bands=130), "ERR_ARGUMENT", "bands", "130"),
                    (dict(table=np.array([0, 3, 3], dtype=np.int32), bands=2), "ERR_ARGUMENT", "edges[2]", "3"),
                    (dict(table=np.array([-2, 3], dtype=np.int32), bands=1), "ERR_ARGUMENT", "edges[0]", "-2"),
                    (dict(table=np.array([0, 130], dtype=np.int32), bands=1), "ERR_ARGUMENT", "edges[1]", "130"),
                    (dict(table=None), "ERR_ARGUMENT", "edges", None),
                    (dict(columns=-3), "ERR_ARGUMENT", "columns", "-3"),
                    (dict(columns=33), "ERR_ARGUMENT", "columns", "33"),
                    (dict(handle=None), "ERR_ARGUMENT", "h", None),
                    (dict(ptr=None), "ERR_ARGUMENT", "x_dev", None),
                    (dict(ptr=buf.ptr + 4), "ERR_ARGUMENT", "x_dev", None),
                    (dict(out=None), "ERR_ARGUMENT", "power", None),
                    (dict(capacity=32 * 2 * 129 - 1), "ERR_ARGUMENT", "capacity", str(32 * 2 * 129 - 1))):
                rc, message = spectro(**kwargs)
                assert rc == getattr(_native, code), (kwargs, message)
                assert message.startswith(word + ":") and (value is None or value in message), (kwargs, message)
            for kwargs, code, word, value in (
                    (dict(n=-1), "ERR_ARGUMENT", "n_frames", "-1"),
                    (dict(n=500000001), "ERR_UNSUPPORTED", "n_frames", "500000001"),
                    (dict(columns=0), "ERR_ARGUMENT", "columns", "0"),
                    (dict(columns=2001), "ERR_ARGUMENT", "columns", "2001"),
                    (dict(n=70000, columns=65537), "ERR_ARGUMENT", "columns", "65537"),
                    (dict(handle=None), "ERR_ARGUMENT", "h", None),
                    (dict(ptr=None), "ERR_ARGUMENT", "x_dev", None),
                    (dict(ptr=buf.ptr + 4), "ERR_ARGUMENT", "x_dev", None),
                    (dict(a=None), "ERR_ARGUMENT", "minmax", None),
                    (dict(b=None), "ERR_ARGUMENT", "sumsq", None)):
                rc, message = over(**kwargs)
                assert rc == getattr(_native, code), (kwargs, message)
                assert message.startswith(word + ":") and (value is None or value in message), (kwargs, message)
            assert over()[0] == 0 and np.all(minmax[:, :, 0] <= minmax[:, :, 1])      # the handle is good for the next call
        finally:
            buf.release()


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_pictures_take_what_measure_takes(dev, tmp_path):
    from matchering_amd.device import DeviceFrames

    rate, fft_size, hop = 44100, 1024, 256
    x = track(6000, 31, fft_size)
    edges = visuals.log_bands(fft_size, rate, 24)
    want = oracle.spectrogram(x, fft_size, hop, 5, edges)
    lo, hi, sq = oracle.overview(x, 16)

    def same(picture, survey, label, spectrum=want, bounds=(lo, hi)):
        assert max(errors(picture.power.astype(np.float64), spectrum)) <= BOUND, label
        assert np.array_equal(survey.lo, bounds[0]) and np.array_equal(survey.hi, bounds[1]), label

    same(mg.spectrogram(x, fft_size, hop, 5, 24, sample_rate=rate), mg.overview(x, 16, sample_rate=rate), "a float array")
    same(mg.spectrogram(x.astype(np.float64), fft_size, hop, 5, edges), mg.overview(x.astype(np.float64), 16), "a float64 array")
    both = np.repeat(x[:, :1], 2, axis=1)
    mono = mg.spectrogram(x[:, 0], fft_size, hop, 5, edges, channels="ms")
    assert max(errors(mono.power.astype(np.float64)[:, :1].repeat(2, axis=1),
                      oracle.spectrogram(both, fft_size, hop, 5, edges, "ms")[:, :1].repeat(2, axis=1))) <= BOUND
    # a mono source goes in two equal columns: no side but what the shared transform's rounding leaks
    assert mono.power[:, 1].max() <= 1e-12 * mono.power[:, 0].max()
    assert np.array_equal(mg.overview(x[:, :1], 16).lo, oracle.overview(both, 16)[0])
    with dev.lock:
        frames = DeviceFrames(dev.upload(x), x.shape[0])
    try:
        same(mg.spectrogram(frames, fft_size, hop, 5, edges, sample_rate=rate), mg.overview(frames, 16, sample_rate=rate), "DeviceFrames")
    finally:
        frames.release()
    path = str(tmp_path / "track.wav")
    ints = np.round(x * 32767.0).astype(np.int16)
    audio_io.write_wav(path, ints, rate, "PCM_16")
    heard = ints.astype(np.float32) / np.float32(32768.0)
    got = mg.spectrogram(path, fft_size, hop, 5, 24)
    same(got, mg.overview(path, 16), "a path", oracle.spectrogram(heard, fft_size, hop, 5, edges), oracle.overview(heard, 16)[:2])
    assert got.sample_rate == rate and got.frames == 6000 and got.hops == 24 and got.times_s.shape == (5,)
    assert got.image().shape == (48, 5) and np.array_equal(got.edges, edges)
    with pytest.raises(ValueError, match="hop"):
        mg.spectrogram("no such file.wav", fft_size, 5000)           # refused before the file is looked for
    with pytest.raises(ValueError):
        mg.spectrogram(np.zeros((10, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="columns"):
        mg.spectrogram(x, fft_size, hop, columns=25)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    folder = tmp_path_factory.mktemp("visuals_pair")
    target, reference = make_pair(2.0, 44100, pair=82, reference_seconds=1.8)
    audio_io.save(str(folder / "target.wav"), target, 44100, "FLOAT")
    audio_io.save(str(folder / "reference.wav"), reference, 44100, "FLOAT")
    return folder, target, reference


SIZES = visuals.VisualsRequest(overview_columns=64, fft_size=1024, hop=512, columns=32, bands=24)


def results_in(folder):
    os.makedirs(folder, exist_ok=True)
    return [mg.pcm16(os.path.join(folder, "plain.wav")), mg.Result(os.path.join(folder, "unlimited.wav"), "PCM_24", use_limiter=False, normalize=False)]


def assert_pictures(value, audio, label):
    edges = SIZES.edges(44100)
    want = oracle.spectrogram(audio, SIZES.fft_size, SIZES.hop, SIZES.columns, edges)
    assert value.spectrogram.power.shape == (32, 2, edges.size - 1), label
    assert max(errors(value.spectrogram.power.astype(np.float64), want)) <= BOUND, label
    lo, hi, sq = oracle.overview(audio, SIZES.overview_columns)
    assert np.array_equal(value.overview.lo, lo) and np.array_equal(value.overview.hi, hi), label
    assert np.allclose(value.overview.sumsq, sq, rtol=1e-12), label


def test_process_draws_tracks_and_renderings(dev, files, tmp_path):
    folder, target, reference = files
    seen = {}
    with_pictures, without = str(tmp_path / "with"), str(tmp_path / "without")
    mg.process(str(folder / "target.wav"), str(folder / "reference.wav"), results_in(with_pictures),
               visuals=(lambda name, value: seen.__setitem__(name, value), SIZES))
    assert list(seen) == ["target", "reference", "result", "result_no_limiter"]
    assert all(type(value) is visuals.Visuals for value in seen.values())
    assert_pictures(seen["target"], target, "target")
    assert_pictures(seen["reference"], reference, "reference")
    assert seen["result"].spectrogram.frames == target.shape[0] and seen["result"].overview.columns == 64
    assert float(np.max(seen["result"].overview.hi)) <= 1.0 and seen["result"].spectrogram.power.max() > 0.0
    mg.process(str(folder / "target.wav"), str(folder / "reference.wav"), results_in(without))
    for name in ("plain.wav", "unlimited.wav"):
        assert open(os.path.join(with_pictures, name), "rb").read() == open(os.path.join(without, name), "rb").read(), name
    drawn_by_default = {}
    mg.process(str(folder / "target.wav"), str(folder / "reference.wav"), [mg.pcm16(os.path.join(without, "again.wav"))],
               visuals=lambda name, value: drawn_by_default.__setitem__(name, value))
    assert list(drawn_by_default) == ["target", "reference", "result"]
    assert drawn_by_default["target"].spectrogram.power.shape == (87, 2, 96)      # a short track: a column per hop
    assert drawn_by_default["target"].overview.columns == 2048
    assert open(os.path.join(without, "again.wav"), "rb").read() == open(os.path.join(without, "plain.wav"), "rb").read()


def test_a_batch_job_carries_its_pictures(dev, files, tmp_path):
    folder, target, reference = files
    sizes = {"overview_columns": 64, "fft_size": 1024, "hop": 512, "columns": 32, "bands": 24}
    jobs = [{"target": str(folder / "target.wav"), "reference": str(folder / "reference.wav"),
             "results": results_in(str(tmp_path / "a")), "visuals": sizes},
            {"target": str(folder / "target.wav"), "reference": str(folder / "reference.wav"),
             "results": results_in(str(tmp_path / "b"))}]
    assert mg.process_batch(jobs, rank=0, world_size=1, lanes=1) == [0, 1]
    carried = jobs[0]["visuals"]
    assert list(carried) == ["target", "reference", "result", "result_no_limiter"] and "visuals" not in jobs[1]
    assert all(type(value) is dict and set(value) == {"overview", "spectrogram"} for value in carried.values())
    lo, hi, _ = oracle.overview(target, 64)
    assert carried["target"]["overview"]["lo"] == lo.tolist() and carried["target"]["overview"]["hi"] == hi.tolist()
    power = np.asarray(carried["target"]["spectrogram"]["power"])
    assert max(errors(power, oracle.spectrogram(target, 1024, 512, 32, SIZES.edges(44100)))) <= BOUND
    for name in ("plain.wav", "unlimited.wav"):
        assert open(os.path.join(str(tmp_path / "a"), name), "rb").read() == open(os.path.join(str(tmp_path / "b"), name), "rb").read()


def test_visuals_report_example_runs(tmp_path, monkeypatch):
    from conftest import ROOT
    from test_visuals_host import read_png

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr("sys.argv", ["visuals_report.py", "3"])
    lines = []
    monkeypatch.setattr("builtins.print", lambda *a, **k: lines.append(" ".join(str(v) for v in a)))
    try:
        runpy.run_path(os.path.join(ROOT, "examples", "visuals_report.py"), run_name="__main__")
    finally:
        mg.log()
    for name in ("visuals_before.png", "visuals_after.png", "visuals_reference.png"):
        picture = read_png(str(tmp_path / name))
        assert picture.shape[0] == 2 * 96 and picture.shape[1] >= 100 and picture.max() > picture.min(), name
    assert any("long-term average spectrum" in line for line in lines)
    assert sum(len(line.split()) == 4 and line.split()[0].isdigit() for line in lines) >= 20, lines
