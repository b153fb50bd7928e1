"""tests/boundary_cases.py on the CPU: the case generators satisfy their own conditions (a wrapping length wraps, a tail of
each size exists, a kept tie is a tie, an edge value is clear of the edge), the mirrored grid caps are the library's, and
the references agree with an independent statement on small inputs -- `struct` for the codec, a double loop for the
windows and fades, math.fsum for the sums.
"""
import ctypes
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

import boundary_cases as bc
import mastering_oracle as mo


# ---- the launch geometry is the library's ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def io_grid():
    """emu_io_grid of tests/emu/emu.cpp: the functions of csrc/io_kernels.h that mgx.hip launches with."""
    import emu_build

    lib = emu_build.load()
    lib.emu_io_grid.restype = ctypes.c_longlong
    lib.emu_io_grid.argtypes = [ctypes.c_int, ctypes.c_longlong]
    return lib.emu_io_grid


def test_mirrored_grid_caps_are_the_librarys(io_grid):
    far = 1 << 40
    assert io_grid(0, far) == bc.PCM_GRID_MAX and io_grid(1, far) == bc.PEAK_GRID_MAX
    assert io_grid(2, far) == bc.PREVIEW_CUT_GRID_MAX and io_grid(3, far) == bc.WINDOW_CHUNKS_MAX
    assert io_grid(4, 0) == bc.WINDOW_ROWS_MAX
    for samples in bc.PCM_COUNTS + bc.PEAK_COUNTS + [bc.PCM_GRID_MAX * 1024 - 1024, bc.PEAK_GRID_MAX * 1024 - 1024]:
        assert io_grid(0, samples) == bc.quad_grid(samples, bc.PCM_GRID_MAX)
        assert io_grid(1, samples) == bc.quad_grid(samples, bc.PEAK_GRID_MAX)
    for size in bc.PREVIEW_SIZES + [bc.PREVIEW_WRAP, bc.PREVIEW_CUT_GRID_MAX * 256]:
        assert io_grid(2, size) == min(-(-size // 256), bc.PREVIEW_CUT_GRID_MAX)
    for _, size, _ in bc.WINDOW_CASES + [bc.MANY_WINDOWS]:
        assert io_grid(3, size) == bc.window_chunks(size)
    assert io_grid(3, bc.WINDOW_CHUNK_FRAMES * 2 - 1) == 1 and io_grid(3, bc.WINDOW_CHUNK_FRAMES * 2) == 2


def test_no_literal_cap_is_left_in_the_launches():
    """mgx.hip launches the five kernels with the named grids."""
    import os

    from conftest import ROOT

    with open(os.path.join(ROOT, "matchering_amd", "csrc", "mgx.hip")) as fh:
        text = fh.read()
    for call, grid in (("k_pcm_decode,", "pcm_grid(samples)"), ("k_pcm_encode,", "pcm_grid(samples)"),
                       ("k_peak_count,", "peak_grid(samples)"), ("k_preview_cut,", "preview_cut_grid(size)"),
                       ("k_window_energy,", "WINDOW_ENERGY_ROWS_MAX")):
        at = text.index("hipLaunchKernelGGL(" + call)
        assert grid in text[at - 400:at], call


# ---- the wrapping lengths wrap ---------------------------------------------------------------------------------------------
def test_the_wrapping_lengths_wrap_and_every_tail_exists():
    # PCM: the grid is capped, the quads need a second trip -- 257 of them -- and three samples are left over
    grid = bc.quad_grid(bc.PCM_WRAP, bc.PCM_GRID_MAX)
    quads = bc.PCM_WRAP // 4
    assert grid == bc.PCM_GRID_MAX and bc.trips(quads, grid) == 2 and quads - grid * 256 == 257 and bc.PCM_WRAP % 4 == 3
    assert bc.trips(bc.PCM_WRAP, grid) == 5                               # (the 32-bit paths move one sample a thread)
    # peak: two whole trips, 256 quads of a third, three samples left over; index 2 * stride - 2 is in the second trip's last quad
    grid = bc.quad_grid(bc.PEAK_WRAP, bc.PEAK_GRID_MAX)
    quads = bc.PEAK_WRAP // 4
    assert grid == bc.PEAK_GRID_MAX and bc.trips(quads, grid) == 3 and quads - 2 * grid * 256 == 256 and bc.PEAK_WRAP % 4 == 3
    assert (2 * bc.PEAK_GRID_MAX * 1024 - 2) // 4 == 2 * grid * 256 - 1
    assert "last_quad_of_second_trip" in bc.peak_cases(bc.PEAK_WRAP)
    # preview cut: one frame a thread
    assert bc.trips(bc.PREVIEW_WRAP, bc.PREVIEW_CUT_GRID_MAX) == 2 and bc.PREVIEW_WRAP - bc.PREVIEW_CUT_GRID_MAX * 256 == 259
    # window energy: more windows than one launch takes, and the window on either side of the seam exists
    n, size, step = bc.MANY_WINDOWS
    assert bc.window_count(n, size, step) == 70001 > bc.WINDOW_ROWS_MAX + 1
    for counts in (bc.PCM_COUNTS, bc.PEAK_COUNTS):
        assert {c % 4 for c in counts} == {0, 1, 2, 3}
        assert {c % 4 for c in counts if c > 1000} == {0, 1, 2, 3} and {1, 2, 3} <= set(counts)
    assert max(bc.PCM_WRAP, bc.PEAK_WRAP, 2 * (bc.PREVIEW_WRAP + bc.PREVIEW_ROOM)) <= 8_400_000
    assert all(2 * n <= 8_400_000 for n, _, _ in bc.WINDOW_CASES)


def test_window_cases_cover_what_they_name():
    chunks = {bc.window_chunks(min(size, n)) for n, size, _ in bc.WINDOW_CASES}
    assert {1, 2, 3, 64} <= chunks
    assert any(size // bc.WINDOW_CHUNK_FRAMES > bc.WINDOW_CHUNKS_MAX for _, size, _ in bc.WINDOW_CASES)
    assert {1, 255, 16383, 32767, 32768, 3 * 16384 + 1, 64 * 16384 + 5} <= {size for _, size, _ in bc.WINDOW_CASES}
    steps = [(n, size, step) for n, size, step in bc.WINDOW_CASES if size < n]
    assert any(step == 1 for _, _, step in steps) and any(step & 1 and step > 1 for _, _, step in steps)
    assert any(step == size for _, size, step in steps) and any(step > size for _, size, step in steps)
    assert any((n - size) % step for n, size, step in steps)
    assert any(size == n for n, size, _ in bc.WINDOW_CASES) and any(size > n for n, size, _ in bc.WINDOW_CASES)
    # a ragged last chunk: the chunks' common length does not divide the window
    size = 3 * 16384 + 1
    assert -(-size // 3) * 3 > size


def test_tail_variants_put_every_special_on_every_tail_sample():
    specials = bc.decode_specials(24)
    for n in (1, 2, 3, 5, 1023):
        variants = bc.tail_variants(bc.integers(24, n), specials)
        assert variants[0][0] == "base" and len(variants) == 1 + len(specials)
        for back in range(1, min(3, n) + 1):
            assert {int(x[n - back]) for _, x in variants[1:]} == set(specials)
        for _, x in variants[1:]:
            assert np.array_equal(x[:max(n - 3, 0)], variants[0][1][:max(n - 3, 0)])
    specials = bc.encode_specials(16)
    seen = np.concatenate([x[-3:] for _, x in bc.tail_variants(bc.floats(16, 1027), specials, stride=3)[1:]])
    assert {v.tobytes() for v in specials} <= {v.tobytes() for v in seen}          # (bytes: -0.0 is not 0.0)


# ---- the codec ---------------------------------------------------------------------------------------------------------------
def test_every_kept_tie_is_a_tie_and_no_other_exists():
    for bits in (16, 24):
        top = (1 << (bits - 1)) - 1
        ties = bc.exact_ties(bits)
        assert ties == ((np.float32(0.5), (1 << (bits - 2)) - 1),)
        for x, k in ties:
            assert Fraction(float(x)) * top == Fraction(2 * k + 1, 2) and k & 1
            # ... and the host codec sends it to the even neighbour, either sign
            assert bc.encode_reference(np.array([x, -x]), bits).tobytes() == bc.as_pcm(np.array([k + 1, -(k + 1)]), bits).tobytes()
        # what the search finds is all there can be: a dyadic x with x top = k + 1/2 needs top | (2 k + 1) < 2 top
        assert top & 1 and (2 * ties[0][1] + 1) == top
    for bits in (16, 24, 32):
        specials = bc.encode_specials(bits)
        assert {np.float32(0.5).tobytes(), np.float32(-0.5).tobytes()} <= {v.tobytes() for v in specials}
        assert np.float32(-0.0).tobytes() in {v.tobytes() for v in specials}
        assert np.abs(specials[specials != 0]).min() < np.finfo(np.float32).tiny                # a denormal
        assert not np.isnan(specials).any()


def test_the_host_codec_sends_infinity_to_the_ends_of_the_range():
    from matchering_amd import audio_io

    for bits in (16, 24, 32):
        low, high = bc.pcm_range(bits)
        q = audio_io._quantise(np.array([np.inf, -np.inf, 3e38, -3e38], dtype=np.float32), bits)
        assert q.tolist() == [high, low, high, low]


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_codec_references_against_struct(bits):
    """as_pcm / decode_reference / encode_reference against struct.pack and Python's own arithmetic."""
    n = 41
    low, high = bc.pcm_range(bits)
    values = bc.integers(bits, n)
    assert {low, high, -1, 0, 1} <= set(values.tolist())
    pcm = bc.as_pcm(values, bits)
    if bits == 24:
        packed = b"".join(struct.pack("<i", int(v))[:3] for v in values)
    else:
        packed = struct.pack("<%d%s" % (n, "h" if bits == 16 else "i"), *[int(v) for v in values])
    assert pcm.tobytes() == packed and pcm.shape == (n, 3 if bits == 24 else 1)
    want = [np.float32(int(v) / float(1 << (bits - 1))) for v in values]        # (one rounding: the quotient is exact)
    assert bc.decode_reference(pcm).tolist() == [float(w) for w in want]
    x = bc.floats(bits, 64)
    top = high
    expect = []
    for v in x:
        if math.isinf(float(v)):
            expect.append(high if v > 0 else low)
        else:
            expect.append(int(min(max(round(Fraction(float(v)) * top), low), high)))    # round(Fraction): ties to even, exact
    if bits == 32:
        # the codec multiplies in float64: one rounding before rint, where the exact product has more than 53 bits
        expect = [int(min(max(round(float(v) * float(top)), low), high)) if math.isfinite(float(v)) else e
                  for v, e in zip(x, expect)]
    assert bc.encode_reference(x, bits).tobytes() == bc.as_pcm(np.array(expect), bits).tobytes()


# ---- peak and count ------------------------------------------------------------------------------------------------------------
def test_isclose_edge_values_straddle_the_edge_and_keep_clear_of_it():
    values, inside = bc.isclose_edge_values(0.9)
    peak = float(np.float32(0.9))
    assert values.dtype == np.float32 and 6 <= values.shape[0] <= 9 and inside.any() and not inside.all()
    for v, flag in zip(values, inside):
        exact = Fraction(peak) - Fraction(float(v))
        tol = Fraction(1e-8) + Fraction(1e-5) * Fraction(peak)
        assert (exact <= tol) == bool(flag) == bool(np.isclose(float(v), peak))
        assert abs(exact - tol) > Fraction(4 * np.finfo(np.float64).eps * peak)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 1023, 1027])
def test_peak_cases_against_the_isclose_statement(n):
    """checker.count_max_peaks -- the GPU test's reference -- against dsp.py:49-54 written with numpy.isclose."""
    from matchering_amd import checker

    for name, x in bc.peak_cases(n).items():
        assert x.dtype == np.float32 and x.shape == (n,)
        peak = np.abs(x.astype(np.float64)).max()
        count = int(np.count_nonzero(np.isclose(np.abs(x.astype(np.float64)), peak)))
        got = checker.count_max_peaks(x)
        assert (float(got[0]), got[1]) == (peak, count), name
        if name == "last_sample":
            assert np.abs(x[-1]) == peak and count == 1
        if name == "every_sample":
            assert count == n
        if name == "negative_only":
            assert x.max() <= 0
        if name == "isclose_plateau" and n >= 1023:
            assert 1 < count < 1 + 2 * bc.isclose_edge_values(0.9)[0].shape[0]


# ---- windows and fades -------------------------------------------------------------------------------------------------------
def test_window_energy_reference_against_a_double_loop():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63                    # the cumulative sum has the bits its docstring says
    for n, size, step in ((50, 7, 3), (64, 64, 5), (20, 31, 2), (33, 1, 1), (1000, 255, 7)):
        x = bc.frames(n)
        got = bc.window_energy_reference(x, size, step)
        s = min(size, n)
        want = [math.fsum(float(v) * float(v) for v in x[b:b + s].reshape(-1)) for b in range(0, n - s + 1, step)]
        assert got.shape == (len(want),) == (bc.window_count(n, size, step),)
        assert np.abs(got / np.array(want) - 1.0).max() <= 4e-16
    # ... and where the differences are of long sums: a window's sum to 1e-15 at the far end of MANY_WINDOWS
    n, size, step = bc.MANY_WINDOWS
    x = bc.frames(n)
    got = bc.window_energy_reference(x, size, step)
    for w in (0, bc.WINDOW_ROWS_MAX - 1, bc.WINDOW_ROWS_MAX, 70000):
        want = math.fsum(float(v) * float(v) for v in x[w:w + size].reshape(-1))
        assert abs(got[w] / want - 1.0) <= 1e-15


def test_cut_reference_against_a_double_loop():
    x = bc.frames(40)
    for size in (1, 2, 9, 10):
        for fade in bc.preview_fades(size):
            for limit in bc.PREVIEW_LIMITS:
                got = bc.cut_reference(x, 5, size, fade, limit)
                for i in range(size):
                    g = 1.0
                    if fade > 0:
                        up = 0.0 if fade == 1 else i / (fade - 1)
                        down = 0.0 if fade == 1 else (size - 1 - i) / (fade - 1)
                        g = (up if i < fade else 1.0) * (down if i >= size - fade else 1.0)
                    for c in range(2):
                        v = float(x[5 + i, c])
                        if limit > 0:
                            v = min(max(v, -limit), limit)
                        assert abs(got[i, c] - v * g) <= 4e-16 * abs(v), (size, fade, limit, i)
    assert bc.preview_fades(257) == [0, 1, 2, 128, 129, 257] and bc.preview_fades(1) == [0, 1]
    binding = bc.frames(bc.PREVIEW_SIZES[-1] + bc.PREVIEW_ROOM)
    assert (np.abs(binding) > 0.3).mean() > 0.3                          # the limit that binds binds
    # expected_previews, which the parity tests use, cuts with the same two functions
    result = bc.frames(900, seed=1)
    begin, target_piece, result_piece = bc.expected_previews(bc.frames(900), result, 200, 50, 30, 0.4)
    assert np.array_equal(result_piece, bc.cut_reference(result, begin, 200, 30, 0.0))
    assert np.array_equal(target_piece, bc.cut_reference(bc.frames(900), begin, 200, 30, 0.4))


def test_float32_steps_counts_representable_values():
    a = np.array([1.0, -1.0, 0.0, 1e-45, 3.0], dtype=np.float32)
    b = np.array([np.nextafter(np.float32(1), np.float32(2)), -1.0, -0.0, -1e-45, 3.0])
    assert bc.float32_steps(a, b).tolist() == [1, 0, 0, 2, 0]


# ---- sums, early-out, band exits ---------------------------------------------------------------------------------------------
def test_sumsq_reference_and_its_cases():
    mid = bc.sumsq_input(3 * 257 + 5)
    assert np.abs(mid).max() * bc.SUMSQ_GAINS[0] < 1.0                  # nothing clips at the smallest gain
    for gain in bc.SUMSQ_GAINS:
        got = bc.sumsq_reference(mid, 257, 3, gain)
        want = [math.fsum(min(max(float(v) * gain, -1.0), 1.0) ** 2 for v in mid[d * 257:(d + 1) * 257]) for d in range(3)]
        assert np.abs(got / np.array(want) - 1.0).max() <= 4e-16
    assert got.min() > 0.9 * 257                                         # at 50 the sum approaches the count
    assert bc.clipped_chunks(bc.SUMSQ_ONE_CHUNK) == 1 and bc.clipped_chunks(bc.SUMSQ_ONE_CHUNK - 1) == 2
    assert bc.clipped_chunks(1) == 1024 and bc.clipped_chunks(3) == 683
    for piece in bc.SUMSQ_PIECES:
        divisions = bc.sumsq_divisions(piece)
        assert divisions[:2] == [1, 3] and (bc.SUMSQ_ONE_CHUNK in divisions) == (piece <= 4097)


def test_early_out_peaks_are_the_sixteen_nearest_and_clear_of_the_edge():
    threshold = mo.params().threshold
    peaks = bc.early_out_peaks(threshold)
    edge = Fraction(threshold) * (1 + Fraction(1e-5) + Fraction(1e-8))
    assert peaks.shape == (16,) and np.all(np.diff(peaks.view(np.int32)) == 1)
    assert all(Fraction(float(p)) < edge for p in peaks[:8]) and all(Fraction(float(p)) > edge for p in peaks[8:])
    flags = [bc.limiter_is_active(p, threshold) for p in peaks]
    assert flags == [False] * 8 + [True] * 8
    for p in peaks:                                                      # no value within a float64 rounding of the edge
        assert abs(abs(float(p) / threshold - 1.0) - (1e-8 + 1e-5)) > 1e-12
        assert np.float32(2) * p * np.float32(0.5) == p                  # doubled and halved: the same float32
    # the oracle takes the same decision on a track with that peak
    for place in ("left", "right_negative", "last_frame"):
        for p, flag in zip(peaks[6:10], flags[6:10]):
            x = bc.early_out_track(place, p)
            assert np.abs(x).max() == p and np.sort(np.abs(x).reshape(-1))[-2] <= 0.5
            assert (mo.limiter_envelopes(x.astype(np.float64), mo.params()) is not None) == flag
    n, at, _, _ = bc.EARLY_OUT_PLACES["block_300"]
    assert at // 4096 == 300 == (n - 1) // 4096 and n % 4096 == 17


@pytest.mark.parametrize("name", sorted(bc.BAND_EXITS))
def test_band_exit_stimuli_leave_the_band_where_they_say(name):
    target, reference = bc.band_exit_pair(name)
    trace = {}
    mo.master(target, reference, mo.params(**bc.band_exit_config(name)), False, True, False, trace=trace)
    running = bc.check_band_routes(name, trace["correction_coefficients"])
    routes = bc.BAND_EXITS[name][2]
    assert running.shape[0] == bc.BAND_EXITS[name][1]
    if name.startswith("up_midway"):
        assert routes[:3] == ["band", "band", "stream"] and running[2] > bc.BAND_G_HI > running[1]
    else:
        assert set(routes) == {"stream"}
