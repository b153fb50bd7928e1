"""The small kernels around the master chain on the GPU at their ragged ends, grid wraps and edges, each against a plain
reference of the same operation (tests/boundary_cases.py holds the inputs and references; tests/test_boundary_cases_host.py
checks those on the CPU and holds the mirrored grid caps to csrc/io_kernels.h).

Kernels reached: k_pcm_decode and k_pcm_encode at 16, 24 and 32 bits with 0 .. 3 samples behind the last quad and a second
trip of the capped grid; k_peak_max / k_peak_count the same, three trips; k_window_energy at every chunk count from 1 to
the cap of 64 and in two launches; k_preview_cut with ramps that meet, a one-frame ramp and a second trip; k_clipped_sumsq
from 1024 workgroups a piece down to one; k_frame_peaks with the peak in the ragged last block, and k_finalize_scalars
over more than 256 blocks, at the limiter's early-out edge.

Measured on an MI355X (largest over the cases of a group):

  PCM decode and encode, peak and count, the early-out decision, the passed-through output: exact (3 x 15 sample counts
  each way, 15 for the peak, 4 x 2 x 16 peaks at the edge).
  window energy, relative to the extended-precision sum (bound 1e-12): 2.7e-15 over 70 001 windows of 16 frames,
  1.3e-15 at 64 chunks, at most 8.9e-16 in the other cases.
  clipped sums, relative (bound 1e-12): 1.4e-15 over the 156 combinations of piece, divisions, length and gain.
  preview cut, float32 steps from float32(reference) (bound 1): 0 in all but the cuts of 255 frames, where 12 samples of
  54 cuts are one step off; 0 over the five cuts of 1 048 835 frames.
  limiter output just above the edge against the oracle: largest error 2.9e-8, RMS 6.0e-9 (bounds 5e-6 and 1e-6).
"""
import ctypes

import numpy as np
import pytest

import boundary_cases as bc
import mastering_oracle as mo
import stage_sweeps as sw

pytestmark = pytest.mark.gpu

LEAD = 16                                       # sentinel bytes in front of an output: the kernels want 16-byte alignment


def native():
    from matchering_amd._native import check, library
    from matchering_amd.device import default_device

    return default_device(), library(), check


def guarded(call, source, out_bytes):
    """`call(device address of source, device address of the output)` with LEAD sentinel bytes in front of the output's
    out_bytes and LEAD behind them, both buffers at the alignment the allocator gives.  Returns (front sentinels, output
    bytes, rear sentinels) as uint8."""
    dev, _, _ = native()
    whole = np.full(LEAD + out_bytes + LEAD, bc.SENTINEL_BYTE, dtype=np.uint8)
    with dev.lock:
        src, out = dev.upload(source, dtype=None), dev.upload(whole, dtype=None)
        try:
            assert src.ptr % 16 == 0 and out.ptr % 16 == 0
            call(ctypes.c_void_p(src.ptr), ctypes.c_void_p(out.ptr + LEAD))
            got = np.array(dev.download(out, whole.shape, np.uint8))
        finally:
            src.release()
            out.release()
    return got[:LEAD], got[LEAD:LEAD + out_bytes], got[LEAD + out_bytes:]


def untouched(front, rear):
    return bool(np.all(front == bc.SENTINEL_BYTE) and np.all(rear == bc.SENTINEL_BYTE))


# ---- 1. PCM decode and encode, bit for bit -----------------------------------------------------------------------------
def decode(pcm, samples, bits):
    dev, lib, check = native()
    front, body, rear = guarded(lambda src, out: check(lib.mgx_pcm_decode(dev.handle, src, samples, bits, out)),
                                pcm, samples * 4)
    assert untouched(front, rear), (samples, bits)
    return body.view(np.float32)


def encode(x, bits):
    dev, lib, check = native()
    front, body, rear = guarded(lambda src, out: check(lib.mgx_pcm_encode(dev.handle, src, x.shape[0], bits, out)),
                                x, x.shape[0] * bits // 8)
    assert untouched(front, rear), (x.shape[0], bits)
    return body


def patched(reference_of_base, tail_reference, samples):
    """An element-wise reference of a variant that differs from its base in the last (up to) three samples only."""
    tail = min(3, samples)
    out = reference_of_base.copy()
    out[samples - tail:] = tail_reference
    return out


@pytest.mark.parametrize("bits", [16, 24, 32])
@pytest.mark.parametrize("samples", bc.PCM_COUNTS)
def test_pcm_decode_every_tail_and_the_second_trip(samples, bits):
    """mgx_pcm_decode of one-dimensional sample counts against audio_io.pcm_to_float, bit for bit: random samples, the ends
    of the range, -1, 0 and 1, each of them on each of the last three samples; the floats in front of and behind the
    output keep their bytes."""
    wraps = samples == bc.PCM_WRAP
    if wraps:
        assert samples // 4 > bc.PCM_GRID_MAX * 256 == bc.quad_grid(samples, bc.PCM_GRID_MAX) * 256 and samples % 4 == 3
    base = bc.integers(bits, samples)
    base_want = bc.decode_reference(bc.as_pcm(base, bits))
    for name, values in bc.tail_variants(base, bc.decode_specials(bits)):
        pcm = bc.as_pcm(values, bits)
        tail = min(3, samples)
        want = patched(base_want, bc.decode_reference(bc.as_pcm(values[samples - tail:], bits)), samples)
        if not wraps:
            assert np.array_equal(want, bc.decode_reference(pcm))
        got = decode(pcm, samples, bits)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (samples, bits, name)


@pytest.mark.parametrize("bits", [16, 24, 32])
@pytest.mark.parametrize("samples", bc.PCM_COUNTS)
def test_pcm_encode_every_tail_and_the_second_trip(samples, bits):
    """mgx_pcm_encode against audio_io._quantise (and _pack24), byte for byte: random floats, full scale and its float32
    neighbours, far beyond it, either zero, a denormal, infinity, near ties and the exact ties, at both signs, each of them
    in the ragged tail; and decode(encode(x)) is the host codec's round trip."""
    wraps = samples == bc.PCM_WRAP
    specials = bc.encode_specials(bits)
    base = bc.floats(bits, samples)
    base_want = bc.encode_reference(base, bits)
    width = base_want.shape[1]
    for name, x in bc.tail_variants(base, specials, stride=3 if wraps else 1):
        tail = min(3, samples)
        want = patched(base_want, bc.encode_reference(x[samples - tail:], bits), samples)
        if not wraps:
            assert np.array_equal(want, bc.encode_reference(x, bits))
        got = encode(x, bits)
        assert got.tobytes() == want.tobytes(), (samples, bits, name)
        if name in ("base", "tail0"):
            back = decode(got.view(want.dtype).reshape(samples, width), samples, bits)
            assert np.array_equal(back.view(np.uint32), bc.decode_reference(want).view(np.uint32)), (samples, bits, name)


def test_upload_frames_and_download_pcm_of_one_odd_channel():
    """The way production reaches the tails: Device.upload_frames / download_pcm of a mono track with an odd frame count."""
    dev, _, _ = native()
    for bits in (16, 24, 32):
        for frames in (1, 3, 1025):
            pcm = bc.as_pcm(bc.integers(bits, frames, seed=1), bits)
            with dev.lock:
                buf = dev.upload_frames(pcm)
                floats = np.array(dev.download(buf, (frames,)))
                again = np.array(dev.download_pcm(buf, frames, 1, bits))
                buf.release()
            assert np.array_equal(floats, bc.decode_reference(pcm)), (bits, frames)
            assert again.dtype == pcm.dtype and again.tobytes() == bc.encode_reference(floats, bits).tobytes()


# ---- 2. peak and count ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", bc.PEAK_COUNTS)
def test_peak_count_every_tail_and_the_third_trip(samples):
    """mgx_peak_count against checker.count_max_peaks, exact peak and exact count: the peak alone in the ragged tail, alone
    in the last quad of the second trip, negative only, on every sample, all zeros, and a plateau on both sides of
    numpy.isclose's edge."""
    from matchering_amd import checker

    dev, _, _ = native()
    if samples == bc.PEAK_WRAP:
        assert samples // 4 > 2 * bc.PEAK_GRID_MAX * 256 and bc.quad_grid(samples, bc.PEAK_GRID_MAX) == bc.PEAK_GRID_MAX
    for name, x in bc.peak_cases(samples).items():
        with dev.lock:
            buf = dev.upload(x)
            got = dev.peak_count(buf, samples)
            buf.release()
        want = checker.count_max_peaks(x)
        assert got == (float(want[0]), want[1]), (samples, name, got, want)


# ---- 3. window energy -----------------------------------------------------------------------------------------------------
def window_energy(x, size, step, capacity=None):
    """mgx_window_energy as the C API has it (Device.window_energy clamps the size itself): (rc, energies, count)."""
    dev, lib, _ = native()
    n = x.shape[0]
    capacity = bc.window_count(n, size, step) if capacity is None else capacity
    energy = np.full(max(capacity, 1), -1.0)
    count = ctypes.c_int64(-1)
    with dev.lock:
        buf = dev.upload(x)
        try:
            rc = lib.mgx_window_energy(dev.handle, ctypes.c_void_p(buf.ptr), n, size, step,
                                       energy.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), capacity, ctypes.byref(count))
        finally:
            buf.release()
    return rc, energy[:capacity], count.value


def check_windows(x, size, step, key):
    want = bc.window_energy_reference(x, size, step)
    rc, got, count = window_energy(x, size, step)
    assert rc == 0 and count == want.shape[0], key
    worst = float(np.abs(got / want - 1.0).max())
    print(f"BOUNDARY window_energy {key} windows={count} chunks={bc.window_chunks(min(size, x.shape[0]))} worst={worst:.3e}")
    assert worst <= 1e-12, (key, worst)
    assert int(np.argmax(got)) == int(np.argmax(want)), key
    return got, want


@pytest.mark.parametrize("n,size,step", bc.WINDOW_CASES)
def test_window_energy_every_chunk_count_and_step(n, size, step):
    """mgx_window_energy against a cumulative sum in extended precision: 1e-12 relative (test_clipped_piece_sumsq's bound
    for the same kind of sum), and numpy's argmax."""
    check_windows(bc.frames(n), size, step, f"n={n} size={size} step={step}")


def test_window_energy_of_more_windows_than_one_launch_takes():
    n, size, step = bc.MANY_WINDOWS
    x = bc.frames(n)
    x[bc.WINDOW_ROWS_MAX + size + 4] = (3.0, -3.0)                      # every window that holds it starts in the second launch
    got, want = check_windows(x, size, step, "many windows")
    assert got.shape[0] == 70001 > bc.WINDOW_ROWS_MAX
    seam = slice(bc.WINDOW_ROWS_MAX - 2, bc.WINDOW_ROWS_MAX + 2)       # the last windows of the first launch, the first of the second
    assert np.abs(got[seam] / want[seam] - 1.0).max() <= 1e-12 and len(set(want[seam])) == 4
    assert int(np.argmax(got)) >= bc.WINDOW_ROWS_MAX


def test_window_energy_refuses_a_short_array_and_works_afterwards():
    x = bc.frames(1000)
    rc, energy, count = window_energy(x, 255, 7, capacity=50)
    assert rc == -1 and count == bc.window_count(1000, 255, 7) == 107           # MGX_ERR_ARGUMENT, *count set
    assert np.all(energy == -1.0)
    for bad in (dict(size=0, step=1), dict(size=5, step=0)):
        assert window_energy(x, bad["size"], bad["step"], capacity=4)[0] == -1
    check_windows(x, 255, 7, "after a refusal")


# ---- 4. preview cut -------------------------------------------------------------------------------------------------------
def preview_cut(x, begin, size, fade, limit):
    dev, lib, check = native()
    n = x.shape[0]
    front, body, rear = guarded(
        lambda src, out: check(lib.mgx_preview_cut(dev.handle, src, n, begin, size, fade, float(limit), out)), x, size * 8)
    assert untouched(front, rear), (size, begin, fade, limit)
    return body.view(np.float32).reshape(size, 2)


def check_cut(x, begin, size, fade, limit):
    """The kernel forms gain * clipped sample in float64 and rounds once to float32.  The reference's numpy.linspace value
    may differ from the kernel's i / (fade - 1) by one float64 rounding, and where the ramps overlap the reference
    multiplies the sample by one factor after the other, the kernel by their product: a relative 4e-16 at most, which
    moves a float32 rounding only where the float64 value lies that close to the middle of two float32 values.  So every
    output is float32(reference) or a float32 neighbour of it -- at most one step."""
    got = preview_cut(x, begin, size, fade, limit)
    steps = bc.float32_steps(got, bc.cut_reference(x, begin, size, fade, limit))
    worst = int(steps.max())
    assert worst <= 1, (size, begin, fade, limit, worst)
    return worst, int(np.count_nonzero(steps))


@pytest.mark.parametrize("size", bc.PREVIEW_SIZES)
def test_preview_cut_every_fade_begin_and_limit(size):
    x = bc.frames(size + bc.PREVIEW_ROOM)
    worst = off = 0
    for begin, fade, limit in bc.preview_cases(size):
        w, c = check_cut(x, begin, size, fade, limit)
        worst, off = max(worst, w), off + c
    print(f"BOUNDARY preview_cut size={size} cases={len(bc.preview_cases(size))} worst_steps={worst} samples_one_step_off={off}")
    # a ramp of one frame silences the first and the last frame (numpy.linspace(0, 1, 1) == [0]) and nothing else
    got = preview_cut(x, 13, size, 1, 0.0)
    assert not got[0].any() and not got[-1].any()
    assert np.array_equal(got[1:-1], x[14:13 + size - 1])


def test_preview_cut_second_trip_of_the_grid():
    size = bc.PREVIEW_WRAP
    assert size > bc.PREVIEW_CUT_GRID_MAX * 256
    x = bc.frames(size + bc.PREVIEW_ROOM)
    worst = off = 0
    for begin, fade, limit in bc.PREVIEW_WRAP_CASES:
        w, c = check_cut(x, begin, size, fade, limit)
        worst, off = max(worst, w), off + c
    print(f"BOUNDARY preview_cut size={size} cases={len(bc.PREVIEW_WRAP_CASES)} worst_steps={worst} samples_one_step_off={off}")


def test_preview_cut_refusals():
    dev, lib, _ = native()
    with dev.lock:
        src, out = dev.upload(bc.frames(100)), dev.alloc(100 * 8)
        try:
            for begin, size, fade in ((-1, 10, 0), (0, 0, 0), (91, 10, 0), (0, 10, 11), (0, 10, -1)):
                rc = lib.mgx_preview_cut(dev.handle, ctypes.c_void_p(src.ptr), 100, begin, size, fade, 0.0,
                                         ctypes.c_void_p(out.ptr))
                assert rc == -1, (begin, size, fade)                             # MGX_ERR_ARGUMENT
            assert lib.mgx_preview_cut(dev.handle, ctypes.c_void_p(src.ptr), 100, 90, 10, 10, 0.0, ctypes.c_void_p(out.ptr)) == 0
            dev.synchronize()
        finally:
            src.release()
            out.release()


# ---- 5. clipped sums of squares ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("piece", bc.SUMSQ_PIECES)
def test_clipped_piece_sumsq_every_piece_and_chunk_count(piece):
    """mgx_clipped_piece_sumsq against numpy in extended precision, 1e-12 relative: 1024, 683 and one workgroup a piece,
    the array exactly the pieces and longer (the frames behind them are ignored), a gain at which nothing clips, one at
    which some samples do and one at which nearly all do."""
    dev, lib, check = native()
    for divisions in bc.sumsq_divisions(piece):
        for extra in (0, 5):
            mid = bc.sumsq_input(piece * divisions + extra)
            if extra:
                mid[piece * divisions:] = 1e3                                    # what is ignored would be seen
            with dev.lock:
                buf = dev.upload(mid)
                try:
                    for gain in bc.SUMSQ_GAINS:
                        got = np.zeros(divisions)
                        check(lib.mgx_clipped_piece_sumsq(dev.handle, ctypes.c_void_p(buf.ptr), mid.shape[0], piece, divisions,
                                                          gain, got.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
                        want = bc.sumsq_reference(mid, piece, divisions, gain)
                        worst = float(np.abs(got / want - 1.0).max())
                        print(f"BOUNDARY clipped_sumsq piece={piece} divisions={divisions} chunks={bc.clipped_chunks(divisions)} "
                              f"gain={gain} worst={worst:.3e}")
                        assert worst <= 1e-12, (piece, divisions, extra, gain, worst)
                finally:
                    buf.release()


def test_clipped_piece_sumsq_refuses_pieces_beyond_the_array():
    from matchering_amd import kernels
    from matchering_amd._native import MgxError

    mid = bc.sumsq_input(3 * 257)
    with pytest.raises(MgxError) as refusal:
        kernels.clipped_piece_sumsq(mid[:-1], 257, 3, gain=1.3)
    assert refusal.value.code == -1                                              # MGX_ERR_ARGUMENT
    assert np.abs(kernels.clipped_piece_sumsq(mid, 257, 3, gain=1.3) / bc.sumsq_reference(mid, 257, 3, 1.3) - 1).max() <= 1e-12


# ---- 6. the limiter's early-out ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", sorted(bc.EARLY_OUT_PLACES))
def test_limiter_early_out_at_its_edge(place):
    """kernels.limit on a track whose one loud sample takes the sixteen float32 values around threshold * (1 + 1e-5 + 1e-8):
    `active` is the float64 statement of hyrax.py:83-85 on float32(peak * gain), at gain 1 and at gain 0.5 with the sample
    doubled.  The output: stage_sweeps.check_limiter against the oracle where the limiter runs; where it does not, the
    input times the gain, exactly.  The long track (the peak in block 300, past k_finalize_scalars' 256 threads) takes
    all sixteen values for the decision and the two nearest the edge for the output."""
    import matchering_amd as mg
    from matchering_amd import kernels

    cfg, ocfg = mg.Config(), mo.params()
    peaks = bc.early_out_peaks(ocfg.threshold)
    long_track = bc.EARLY_OUT_PLACES[place][0] > 100000
    for gain in (1.0, 0.5):
        for i, peak in enumerate(peaks):
            want_active = bc.limiter_is_active(peak, ocfg.threshold)
            assert want_active == (i >= 8)
            after_gain = bc.early_out_track(place, peak)
            x = after_gain if gain == 1.0 else after_gain * np.float32(2.0)
            assert x.dtype == np.float32 and np.array_equal(x * np.float32(gain), after_gain)
            out, active = kernels.limit(x, cfg, gain=gain)
            assert active == want_active, (place, gain, i, float(peak))
            if long_track and i not in (7, 8):
                continue
            if want_active:
                sw.check_limiter(out, active, after_gain, ocfg, False, f"early-out {place} gain={gain} peak#{i}")
            else:
                assert np.array_equal(out, after_gain), (place, gain, i)
