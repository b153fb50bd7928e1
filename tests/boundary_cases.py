"""Inputs and plain references for the tails, grid wraps and band exits of the small kernels around the master chain.

Shared by tests/test_boundary_cases_host.py (the generators hold their own conditions, the references agree with an
independent statement) and tests/test_gpu_boundary_kernels.py / tests/test_gpu_band_exits.py (the kernels).  numpy only:
no tests here and nothing that needs a GPU.

A reference is the project's own host statement of the operation (audio_io._quantise, _pack24, pcm_to_float,
checker.count_max_peaks), the float64 restatement of dsp.py / preview_creator.py that the parity tests use
(expected_previews, here since it has two users), or a numpy sum in extended precision.  Never the library under test.
"""
import functools

import numpy as np

# ---- launch geometry (csrc/io_kernels.h; tests/test_boundary_cases_host.py holds these to the library's own functions) ----
PCM_GRID_MAX = 8192                 # workgroups of k_pcm_decode / k_pcm_encode, four samples a thread
PEAK_GRID_MAX = 4096                # ... of k_peak_max / k_peak_count, four samples a thread
PREVIEW_CUT_GRID_MAX = 4096         # ... of k_preview_cut, one frame a thread
WINDOW_ROWS_MAX = 65535             # windows of one k_window_energy launch
WINDOW_CHUNK_FRAMES, WINDOW_CHUNKS_MAX = 16384, 64         # workgroups of a window: size // 16384, 1 .. 64
THREADS = 256

SMALL_COUNTS = list(range(1, 8)) + list(range(1021, 1028))
PCM_WRAP = PCM_GRID_MAX * 1024 + 1031            # a second trip of the grid for 257 whole quads and a tail of three
PCM_COUNTS = SMALL_COUNTS + [PCM_WRAP]
PEAK_WRAP = PEAK_GRID_MAX * 1024 * 2 + 1027      # two whole trips, a third for 256 quads and a tail of three
PEAK_COUNTS = SMALL_COUNTS + [PEAK_WRAP]
PREVIEW_WRAP = PREVIEW_CUT_GRID_MAX * THREADS + 259

SENTINEL_BYTE = 0xA5                             # what stands in front of and behind an output buffer


def quad_grid(samples, cap):
    """mgx.hip's grid for a kernel that moves four samples a thread: one workgroup more than the whole quads need."""
    return min((samples // 4 + THREADS - 1) // THREADS + 1, cap)


def trips(items, grid):
    """How often a grid-stride loop of `grid` workgroups, one item a thread, goes round for `items` items."""
    return -(-items // (grid * THREADS))


def window_chunks(size):
    return max(1, min(WINDOW_CHUNKS_MAX, size // WINDOW_CHUNK_FRAMES))


# =====================================================================================================================
# 1. PCM at the file boundary
# =====================================================================================================================
def pcm_range(bits):
    return -(1 << (bits - 1)), (1 << (bits - 1)) - 1


def decode_specials(bits):
    low, high = pcm_range(bits)
    return [low, high, -1, 0, 1]


def integers(bits, n, seed=0):
    """n random samples of the width over its whole range (int64), the special values on the first samples that exist."""
    low, high = pcm_range(bits)
    x = np.random.RandomState(1000 * bits + seed + n % 9973).randint(low, high + 1, size=n, dtype=np.int64)
    special = decode_specials(bits)
    x[:len(special)] = special[:n]
    return x


def as_pcm(values, bits):
    """int64 sample values -> what a file of the width holds and Device.upload_frames takes, one channel: int16 (n, 1),
    int32 (n, 1), or packed little-endian uint8 (n, 3)."""
    from matchering_amd import audio_io

    values = np.asarray(values)
    if bits == 24:
        return audio_io._pack24(values.astype(np.int32))
    return values.astype(np.int16 if bits == 16 else np.int32).reshape(-1, 1)


def decode_reference(pcm):
    """The host codec's floats of PCM samples (audio_io.pcm_to_float), one-dimensional."""
    from matchering_amd import audio_io

    return audio_io.pcm_to_float(pcm, np.float32).reshape(-1)


def encode_reference(x, bits):
    """The host codec's PCM of float32 samples (audio_io._quantise, _pack24), shaped as as_pcm shapes it."""
    from matchering_amd import audio_io

    return as_pcm(audio_io._quantise(np.asarray(x, dtype=np.float32), bits), bits)


def tail_variants(base, specials, stride=1):
    """`base` itself, then copies whose last (up to) three samples are specials[r], specials[r + 1], specials[r + 2]
    (cyclically) for r = 0, stride, 2 stride ...: with stride 1 every special value stands once on each of the last
    three samples, with stride 3 once somewhere in them."""
    out = [("base", base)]
    tail = min(3, base.shape[0])
    for r in range(0, len(specials), stride):
        x = base.copy()
        x[base.shape[0] - tail:] = [specials[(r + j) % len(specials)] for j in range(tail)]
        out.append((f"tail{r}", x))
    return out


@functools.lru_cache(maxsize=None)
def exact_ties(bits):
    """Every float32 x in (0, 1) whose product with top = 2**(bits - 1) - 1 is k + 0.5 for an integer k, as (x, k) pairs,
    found by trying every k: the candidate float32((k + 0.5) / top) is kept where its float64 product with top -- which
    is exact, 24 + (bits - 1) significant bits at most -- is k + 0.5 again.  (2 k + 1) / (2 top) is a float32 only where
    top divides 2 k + 1, so the search finds x = 0.5 alone, with k = 2**(bits - 2) - 1, an odd k: the codec's tie goes
    up to the even k + 1 for +0.5 and down to -(k + 1) for -0.5.  There is no tie with an even k in either width."""
    top = float((1 << (bits - 1)) - 1)
    found = []
    for first in range(0, int(top), 1 << 20):
        k = np.arange(first, min(first + (1 << 20), int(top)), dtype=np.float64)
        x = ((k + 0.5) / top).astype(np.float32)
        hit = x.astype(np.float64) * top == k + 0.5
        found += [(np.float32(a), int(b)) for a, b in zip(x[hit], k[hit])]
    return tuple(found)


def encode_specials(bits):
    """float32 values at which a quantiser goes wrong, each at both signs: full scale, one float32 step either side of
    it, far beyond it, zero with either sign, the smallest denormal, the float32 values nearest half a step and a step
    and a half (near ties, not exact ones), infinity (audio_io._quantise sends it to the ends of the range; the CPU suite
    checks that), and every exact rounding tie of the 16 and 24-bit widths."""
    one = np.float32(1.0)
    top = float((1 << (bits - 1)) - 1)
    values = [one, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)), np.float32(1.7), np.float32(3e9),
              np.float32(3e38), np.float32(0.0), np.float32(1e-45), np.float32(0.5 / top), np.float32(1.5 / top),
              np.float32(np.inf)]
    for width in (16, 24):
        values += [x for x, _ in exact_ties(width)]
    out = []
    for v in values:
        out += [v, -v]
    return np.array(out, dtype=np.float32)


def floats(bits, n, seed=0):
    """n random float32 samples, a few beyond full scale, the special values on the first samples that exist."""
    rng = np.random.RandomState(2000 * bits + seed + n % 9973)
    x = (0.5 * rng.randn(n)).astype(np.float32)
    special = encode_specials(bits)
    x[:special.shape[0]] = special[:n]
    return x


# =====================================================================================================================
# 2. peak and count
# =====================================================================================================================
def isclose_edge_values(peak, steps=4):
    """float32 values around peak * (1 - 1e-5) - 1e-8, where numpy.isclose(x, peak) changes its answer: the float32
    neighbours of the edge and `steps` more either way, without those for which peak - x and the tolerance
    1e-8 + 1e-5 peak differ by less than a few float64 roundings (there the float64 statement depends on how it is
    written: |x - peak| <= tol here, x >= peak - tol in checker.count_max_peaks).  Returns (values, inside flags)."""
    peak = np.float32(peak)
    tol = 1e-8 + 1e-5 * float(peak)
    v = np.float32(float(peak) - tol)
    values = [v]
    lo = hi = v
    for _ in range(steps):
        lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(2) * peak)
        values += [lo, hi]
    values = np.array(sorted(values), dtype=np.float32)
    gap = float(peak) - values.astype(np.float64)               # exact: two float32 values a few steps apart
    keep = np.abs(gap - tol) > 4 * np.finfo(np.float64).eps * float(peak)         # (peak - tol is rounded at the peak's scale)
    return values[keep], (gap <= tol)[keep]


def peak_cases(n):
    """name -> float32 samples of length n for mgx_peak_count."""
    rng = np.random.RandomState(3000 + n % 9973)
    quiet = (0.25 * rng.uniform(-1.0, 1.0, n)).astype(np.float32)
    cases = {"zeros": np.zeros(n, dtype=np.float32)}
    x = quiet.copy()
    x[n - 1] = 0.75
    cases["last_sample"] = x                                   # alone in the ragged tail (or the last quad)
    if n >= 3:
        x = quiet.copy()
        x[n - 3] = -0.75
        cases["third_from_last_negative"] = x
    x = -np.abs(quiet)
    x[n // 2] = -0.8125
    cases["negative_only"] = x
    cases["every_sample"] = np.where(np.arange(n) & 1, np.float32(-0.625), np.float32(0.625)).astype(np.float32)
    stride = PEAK_GRID_MAX * 1024
    if n > 2 * stride:                                          # alone in the last quad of the second trip
        x = quiet.copy()
        x[2 * stride - 2] = -0.75
        cases["last_quad_of_second_trip"] = x
    # a plateau on both sides of numpy.isclose's edge below the peak, either sign, the peak itself in the tail
    values, _ = isclose_edge_values(0.9)
    x = quiet.copy()
    m = min(values.shape[0], max(n - 1, 0))
    x[:m] = values[:m] * np.where(np.arange(m) & 1, -1, 1)
    if n >= 2 * m + 3:                                          # ... and again, signs swapped, in front of the tail
        x[n - 2 - m:n - 2] = -x[:m]
    x[n - 1] = 0.9
    cases["isclose_plateau"] = x.astype(np.float32)
    return cases


# =====================================================================================================================
# 3. window energy (dsp.py:128-143)
# =====================================================================================================================
def frames(n, seed=0, scale=0.5):
    return (scale * np.random.RandomState(4000 + seed + n % 9973).randn(n, 2)).astype(np.float32)


# (n, size, step): every size at which the chunk count steps, every kind of step, the edge geometries
WINDOW_CASES = [
    (300, 1, 1),
    (600, 255, 1),
    (1000, 255, 7),                                        # an odd step, (n - size) % step = 3
    (1020, 255, 255),                                      # a step equal to the size
    (1500, 255, 400),                                      # a step larger than the size, (n - size) % step = 45
    (3 * 16383 + 11, 16383, 8191),                         # the longest window of one chunk
    (32767 + 1000, 32767, 333),                            # ... still one: 32767 // 16384 = 1
    (2 * 32768 + 77, 32768, 10001),                        # two chunks
    (3 * 16384 + 1 + 5000, 3 * 16384 + 1, 1667),           # three chunks of 16385, the last one ragged
    (64 * 16384 + 5 + 120001, 64 * 16384 + 5, 40000),      # 64 chunks, the most
    (70 * 16384 + 3 + 50001, 70 * 16384 + 3, 25000),       # size // 16384 = 70: capped at 64
    (777, 777, 5),                                         # size == n: one window
    (500, 900, 3),                                         # size > n: one window over the whole array
]
MANY_WINDOWS = (70016, 16, 1)                              # 70 001 windows: two launches


def window_count(n, size, step):
    size = min(size, n)
    return (n - size) // step + 1


def window_energy_reference(x, size, step):
    """Sum of squares of both channels of every window, by differences of a cumulative sum in numpy's extended precision
    (64 significant bits where the platform has them: a difference of two sums thousands of windows long then still
    holds a window's sum to 1e-15), rounded to float64."""
    n = x.shape[0]
    size = min(size, n)
    sq = (x.astype(np.float64) ** 2).sum(axis=1, dtype=np.longdouble)          # (a float32's square is exact in float64)
    total = np.concatenate([np.zeros(1, dtype=np.longdouble), np.cumsum(sq, dtype=np.longdouble)])
    starts = np.arange(window_count(n, size, step)) * step
    return (total[starts + size] - total[starts]).astype(np.float64)


# =====================================================================================================================
# 4. preview cut (preview_creator.py:30-94, dsp.py:109-110 and 146-152)
# =====================================================================================================================
def fade(piece, size):
    """dsp.py:146-152 on a float64 piece, in place: numpy.linspace(0, 1, size) over the first `size` frames, its mirror
    over the last `size`; where the two overlap both factors apply."""
    ramp = np.linspace(0, 1, size)
    piece[:size] *= ramp[:, None]
    piece[piece.shape[0] - size:] *= ramp[::-1, None]
    return piece


def cut_reference(x, begin, size, fade_size, limit):
    """Frames [begin, begin + size) of x, clipped to +-limit where limit > 0, faded: float64."""
    x = np.asarray(x, dtype=np.float64)
    if limit > 0:
        x = np.clip(x, -limit, limit)
    return fade(x[begin:begin + size].copy(), fade_size)


def expected_previews(target, result, size, step, fade_size, threshold):
    """preview_creator.py:30-94 + dsp.py:128-152 restated on host arrays (float64): (first frame of the loudest window
    of the result, the clipped target's piece, the result's piece)."""
    result = np.asarray(result, dtype=np.float64)
    n = result.shape[0]
    if size > n:
        starts, size = np.array([0]), n
    else:
        starts = np.arange((n - size) // step + 1) * step
    rms = [np.sqrt(np.mean(result[s:s + size] ** 2)) for s in starts]
    begin = int(starts[int(np.argmax(rms))])
    pieces = []
    for x in (np.clip(np.asarray(target, dtype=np.float64), -threshold, threshold), result):
        piece = x[begin:begin + size].copy()
        if size != n:
            fade(piece, fade_size)
        pieces.append(piece)
    return begin, pieces[0], pieces[1]


PREVIEW_SIZES = [1, 2, 255, 256, 257]
PREVIEW_ROOM = 37                                          # frames of the input beyond the cut: begin = n - size = 37
PREVIEW_LIMITS = [0.0, -1.0, 0.3]                          # none, none, one that binds (the input's deviation is 0.5)


def preview_fades(size):
    return sorted({f for f in (0, 1, 2, size // 2, size // 2 + 1, size) if f <= size})


def preview_cases(size):
    """(begin, fade, limit) for a cut of `size` frames out of size + PREVIEW_ROOM."""
    return [(b, f, lim) for b in (0, 13, PREVIEW_ROOM) for f in preview_fades(size) for lim in PREVIEW_LIMITS]


# the second trip of the grid depends on the size alone: every begin, every limit and the fades whose ramps meet, end
# in their middle or are absent, once each
PREVIEW_WRAP_CASES = [(0, PREVIEW_WRAP // 2 + 1, 0.3), (13, PREVIEW_WRAP, 0.0), (PREVIEW_ROOM, 1, -1.0), (13, 0, 0.3),
                      (PREVIEW_ROOM, PREVIEW_WRAP // 2, 0.0)]


def float32_steps(got, want64):
    """How many float32 values lie between each got and float32(want64) (0: the same value)."""
    def ordinal(a):
        bits = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(bits < 0, -(bits & 0x7FFFFFFF), bits)

    return np.abs(ordinal(got) - ordinal(np.asarray(want64).astype(np.float32)))


# =====================================================================================================================
# 5. clipped sums of squares per piece (stages.py:149-160)
# =====================================================================================================================
SUMSQ_PIECES = [1, 255, 256, 257, 1023, 1024, 1025, 4097, 9001]
SUMSQ_ONE_CHUNK = 2048                                     # run_conv.h clipped_chunks: (2048 + d - 1) // d == 1 from here
SUMSQ_GAINS = [0.3, 1.3, 50.0]                             # the input stays below 1 / 0.3: nothing clips at 0.3
SUMSQ_MAX_SAMPLES = 8_400_000                             # 4097 x 2048 still fits; no input of these tests is longer


def clipped_chunks(divisions):
    return max(1, min(1024, (2048 + divisions - 1) // divisions))


def sumsq_divisions(piece):
    """1, 3 and the first count at which a piece is one workgroup's, where the array that needs stays within bounds."""
    return [d for d in (1, 3, SUMSQ_ONE_CHUNK) if piece * d <= SUMSQ_MAX_SAMPLES]


def sumsq_input(samples, seed=0):
    x = 0.8 * np.random.RandomState(5000 + seed + samples % 9973).randn(samples)
    return np.clip(x, -3.3, 3.3).astype(np.float32)


def sumsq_reference(mid, piece, divisions, gain):
    rows = np.clip(mid[:piece * divisions].astype(np.float64) * gain, -1.0, 1.0).reshape(divisions, piece)
    return (rows * rows).sum(axis=1, dtype=np.longdouble).astype(np.float64)


# =====================================================================================================================
# 6. the limiter's early-out (hyrax.py:83-85: numpy.isclose(max(peak, threshold) / threshold, 1))
# =====================================================================================================================
def early_out_peaks(threshold):
    """The sixteen float32 values nearest threshold * (1 + 1e-5 + 1e-8), eight on each side, ascending."""
    edge = threshold * (1.0 + 1e-5 + 1e-8)
    v = np.float32(edge)
    below = v if float(v) < edge else np.nextafter(v, np.float32(0))
    out = [below]
    for _ in range(7):
        out.insert(0, np.nextafter(out[0], np.float32(0)))
    for _ in range(8):
        out.append(np.nextafter(out[-1], np.float32(2)))
    return np.array(out, dtype=np.float32)


def limiter_is_active(peak, threshold):
    """The float64 statement on a float32 peak."""
    return abs(max(float(np.float32(peak)), threshold) / threshold - 1.0) > 1e-8 + 1e-5


# name -> (frames, frame of the peak, channel, sign)
EARLY_OUT_PLACES = {
    "left": (4096 * 3 + 1, 1000, 0, 1.0),
    "right_negative": (4096 * 3 + 1, 5000, 1, -1.0),
    "last_frame": (4096 * 3 + 1, 4096 * 3, 0, 1.0),                    # a block of one frame
    "block_300": (4096 * 300 + 17, 4096 * 300 + 5, 1, 1.0),            # k_finalize_scalars strides past its 256 threads
}


@functools.lru_cache(maxsize=1)
def _early_out_bed(place):
    n, at, _, _ = EARLY_OUT_PLACES[place]
    return (0.5 * np.random.RandomState(6000 + at % 9973).uniform(-1.0, 1.0, (n, 2))).astype(np.float32)


def early_out_track(place, peak):
    """Samples of at most 0.5 with one sample of +-peak."""
    _, at, channel, sign = EARLY_OUT_PLACES[place]
    x = _early_out_bed(place).copy()
    x[at, channel] = np.float32(sign) * np.float32(peak)
    return x


# =====================================================================================================================
# B. level correction outside its band (csrc/correction_kernels.h: BAND_G_LO, BAND_G_HI)
# =====================================================================================================================
BAND_G_LO, BAND_G_HI = 0.7, 1.5
BAND_RATE = 44100
BAND_CONFIG = dict(max_piece_size=0.6, fft_size=1024)


def _noise():
    return np.random.RandomState(1).randn(3 * BAND_RATE, 2) * 0.2


def _up_midway():
    from matchering_amd.synth import make_pair

    target, reference = make_pair(3.0, BAND_RATE, pair=5, reference_seconds=2.6)
    return target, np.clip(40.0 * reference, -0.98, 0.98)


def _down_at_once():
    noise = _noise()
    n = noise.shape[0]
    spectrum = np.fft.rfft(noise, axis=0)
    spectrum[np.arange(spectrum.shape[0]) % 256 >= 16] = 0.0
    target = np.fft.irfft(spectrum, n, axis=0)
    return target * (0.2 / np.abs(target).max()), noise[:int(2.6 * BAND_RATE)]


def _far_up():
    noise = _noise()
    target = np.zeros_like(noise)
    target[::997] = 0.9
    return target, noise[:int(2.6 * BAND_RATE)]


# name -> (pair, correction rounds, the route of rounds 1, 2, ... ("band" or "stream"))
BAND_EXITS = {
    # an ordinary pair against a hard-clipped reference: running gains 1.2656, 1.4337, 1.5521, 1.6387
    "up_midway": (_up_midway, 4, ["band", "band", "stream"]),
    # ... on to 1.88: nine rounds stream in one tail launch
    "up_midway_12": (_up_midway, 12, ["band", "band"] + ["stream"] * 9),
    # a target of sixteen bins in every 256 against broadband noise: 0.5245, then 0.5241
    "down_at_once": (_down_at_once, 4, ["stream"] * 3),
    # a click every 997 frames against the same noise: 4.77, 18.97, 31.5, 34.0, 35.0, 35.3
    "far_up": (_far_up, 6, ["stream"] * 5),
}


def band_exit_pair(name):
    target, reference = BAND_EXITS[name][0]()
    return np.ascontiguousarray(target, dtype=np.float32), np.ascontiguousarray(reference, dtype=np.float32)


def band_exit_config(name):
    return dict(BAND_CONFIG, rms_correction_steps=BAND_EXITS[name][1])


def check_band_routes(name, coefficients):
    """The gain a round starts from -- the product of the coefficients before it -- lies inside the band for the rounds
    meant to read the band lists and outside it by 1 % at least for the rounds meant to stream the mid plane again.
    Returns the running gains."""
    running = np.cumprod(np.asarray(coefficients, dtype=np.float64))
    routes = BAND_EXITS[name][2]
    assert len(routes) == running.shape[0] - 1
    for r, route in enumerate(routes, start=1):
        g = running[r - 1]
        if route == "band":
            assert BAND_G_LO <= g <= BAND_G_HI, (name, r, g)
        else:
            assert g <= BAND_G_LO * 0.99 or g >= BAND_G_HI * 1.01, (name, r, g)
    return running
