"""Case tables, inputs, float64 references and float32 yardsticks of the stage sweeps.

Shared by tests/test_emu_stage_sweeps.py (the kernels' phase functions on the CPU) and tests/test_gpu_stage_sweeps.py
(the kernels themselves), so that what a machine without a GPU checks is what the GPU run checks.  No tests here.

A *reference* is the operation in float64 numpy/scipy on the float32-rounded input (oracle/mastering_oracle.py).  A
*yardstick* is the same operation done by scipy in float32: what an unrelated float32 implementation loses on the very
same input.  Bounds that are not the project's own are multiples of a yardstick, never of what a kernel returned.
"""
from types import SimpleNamespace

import numpy as np
import scipy.fft
from scipy import signal

import mastering_oracle as mo
from conftest import rms_error

SAMPLE_RATE = 44100
MAX_FRAMES = 1500 * 8192 + 17            # the longest input of tests/test_gpu_parity.py: no sweep goes beyond it

# what the tests measured, for the tables in their docstrings: (stage, key, kernel error, yardstick error)
MEASURED = []


def record(stage, key, kernel, yardstick):
    MEASURED.append((stage, key, float(kernel), float(yardstick)))
    print(f"SWEEP {stage} {key} kernel={kernel:.3e} yardstick={yardstick:.3e}")


# =====================================================================================================================
# A. analysis
# =====================================================================================================================
FFT_SIZES = [8 << i for i in range(14)]                  # 8 .. 65536
CUS, ANALYZE_MAX_WGS = 256, 8                            # MI355X; mgx_kernels.h ANALYZE_MAX_WGS


def analysis_cases(fft):
    """name -> dict(D, q, left, tail, spike, emu): `D` pieces of q * fft + left frames and `tail` (< D) ignored frames
    behind them.  `spike`: where the track's largest sample sits.  `emu`: the emulation runs it too."""
    f = fft
    cases = {
        # piece an exact multiple of fft_size and n == divisions * piece: the last segment ends on the buffer's last
        # frame (k_analyze<14> asks for the segment behind it: the request lies wholly past the view and answers zeros)
        "exact": dict(D=3, q=2, left=0, tail=0, spike=None, emu=True),
        # the largest leftover, with the track's largest sample inside piece 1's leftover: it counts for that piece's
        # RMS and for the peak, and belongs to no segment
        "leftover_peak": dict(D=3, q=3, left=f - 1, tail=0, spike="leftover", emu=True),
        # ... and inside the ignored tail [divisions * piece, n): the peak counts there, the RMS does not
        # (dsp.py:97 against match_levels.py:93-103)
        "tail_peak": dict(D=3, q=2, left=f - 1, tail=2, spike="tail", emu=True),
        "one_segment": dict(D=4, q=1, left=f // 2, tail=1, spike=None, emu=True),
        # a prime number of segments: the emulation deals them to (q + 4) / 5 = 3 chunks of 4, 4 and 5
        "prime_segments": dict(D=2, q=13, left=5, tail=0, spike=None, emu=True),
        "one_division": dict(D=1, q=5, left=3, tail=0, spike=None, emu=True),
    }
    # More workgroups than the chip holds (choose_chunks in run_analysis.h: at most CUs x workgroups-per-CU, the latter at
    # most ANALYZE_MAX_WGS = 8 and at most what the LDS admits: 4 / 2 / 1 for 4096 / 8192 / 16384-point transforms):
    # D * q beyond that forces more than one segment per workgroup, and with q prime the s0/s1 split is uneven.
    if fft <= 256:
        # 300 x 17 = 5100 workgroups > 2048: 3 segments per workgroup, 6 chunks for 17 segments
        cases["many_pieces"] = dict(D=300, q=17, left=f - 1, tail=7, spike="tail", emu=fft >= 64)
    if 64 <= fft <= 32768:
        q = {4096: 521, 8192: 263, 16384: 131, 32768: 131}.get(fft, 1031)      # primes; 2 q > 2048, 1024, 512, 256, 256
        cases["grid_full"] = dict(D=2, q=q, left=1, tail=1, spike=None, emu=False)
    if fft <= 16:
        # k_analyze_small: one thread per segment, 256 segments per trip.  Only beyond 2048 x 256 segments does a
        # workgroup get a second trip: 2 x 270001 segments (at fft_size 32 that is longer than MAX_FRAMES: not reachable)
        cases["second_trip"] = dict(D=2, q=270001, left=3, tail=1, spike=None, emu=False)
    return cases


def analysis_geometry(fft, case):
    """(n, max_piece_size in seconds) for a case: divisions = int(n / max) + 1 = D needs n / max in [D - 1, D): the
    middle of it; piece = int(n / D) = q fft + left needs tail < D."""
    d, piece = case["D"], case["q"] * fft + case["left"]
    assert case["tail"] < d
    n = d * piece + case["tail"]
    return n, n / (d - 0.5) / SAMPLE_RATE


def piece_gains(divisions):
    """Gain of each piece: even pieces 0.80 .. 0.99, odd pieces 0.30 .. 0.45, in steps of 1 % of full scale, so that
    neighbours differ by a third at least and the average that decides the loud set (about 0.7 of the comb's or the noise's
    own level) lies in the gap between the two groups: no piece's RMS ties with it, however short the pieces."""
    d = np.arange(divisions)
    return np.where(d & 1, 0.30 + 0.01 * ((d // 2 * 3) % 16), 0.80 + 0.01 * ((d // 2 * 7) % 20))


def comb_amplitudes(fft):
    """Amplitudes of the cosines at bins 0 .. fft/2 of mid and of side, before the common scale: both fall 40 dB from
    bin 0 to bin fft/2; side is lower and carries a ripple from odd to even bins, so that no two bins of the two
    spectra agree."""
    half = fft // 2
    k = np.arange(half + 1)
    a_mid = 10.0 ** (-2.0 * k / half)
    a_side = 0.4 * 10.0 ** (-2.0 * k / half) * (1.0 + 0.5 * (k & 1))
    return a_mid, a_side


def comb_period(fft, seed):
    """One period of the bin comb: mid and side as sums of cosines at every exact bin centre k / fft with random phases
    (0 at bins 0 and fft/2, whose cosines would otherwise lose amplitude to their phase).  Returns (L, R, amplitudes of
    mid, of side), scaled so that max(|L|, |R|) = 0.9."""
    rng = np.random.RandomState(seed)
    half = fft // 2
    a_mid, a_side = comb_amplitudes(fft)

    def period(amp):
        phase = rng.uniform(0.0, 2.0 * np.pi, half + 1)
        phase[0] = phase[half] = 0.0
        spec = 0.5 * fft * amp * np.exp(1j * phase)
        spec[0] = fft * amp[0]
        spec[half] = fft * amp[half]
        return np.fft.irfft(spec, fft)

    mid, side = period(a_mid), period(a_side)
    left, right = mid + side, mid - side
    scale = 0.9 / max(np.abs(left).max(), np.abs(right).max())
    return left * scale, right * scale, a_mid * scale, a_side * scale


def analysis_input(fft, case, kind, seed=0):
    """(n, 2) float32 track for a case.  kind: 'comb', 'noise', 'mono' (L == R), 'panned' (R == 0)."""
    n, _ = analysis_geometry(fft, case)
    piece = case["q"] * fft + case["left"]
    if kind == "comb":
        left, right, _, _ = comb_period(fft, seed + fft)
        reps = -(-n // fft)
        x = np.stack((np.tile(left, reps)[:n], np.tile(right, reps)[:n]), axis=1)
    else:
        rng = np.random.RandomState(seed + fft + 1)
        x = (0.3 * rng.randn(n, 2)).astype(np.float32).astype(np.float64)
        x = np.clip(x, -0.9, 0.9)
        if kind == "mono":
            x[:, 1] = x[:, 0]
        elif kind == "panned":
            x[:, 1] = 0.0
        else:
            assert kind == "noise"
    gain = piece_gains(case["D"])[np.minimum(np.arange(n) // piece, case["D"] - 1)]
    x = (x * gain[:, None]).astype(np.float32)
    if case["spike"] is not None:
        at = n - 1 if case["spike"] == "tail" else piece + case["q"] * fft + (fft - 1) // 2
        assert (case["D"] * piece <= at < n) if case["spike"] == "tail" else (piece + case["q"] * fft <= at < 2 * piece)
        x[at] = (0.95, 0.2) if kind not in ("mono", "panned") else ((0.95, 0.95) if kind == "mono" else (0.95, 0.0))
        assert np.abs(x).max() == np.float32(0.95) and np.count_nonzero(np.abs(x) == np.float32(0.95)) <= 2
    return np.ascontiguousarray(x)


def analysis_configs(fft, case):
    """(matchering_amd Config, oracle parameters) of a case."""
    import matchering_amd as mg

    _, seconds = analysis_geometry(fft, case)
    return mg.Config(fft_size=fft, max_piece_size=seconds), mo.params(fft_size=fft, max_piece_size=seconds)


def analysis_reference(x32, ocfg, is_reference, case, fft):
    """float64 levels and average spectra of the float32 track (match_levels.py:134-161, match_frequencies.py:30-42);
    asserts that the case has the geometry it is meant to have and that the loud set is not decided by a near-tie."""
    x64 = x32.astype(np.float64)
    c = 1.0
    if is_reference:
        x64, c = mo.peak_normalize(x64, ocfg.threshold, ocfg.min_value, False)
    a = mo.analyze(x64, ocfg)
    n = x32.shape[0]
    assert a.divisions == case["D"] and a.piece == case["q"] * fft + case["left"] and a.piece // fft == case["q"]
    assert n - a.divisions * a.piece == case["tail"]
    if a.divisions > 1:                     # (one piece is its own average: nothing to tie with)
        assert np.abs(a.rmses / a.average_rms - 1.0).min() >= 1e-4, "loud-piece decision is a near-tie: change the case"
    return SimpleNamespace(
        divisions=a.divisions, piece=a.piece, rmses=a.rmses, match_rms=a.match_rms, loud_idx=a.loud_idx, c=c,
        peak=float(np.abs(x32).max()), avg_mid=mo.average_spectrum(a.mid_loud, fft),
        avg_side=mo.average_spectrum(a.side_loud, fft))


def comb_closed_form(fft, case, ref, seed=0):
    """Average |rfft| / fft of the comb over the loud pieces: A_k / 2 (A_0 and A_{fft/2} undivided) times the mean gain of
    the loud pieces, over the normalisation."""
    _, _, a_mid, a_side = comb_period(fft, seed + fft)
    g = piece_gains(case["D"])[ref.loud_idx].mean() / ref.c
    shape = np.full(fft // 2 + 1, 0.5)
    shape[0] = shape[-1] = 1.0
    return a_mid * shape * g, a_side * shape * g


def analysis_yardstick(x32, ref, fft):
    """scipy.fft.rfft in float32 on the float32 mid and side of the loud pieces, magnitudes accumulated in float64:
    largest error of a bin against the float64 reference, of the reference's peak bin."""
    x = x32 if ref.c == 1.0 else (x32.astype(np.float64) / ref.c).astype(np.float32)
    mid = (x[:, 0] + x[:, 1]) * np.float32(0.5)
    side = mid - x[:, 1]
    q = ref.piece // fft
    worst = 0.0
    for v, want in ((mid, ref.avg_mid), (side, ref.avg_side)):
        if want.max() == 0.0:
            continue
        rows = v[: ref.divisions * ref.piece].reshape(ref.divisions, ref.piece)[ref.loud_idx, : q * fft]
        spec = scipy.fft.rfft(rows.reshape(-1, fft), axis=-1)
        assert spec.dtype == np.complex64
        got = np.abs(spec).astype(np.float64).mean(axis=0) / fft
        worst = max(worst, np.abs(got - want).max() / want.max())
    return worst


def check_analysis(st, x32, ref, is_reference, key, mono_side=False):
    """`st`: what mgx_analyze returned (kernels.LevelStats or the emulation's equal).  Every bin 0 .. fft/2 is compared."""
    assert st.divisions == ref.divisions and st.piece_size == ref.piece
    assert np.array_equal(np.flatnonzero(st.loud), ref.loud_idx)
    assert np.abs(st.rmses / ref.rmses - 1).max() <= 1e-7
    assert abs(st.match_rms / ref.match_rms - 1) <= 1e-7
    assert st.peak == ref.peak                                   # exactly the float32 maximum
    assert abs(st.amplitude_coefficient - ref.c) <= 1e-7
    assert (ref.c != 1.0) == (is_reference and ref.peak < mo.params().threshold)
    worst = 0.0
    for name, mine, want in (("mid", st.average_spectrum_mid, ref.avg_mid), ("side", st.average_spectrum_side, ref.avg_side)):
        assert mine.shape == want.shape
        err = np.abs(mine - want).max()
        if mono_side and name == "side":
            assert want.max() == 0.0 and err <= 1e-7, (key, name, err)       # the existing test's absolute floor
            continue
        worst = max(worst, err / want.max())
        # the project's own bound (test_analysis_stage): 2e-6 of the peak bin, for every bin
        assert err <= 2e-6 * want.max(), (key, name, err / want.max(), int(np.abs(mine - want).argmax()))
    return worst


# =====================================================================================================================
# B. convolution
# =====================================================================================================================
TAP_COUNTS = [2 << i for i in range(16)]                # 2 .. 65536
CONV_DIRECT_TILE = 1024                                  # small_fft_kernels.h


def conv_route(taps):
    """(route, hop in output frames, frames of one block) as run_conv in run_conv.h decides."""
    if taps <= 32:
        return "direct", CONV_DIRECT_TILE, CONV_DIRECT_TILE
    if taps == 4096:
        return "wide", 12288, 12288
    if taps == 16384:
        return "delay", 8192, 8192
    if taps >= 32768:
        return "partitioned", 16384, 8192
    return "queue", 2 * taps, taps


def conv_lengths(taps, with_grid_overflow=True):
    """Track lengths around the route's hop and around the 'same' offset taps / 2, one odd length of a few hops, and,
    below 2048 taps, one with more blocks than the grid holds at once."""
    route, hop, _ = conv_route(taps)
    ns = [1, 2, hop - 1, hop, hop + 1, 2 * hop + 1, taps // 2 - 1, taps // 2, taps // 2 + 1, (3 * hop + 777) | 1]
    if with_grid_overflow and taps < 2048:
        # workgroups resident at once: CUs x min(2048 / threads, LDS per CU / LDS of a block) -- at most 32 per CU
        # (64-thread workgroups), and at most 160 KB / (8 bytes x 2 taps) where the LDS binds (mgx_hd.h workgroups_per_cu)
        per_cu = 8 if route == "direct" else min(32, (160 * 1024) // (16 * taps))
        ns.append(CUS * per_cu * hop + 1237)
    return sorted({n for n in ns if 0 < n <= MAX_FRAMES})


def conv_taps(taps, kind, seed):
    rng = np.random.RandomState(seed)
    if kind == "random":
        return rng.randn(taps) / np.sqrt(taps), rng.randn(taps) / np.sqrt(taps)
    if kind == "range60":                                # random signs, magnitudes spread over 60 dB
        return tuple(rng.choice([-1.0, 1.0], taps) * 10.0 ** (-3.0 * rng.rand(taps)) for _ in range(2))
    raise ValueError(kind)


def conv_delta(taps, where):
    at = {"first": 0, "last": taps - 1, "centre": (taps - 1) // 2}[where]
    h = np.zeros(taps)
    h[at] = 1.0
    return h, at


def conv_noise(n, seed):
    return (0.3 * np.random.RandomState(seed).randn(n, 2)).astype(np.float32)


def conv_edge_impulses(n, taps):
    """Zero but for impulses on frame 0, frame n - 1 and the two sides of the first block seam (those that exist): the
    output around each is the filter itself, tap 0 and tap taps - 1 included."""
    _, _, block = conv_route(taps)
    x = np.zeros((n, 2), dtype=np.float32)
    for i, at in enumerate((0, n - 1, block - 1, block)):
        if 0 <= at < n:
            x[at] += np.float32((1.0, 0.5)) * np.float32(1.0 - 0.125 * i)       # mid 0.75, side 0.25, exact in float32
    return x


def conv_reference(x32, hm, hs, gain):
    """float64 result (n, 2) and mid of match_frequencies.py:104-119 on the float32 frames."""
    mid, side = mo.mid_side(x32.astype(np.float64))
    want, want_mid = mo.convolve_same(mid * gain, hm, side * gain, hs)
    return np.ascontiguousarray(want), want_mid


def conv_yardstick(x32, hm, hs, gain, want, want_mid):
    """scipy.signal.fftconvolve in float32 on the float32 mid and side with float32 taps: its largest error of a frame
    against the float64 result.  Not below 2^-24: a float32 output of a signal whose full scale is 1 is itself rounded
    that far, and a maximum over the one or two frames of the shortest tracks can fall below it by luck."""
    mid = (x32[:, 0] + x32[:, 1]) * np.float32(0.5)
    side = mid - x32[:, 1]
    ym = signal.fftconvolve(mid, (hm * gain).astype(np.float32), "same")
    ys = signal.fftconvolve(side, (hs * gain).astype(np.float32), "same")
    assert ym.dtype == np.float32 and ys.dtype == np.float32
    want_side = 0.5 * (want[:, 0] - want[:, 1])
    worst = max(np.abs(ym - want_mid).max(), np.abs(ys - want_side).max())
    return max(float(worst), 2.0 ** -24)


# 8 x the yardstick: 2 because L = mid + side adds two errors, 4 for the kernels' other radices, the two-for-one
# un-mixing and contracted FMAs; never more than the project's 5e-6 between two of its own kernels.
CONV_MAX_FACTOR = {"direct": 8.0, "queue": 8.0, "wide": 8.0, "delay": 8.0, "partitioned": 8.0}
CONV_MAX_CAP = 5e-6


def check_convolution(y, ymid, peak, x32, hm, hs, gain, taps, key):
    want, want_mid = conv_reference(x32, hm, hs, gain)
    yard = conv_yardstick(x32, hm, hs, gain, want, want_mid)
    route = conv_route(taps)[0]
    err = max(np.abs(y - want).max(), np.abs(ymid - want_mid).max())
    record("convolve", f"taps={taps} route={route} {key}", err, yard)
    assert rms_error(y, want) <= 1e-6, key
    assert rms_error(ymid, want_mid) <= 1e-6, key
    assert abs(peak - np.abs(y).max()) <= 1e-6, key
    bound = min(CONV_MAX_FACTOR[route] * yard, CONV_MAX_CAP)
    worst = int(np.abs(y - want).max(axis=1).argmax())
    assert err <= bound, (key, err, bound, "frame", worst)
    return err, yard


# =====================================================================================================================
# C. limiter
# =====================================================================================================================
LIMITER_CONFIGS = {
    "44100": dict(sr=44100),                                     # k_limit<256, 4, 44, 43, 26>
    "48000": dict(sr=48000),                                     # k_limit<256, 4, 48, 47, 28>
    "96000": dict(sr=96000),                                     # k_limit<256, 4, 96, 95, 55>
    "22050": dict(sr=22050),                                     # k_limit<256, 4>
    "long_attack": dict(sr=44100, attack=8.0, hold=2.0),         # k_limit<1024, 1>
    "short_windows": dict(sr=44100, attack=0.1, hold=0.1),       # windows read out frame by frame
    "orders_2_2": dict(sr=44100, hold_filter_order=2, release_filter_order=2),     # k_limit_general<2>
    "orders_3_1": dict(sr=44100, hold_filter_order=3, release_filter_order=1),     # k_limit_general<3>
}
SPECIALISED = ("44100", "48000", "96000")


def limiter_configs(name):
    import matchering_amd as mg

    kw = dict(LIMITER_CONFIGS[name])
    sr = kw.pop("sr")
    return mg.Config(internal_sample_rate=sr, limiter=mg.LimiterConfig(**kw)), mo.params(internal_sample_rate=sr, **kw)


def load_emulation():
    """tests/emu/libmgx_emu.so (built when stale): the kernels' phase functions and the host's launch parameters."""
    import emu_build

    return emu_build.load()


def limiter_geometry(emu, cfg):
    """What limiter_params (host_params.h) decides for a configuration: threads (blocks per chunk), core_blocks, chunk
    (frames of a chunk's core), gl, gr (halos in blocks), general (0, or the order k_limit_general runs with)."""
    import ctypes

    native = cfg.to_native()
    vals = [ctypes.c_int() for _ in range(6)]
    assert emu.emu_limiter_geometry(ctypes.byref(native), *[ctypes.byref(v) for v in vals]) == 0
    return SimpleNamespace(**{k: v.value for k, v in zip(("threads", "core_blocks", "chunk", "gl", "gr", "general"), vals)})


def limiter_lengths(chunk):
    return [8, 9, 15, 16, 17, chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk + 1, 5 * chunk + 7]


def limiter_noise(n, seed=0):
    return (0.9 * np.random.RandomState(seed + n).randn(n, 2)).astype(np.float32)


def limiter_spikes(n, chunk, threshold, seed=0):
    """A track capped at half the threshold with single frames of 1.5 on frame 0, frame n - 1, the last frame of chunk
    0's core and the first frame of chunk 1 (those that exist): busy chunks at the ends, window maxima that reach across
    the seam through the halos, and, from three chunks on, quiet chunks (the closed-form path) beside busy ones."""
    rng = np.random.RandomState(seed + n)
    x = (0.5 * threshold * rng.uniform(-1.0, 1.0, (n, 2))).astype(np.float32)
    places = sorted({p for p in (0, n - 1, chunk - 1, chunk) if 0 <= p < n})
    for i, p in enumerate(places):
        x[p] = (1.5, -1.5) if i & 1 else (-1.5, 1.25)
    return x, places


def check_limiter(out, active, x32, ocfg, general, key):
    """Everything but the track's first and last 64 frames (limiter_edge_errors).  Returns (max error, edge error)."""
    want = mo.limit(x32.astype(np.float64), ocfg)
    err, rms = np.abs(out - want).max(), rms_error(out, want)
    edge = max(np.abs(out[:64] - want[:64]).max(), np.abs(out[-64:] - want[-64:]).max())
    print(f"SWEEP limit {key} max={err:.3e} rms={rms:.3e} edges={edge:.3e}")
    assert active is None or active, key
    assert np.abs(out).max() <= ocfg.threshold * (1 + 1e-6), key                  # the brick wall
    assert rms <= 1e-6, (key, rms)
    assert err <= (1e-5 if general else 5e-6), (key, err)
    return err, edge


LIMITER_EDGE_BOUND = 1e-6            # first and last 64 frames, first-order filters (test_limiter_stage)


# =====================================================================================================================
# D. scale
# =====================================================================================================================
SCALE_LENGTHS = [1, 2, 3, 4, 5, 255, 256, 257, 8192 * 256 + 3]      # the last: more frames than the capped grid's stride
SCALE_GAINS = [1.0, 0.0, -0.5, 1.0 / 3.0]
SENTINEL = np.float32(-77.25)


def scale_input(n):
    return (0.7 * np.random.RandomState(n).randn(n, 2)).astype(np.float32)


def scale_reference(x32, gain):
    """The kernel multiplies in float64 and rounds once."""
    return (x32.astype(np.float64) * gain).astype(np.float32)
