"""Float64 restatement of the noise-shaped deliveries (include/mgx.h: mgx_deliver_shaped, mgx_delivery_gain_shaped,
mgx_noise_shaper_preset) in plain Python and numpy loops: the segmented error feedback frame by frame, vectorised over the
chains only (no chain depends on another), the presets, the head-room.  Nothing here knows about tiles, steps or the LDS.
Test infrastructure; shared by the CPU and the GPU tests."""

import math

import numpy as np

import delivery_oracle
from delivery_oracle import decoded, packed, philox  # noqa: F401  (the generator and the byte order are mgx_deliver's)

SEGMENT, WARMUP, TAPS_MAX = 1024, 64, 16          # MGX_SHAPER_SEGMENT, MGX_SHAPER_WARMUP, MGX_SHAPER_TAPS_MAX
SLACK = 1.0 + 2.0 ** -20
LIPSHITZ5 = (2.033, -2.165, 1.959, -1.590, 0.6149)
WANNAMAKER9 = (2.412, -3.370, 3.937, -4.174, 3.353, -2.205, 1.281, -0.569, 0.0847)
PRESETS = {1: LIPSHITZ5, 2: WANNAMAKER9}
PRESET_RATES = (44100, 48000)


def scaled_and_dither(x, gain, bits, seed):
    """a[n][2] and d[n][2]: exactly mgx_deliver's values at dither 1."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 2)
    top = float(2 ** (bits - 1) - 1)
    a = (x.astype(np.float64) * float(gain)) * top
    return a, delivery_oracle.dither(x.size, 1, seed).reshape(-1, 2), top


def feedback(a, d, coefficients, segment=SEGMENT, warmup=WARMUP):
    """r[n][2] before the clip: every chain (segment, channel) from frame max(0, j B - W) with e = 0; the frames before
    j B are computed and not kept.  ``segment`` >= n with any warm-up is the purely sequential filter."""
    n = a.shape[0]
    c = [float(v) for v in coefficients]
    K = len(c)
    segments = -(-n // segment)
    starts = np.arange(segments) * segment
    r_out = np.zeros((n, 2))
    e = [np.zeros((segments, 2)) for _ in range(K)]                 # e[k - 1] = e_k of every chain
    for step in range(-warmup, segment):
        m = starts + step                                           # this step's frame of every segment
        live = (m >= 0) & (m < n)
        if not live.any():
            continue
        idx = np.where(live, m, 0)
        t = np.zeros((segments, 2))
        for k in range(K):
            t = t + c[k] * e[k]                                     # one product and one sum per tap, in this order
        w = a[idx] - t
        r = np.rint(w + d[idx])
        e_new = r - w
        keep = live[:, None]
        # (a chain outside the track stays as it is: before frame 0 that is e = 0, behind the end nothing reads it)
        e = [np.where(keep, new, old) for new, old in zip([e_new] + e[:-1], e)] if K else e
        if step >= 0:
            r_out[m[live]] = r[live]
    return r_out


def deliver_shaped(x, gain, bits, coefficients, seed, segment=SEGMENT, warmup=WARMUP):
    """mgx_deliver_shaped: the integer values (int64, (n, 2)) of the file."""
    a, d, top = scaled_and_dither(x, gain, bits, seed)
    if a.shape[0] == 0:
        return np.zeros((0, 2), dtype=np.int64)
    return np.clip(feedback(a, d, coefficients, segment, warmup), -top - 1.0, top).astype(np.int64)


def sequential_reference(x, gain, bits, coefficients, seed):
    """One frame after the other in plain Python floats, no segments: the textbook error-feedback quantiser (what
    ``feedback`` must give with segment >= n).  Small inputs only."""
    a, d, top = scaled_and_dither(x, gain, bits, seed)
    out = np.zeros(a.shape, dtype=np.int64)
    for ch in range(2):
        e = [0.0] * len(coefficients)
        for m in range(a.shape[0]):
            t = 0.0
            for k, ck in enumerate(coefficients):
                t = t + float(ck) * e[k]
            w = float(a[m, ch]) - t
            r = float(np.rint(w + float(d[m, ch])))
            e = ([r - w] + e[:-1]) if e else e
            out[m, ch] = int(min(max(r, -top - 1.0), top))
    return out


def ntf_power(coefficients, freqs, rate):
    """|H(f)|^2, H(z) = 1 - sum c[k] z^-k."""
    omega = 2.0 * np.pi * np.asarray(freqs, dtype=np.float64) / float(rate)
    h = np.ones_like(omega, dtype=np.complex128)
    for k, ck in enumerate(coefficients, start=1):
        h = h - float(ck) * np.exp(-1j * omega * k)
    return np.abs(h) ** 2


def error_lsb(coefficients):
    """e_shaped = (3/2)(1 + sum |c|)(1 + 2^-20)."""
    total = 0.0
    for ck in coefficients:
        total += abs(float(ck))
    return 1.5 * (1.0 + total) * SLACK


def room(ceiling_dbtp, bits, coefficients):
    """The numerator of g_peak and the limiter's ceiling: 10^(ceiling / 20) - A e_shaped / 2^(bits-1)."""
    return 10.0 ** (float(ceiling_dbtp) / 20.0) - delivery_oracle.interpolator_gain() * error_lsb(coefficients) / 2.0 ** (bits - 1)


def delivery_gain(target, ceiling, bits, coefficients, integrated, true_peak):
    """mgx_delivery_gain_shaped: mgx_delivery_gain's rule with the shaper's head-room."""
    target = math.nan if target is None else float(target)
    ceiling = math.nan if ceiling is None else float(ceiling)
    has_loud = not math.isnan(target) and math.isfinite(integrated)
    g_loud = 10.0 ** ((target - integrated) / 20.0) if has_loud else 1.0
    g_peak = math.inf
    if not math.isnan(ceiling):
        left = room(ceiling, bits, coefficients)
        if not left > 0.0:
            raise ValueError("ceiling_dbtp")
        if true_peak > 0.0:
            g_peak = left / true_peak
    gain = min(g_loud, g_peak)
    by_peak = g_peak < g_loud
    return delivery_oracle.Gain(gain, integrated + 20.0 * math.log10(gain) if math.isfinite(integrated) else -math.inf,
                                gain * true_peak, 20.0 * math.log10(g_loud / gain) if by_peak and has_loud else 0.0,
                                2 if by_peak else (1 if has_loud else 0))
