"""The visuals of include/mgx.h, "Visuals" (V1) - (V3), restated in float64 with numpy and scipy only: the waveform
overview and the spectrogram of (n, 2) float32 frames.  Test infrastructure: the reference the GPU tests and the CPU
emulation are held to."""
import numpy as np
import scipy.fft


def hops(n, hop):
    return (n - 1) // hop + 1 if n > 0 else 0


def column_bounds(count, columns):
    """[columns + 1] int64: column c covers items [b[c], b[c + 1]) of ``count``."""
    c = np.arange(columns + 1, dtype=object)                      # (Python integers: 64-bit products cannot wrap)
    return np.array([int(v) * int(count) // int(columns) for v in c], dtype=np.int64)


def plan(n, hop, columns):
    """(T, W) of mgx_spectrogram_plan."""
    t = hops(n, hop)
    return t, (t if columns == 0 else columns) if n > 0 else 0


def window(fft_size):
    """Periodic Hann, float64 rounded to float32."""
    i = np.arange(fft_size, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * i / fft_size)).astype(np.float32)


def channels_of(x, mode):
    """(n, 2) float32 -> the two float32 channels that are transformed: left / right, or mid / side as the analysis
    forms them in float32."""
    x = np.asarray(x, dtype=np.float32)
    if mode in (0, "lr"):
        return x
    m = (x[:, 0] + x[:, 1]) * np.float32(0.5)
    s = m - x[:, 1]
    return np.stack([m, s], axis=1).astype(np.float32)


def hop_frames(ch, t, hop, fft_size, dtype=np.float64):
    """Hop t: frames [t hop - N/2, t hop + N/2), zero outside the track; (N, 2)."""
    n = ch.shape[0]
    start = t * hop - fft_size // 2
    out = np.zeros((fft_size, 2), dtype=dtype)
    a, b = max(start, 0), min(start + fft_size, n)
    if b > a:
        out[a - start:b - start] = ch[a:b]
    return out


def hop_powers(x, fft_size, hop, mode=0, float32=False):
    """(T, 2, N/2 + 1): P_t[k] = |X_t[k]|^2 (2 / sum w)^2.  ``float32``: the yardstick -- scipy's float32 transform of
    float32 windowed hops -- instead of float64."""
    ch = channels_of(x, mode)
    w32 = window(fft_size)
    scale = (2.0 / np.sum(w32.astype(np.float64))) ** 2
    count = hops(ch.shape[0], hop)
    out = np.zeros((count, 2, fft_size // 2 + 1), dtype=np.float64)
    for t in range(count):
        if float32:
            seg = hop_frames(ch, t, hop, fft_size, np.float32) * w32[:, None]
            spec = scipy.fft.rfft(seg.astype(np.float32), axis=0)
            assert spec.dtype == np.complex64
        else:
            seg = hop_frames(ch, t, hop, fft_size) * w32.astype(np.float64)[:, None]
            spec = scipy.fft.rfft(seg, axis=0)
        spec = spec.astype(np.complex128)
        out[t] = (spec.real ** 2 + spec.imag ** 2).T * scale
    return out


def pool(powers, columns, edges):
    """(T, 2, bins) -> (W, 2, B): the mean over each column's hops, then over each band's bins."""
    count = powers.shape[0]
    bounds = column_bounds(count, columns)
    edges = np.asarray(edges, dtype=np.int64)
    out = np.zeros((columns, 2, edges.size - 1), dtype=np.float64)
    for c in range(columns):
        mean = powers[bounds[c]:bounds[c + 1]].mean(axis=0)
        for b in range(edges.size - 1):
            out[c, :, b] = mean[:, edges[b]:edges[b + 1]].mean(axis=1)
    return out


def spectrogram(x, fft_size, hop, columns, edges, mode=0, float32=False):
    """(W, 2, B) float64 linear power; n == 0: (0, 2, B)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 2)
    _, width = plan(x.shape[0], hop, columns)
    if width == 0:
        return np.zeros((0, 2, len(edges) - 1))
    return pool(hop_powers(x, fft_size, hop, mode, float32), width, edges)


def overview(x, columns):
    """(lo, hi, sumsq): (W, 2) float32 least and largest sample (NaN skipped) and the (W, 2) float64 sum of squares --
    squares are their own magnitudes, so the sum is also what a bound on its rounding is taken of."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 2)
    bounds = column_bounds(x.shape[0], columns)
    lo = np.zeros((columns, 2), dtype=np.float32)
    hi = np.zeros((columns, 2), dtype=np.float32)
    sq = np.zeros((columns, 2), dtype=np.float64)
    for c in range(columns):
        part = x[bounds[c]:bounds[c + 1]]
        lo[c] = np.fmin.reduce(part, axis=0, initial=np.float32(np.inf))
        hi[c] = np.fmax.reduce(part, axis=0, initial=np.float32(-np.inf))
        squares = part.astype(np.float64) ** 2
        sq[c] = squares.sum(axis=0)
    return lo, hi, sq
