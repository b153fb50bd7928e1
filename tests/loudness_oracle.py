"""Float64 numpy / scipy restatement of the loudness meter's definitions (include/mgx.h, mgx_loudness): ITU-R BS.1770-4
K-weighting, gating and true peak, EBU Tech 3341 momentary and short-term loudness, EBU Tech 3342 loudness range.  The
filters run over the whole track with ``scipy.signal.lfilter``, the true peak is one ``numpy.convolve`` per channel:
nothing here knows about tiles, warm-ups or workgroups.  Test infrastructure; shared by the CPU and the GPU tests.
"""

import math
from collections import namedtuple

import numpy as np
from scipy.signal import lfilter

Measured = namedtuple("Measured", "integrated range momentary_max short_term_max true_peak sample_peak sub_energy")

OFFSET, ABSOLUTE = -0.691, -70.0


def k_weighting(fs):
    """((b, a) of the high shelf, (b, a) of the high-pass) at sample rate ``fs``."""
    f0, gain, q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    k = math.tan(math.pi * f0 / fs)
    vh = 10.0 ** (gain / 20.0)
    vb = vh ** 0.4996667741545416
    a0 = 1.0 + k / q + k * k
    shelf = (np.array([(vh + vb * k / q + k * k) / a0, 2.0 * (k * k - vh) / a0, (vh - vb * k / q + k * k) / a0]),
             np.array([1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0]))
    f0, q = 38.13547087602444, 0.5003270373238773
    k = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + k / q + k * k
    high = (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0]))
    return shelf, high


def sub_block_frames(fs):
    return (int(fs) + 5) // 10


def sub_energies(x, fs):
    """e[nsub][2]: the K-weighted energy of every whole sub-block of x[n][2]."""
    x = np.asarray(x, dtype=np.float64)
    size = sub_block_frames(fs)
    nsub = x.shape[0] // size
    if nsub == 0:
        return np.zeros((0, 2))
    shelf, high = k_weighting(fs)
    y = lfilter(high[0], high[1], lfilter(shelf[0], shelf[1], x, axis=0), axis=0)
    return (y[:nsub * size] ** 2).reshape(nsub, size, 2).sum(axis=1)


def lufs(z):
    z = np.asarray(z, dtype=np.float64)
    out = np.full(z.shape, -np.inf)
    np.log10(z, out=out, where=z > 0)
    out[z > 0] = OFFSET + 10.0 * out[z > 0]
    return out


def block_powers(e, size, length, step):
    """Mean square (both channels, weights 1) of the blocks of ``length`` sub-blocks starting every ``step``."""
    total = np.asarray(e, dtype=np.float64).reshape(-1, 2).sum(axis=1)
    starts = range(0, len(total) - length + 1, step)
    return np.array([total[j:j + length].sum() / (length * size) for j in starts], dtype=np.float64)


def relative_gate(z, relative):
    """The gate of the second stage: ``relative`` LU from the loudness of the blocks above the absolute gate, or None."""
    loud = z[lufs(z) > ABSOLUTE]
    return None if loud.size == 0 else float(lufs(np.array([loud.mean()]))[0]) + relative


def gated(z, relative):
    gate = relative_gate(z, relative)
    if gate is None:
        return z[:0]
    level = lufs(z)
    return z[(level > ABSOLUTE) & (level > gate)]


def gate_margin(e, fs):
    """Smallest distance in LU of a gated block's loudness from the absolute gate or from its relative gate, over the
    integrated measure and the range: the tests require it to be large against the bounds they assert."""
    size = sub_block_frames(fs)
    worst = np.inf
    for length, step, relative in ((4, 1, -10.0), (30, 10, -20.0)):
        z = block_powers(e, size, length, step)
        level = lufs(z)
        finite = level[np.isfinite(level)]
        if finite.size:
            worst = min(worst, float(np.abs(finite - ABSOLUTE).min()))
        gate = relative_gate(z, relative)
        if gate is not None and finite.size:
            worst = min(worst, float(np.abs(finite - gate).min()))
    return worst


def gate(e, fs):
    """(integrated, range, momentary_max, short_term_max) from sub-block energies."""
    size = sub_block_frames(fs)
    momentary = block_powers(e, size, 4, 1)
    short = block_powers(e, size, 30, 1)
    kept = gated(momentary, -10.0)
    integrated = float(lufs(np.array([kept.mean()]))[0]) if kept.size else -np.inf
    levels = np.sort(lufs(gated(block_powers(e, size, 30, 10), -20.0)))
    spread = 0.0
    if levels.size:
        m1 = levels.size - 1
        spread = float(levels[int(m1 * 0.95 + 0.5)] - levels[int(m1 * 0.10 + 0.5)])
    return (integrated, spread, float(lufs(momentary).max()) if momentary.size else -np.inf,
            float(lufs(short).max()) if short.size else -np.inf)


def true_peak_taps():
    k = np.arange(-24, 25)
    return np.sinc(k / 4.0) * np.kaiser(49, 8.0)


def peaks(x):
    """(true peak, sample peak) of x[n][2], linear."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    if n == 0:
        return 0.0, 0.0
    taps = true_peak_taps()
    best = 0.0
    for c in range(x.shape[1]):
        up = np.zeros(4 * n)
        up[::4] = x[:, c]
        over = np.convolve(up, taps)[24:24 + 4 * n]          # entry 4 m + p: phase p at frame m
        best = max(best, float(np.abs(over).max()))
    return best, float(np.abs(x).max())


def measure(x, fs):
    e = sub_energies(x, fs)
    true_peak, sample_peak = peaks(x)
    return Measured(*gate(e, fs), true_peak, sample_peak, e)
