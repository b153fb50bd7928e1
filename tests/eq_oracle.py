"""The matching EQ's controls (include/mgx.h, mgx_eq_shape) restated in float64 numpy on top of oracle/mastering_oracle.py.
A helper, not a test: the shape stage on a smoothed curve, the linear-phase synthesis (match_frequencies.py:98-99), the
minimum-phase form by the folded cepstrum on N = 4F points, and the pair of taps ``mastering_oracle.master(fir=...)``
takes."""

import numpy as np
from scipy import signal

import mastering_oracle as mo

FLOOR = 1e-9
OVERSAMPLE = 4


def shape_curve(smooth, min_value, amount=1.0, max_boost_db=None, max_cut_db=None):
    """Step 1.  Skipped entirely (not multiplied by one) at amount 1 without caps."""
    smooth = np.asarray(smooth, dtype=np.float64)
    if amount == 1.0 and max_boost_db is None and max_cut_db is None:
        return smooth.copy()
    d = amount * 20.0 * np.log10(np.maximum(smooth[1:], min_value))
    if max_boost_db is not None:
        d = np.minimum(d, max_boost_db)
    if max_cut_db is not None:
        d = np.maximum(d, -max_cut_db)
    out = np.empty_like(smooth)
    out[0] = 0.0
    out[1:] = 10.0 ** (d / 20.0)
    return out


def linear_taps(curve):
    """Step 2: the reference's synthesis, float64."""
    taps = np.fft.irfft(curve)
    return np.fft.ifftshift(taps) * signal.windows.hann(taps.shape[0])


def minimum_phase(lin, oversample=OVERSAMPLE, permute=None):
    """Step 3 from linear-phase taps (float64, or float32 widened).  ``permute``: a test's knob -- the transforms are
    evaluated as matrix-free DFTs of a circularly shifted signal with the shift undone in the spectrum, i.e. the same
    numbers through another summation order."""
    lin = np.asarray(lin, dtype=np.float64)
    f = lin.shape[0]
    n = oversample * f

    def fft(x):
        if permute is None:
            return np.fft.fft(x)
        k = np.arange(n)
        return np.fft.fft(np.roll(x, permute)) * np.exp(2j * np.pi * k * permute / n)

    def ifft(x):
        if permute is None:
            return np.fft.ifft(x)
        k = np.arange(n)
        return np.fft.ifft(np.roll(x, permute)) * np.exp(-2j * np.pi * k * permute / n)

    padded = np.zeros(n)
    padded[:f] = lin
    h = np.abs(fft(padded))
    log_h = np.log(np.maximum(h, FLOOR * h.max()))
    c = ifft(log_h).real
    fold = np.zeros(n)
    fold[0] = c[0]
    fold[n // 2] = c[n // 2]
    fold[1:n // 2] = 2.0 * c[1:n // 2]
    g = ifft(np.exp(fft(fold))).real
    j = np.arange(f // 2)
    taper = np.where(j < f // 4, 1.0, 0.5 * (1.0 + np.cos(np.pi * (j - f // 4) / (f // 4))))
    taps = np.zeros(f)
    taps[f // 2:] = g[:f // 2] * taper
    return taps


def shape_fir(smooth, min_value, amount=1.0, max_boost_db=None, max_cut_db=None, phase="linear", float32_linear=False):
    """Steps 1 to 3 for one channel.  ``float32_linear``: round the linear taps to float32 before step 3, as the device
    does (they live as float32 in the handle)."""
    lin = linear_taps(shape_curve(smooth, min_value, amount, max_boost_db, max_cut_db))
    if phase == "linear":
        return lin
    if float32_linear:
        lin = lin.astype(np.float32).astype(np.float64)
    return minimum_phase(lin)


def pair_taps(target, reference, cfg, **shape):
    """(mid taps, side taps, trace) of a pair under a shape: the oracle's own curves, shaped."""
    trace = {}
    mo.master(target, reference, cfg, False, True, False, trace=trace)
    mid = shape_fir(trace["mid"].smooth, cfg.min_value, **shape)
    side = shape_fir(trace["side"].smooth, cfg.min_value, **shape)
    return mid, side, trace


def magnitude_db(taps, f=None):
    """|rfft| of the taps on their own F grid, in dB."""
    return 20.0 * np.log10(np.maximum(np.abs(np.fft.rfft(taps, f)), 1e-300))
