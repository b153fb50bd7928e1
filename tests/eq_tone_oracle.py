"""The matching EQ's tone controls (include/mgx.h, mgx_eq_tone) restated in float64 numpy on top of tests/eq_oracle.py and
oracle/mastering_oracle.py.  A helper, not a test: the three per-bin terms, the toned curve, and the taps of one channel
or of a pair.

A tone here is a plain dict with the keys of ``TONE_DEFAULT`` (None: open / off / the shape's amount); ``bands`` is a
sequence of ``(kind, channels, hz, gain_db, q)`` with kind 0 bell, 1 low shelf, 2 high shelf and channels 1 mid, 2 side,
3 both."""

import numpy as np

import eq_oracle
import mastering_oracle as mo

TONE_DEFAULT = dict(low_hz=None, high_hz=None, range_octaves=1.0, side_amount=None, mono_below_hz=None, mono_octaves=1.0,
                    tilt_db_per_octave=0.0, tilt_pivot_hz=1000.0, bands=())


def tone_of(**given):
    unknown = set(given) - set(TONE_DEFAULT)
    assert not unknown, unknown
    return dict(TONE_DEFAULT, **given)


def is_neutral(tone):
    return tone is None or (tone["low_hz"] is None and tone["high_hz"] is None and tone["side_amount"] is None
                            and tone["mono_below_hz"] is None and tone["tilt_db_per_octave"] == 0.0 and not tone["bands"])


def frequencies(fft, fs):
    """f_k = (k * fs) / F for k = 0 .. F/2, the product first."""
    return (np.arange(fft // 2 + 1, dtype=np.float64) * float(fs)) / float(fft)


def ramp(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x <= 0.0, 0.0, np.where(x >= 1.0, 1.0, 0.5 - 0.5 * np.cos(np.pi * np.clip(x, 0.0, 1.0))))


def edge(f, f0, w):
    f = np.asarray(f, dtype=np.float64)
    if w == 0.0:
        return np.where(f >= f0, 1.0, 0.0)
    return ramp(np.log2(f / f0) / w + 0.5)


def band_db(band, f):
    kind, _, hz, gain_db, q = band
    with np.errstate(over="ignore"):
        if kind == 0:
            return gain_db / (1.0 + (q * (f / hz - hz / f)) ** 2)
        ratio = f / hz if kind == 1 else hz / f
        return gain_db / (1.0 + ratio ** (4.0 * q))


def terms(fft, fs, channel, tone, amount=1.0):
    """(a * w, t, g) of ``channel`` (0 mid, 1 side), each F/2 + 1 values with entry 0 zero."""
    f = frequencies(fft, fs)[1:]
    w = np.ones_like(f)
    if tone["low_hz"] is not None:
        w = edge(f, tone["low_hz"], tone["range_octaves"])
    if tone["high_hz"] is not None:
        w = w * (1.0 - edge(f, tone["high_hz"], tone["range_octaves"]))
    a = tone["side_amount"] if channel == 1 and tone["side_amount"] is not None else amount
    t = tone["tilt_db_per_octave"] * np.log2(f / tone["tilt_pivot_hz"])
    for band in tone["bands"]:
        if band[1] & (1 << channel):
            t = t + band_db(band, f)
    g = edge(f, tone["mono_below_hz"], tone["mono_octaves"]) if channel == 1 and tone["mono_below_hz"] is not None \
        else np.ones_like(f)
    return tuple(np.concatenate(([0.0], v)) for v in (a * w, t, g))


def tone_curve(smooth, min_value, fs, channel, tone, amount=1.0, max_boost_db=None, max_cut_db=None):
    """Step 1 with a tone.  A neutral tone is eq_oracle.shape_curve: the call without a tone."""
    smooth = np.asarray(smooth, dtype=np.float64)
    if is_neutral(tone):
        return eq_oracle.shape_curve(smooth, min_value, amount, max_boost_db, max_cut_db)
    fft = 2 * (smooth.shape[0] - 1)
    aw, t, g = terms(fft, fs, channel, tone, amount)
    d = aw[1:] * (20.0 * np.log10(np.maximum(smooth[1:], min_value)))
    if max_boost_db is not None:
        d = np.minimum(d, max_boost_db)
    if max_cut_db is not None:
        d = np.maximum(d, -max_cut_db)
    out = np.empty_like(smooth)
    out[0] = 0.0
    out[1:] = 10.0 ** ((d + t[1:]) / 20.0) * g[1:]
    return out


def tone_fir(smooth, min_value, fs, channel, tone, amount=1.0, max_boost_db=None, max_cut_db=None, phase="linear",
             float32_linear=False):
    """Steps 1 to 3 for one channel under a tone (eq_oracle.shape_fir's steps 2 and 3 on the toned curve)."""
    lin = eq_oracle.linear_taps(tone_curve(smooth, min_value, fs, channel, tone, amount, max_boost_db, max_cut_db))
    if phase == "linear":
        return lin
    if float32_linear:
        lin = lin.astype(np.float32).astype(np.float64)
    return eq_oracle.minimum_phase(lin)


def pair_taps(target, reference, cfg, tone, **shape):
    """(mid taps, side taps, trace) of a pair under a shape and a tone: the oracle's own curves, toned."""
    trace = {}
    mo.master(target, reference, cfg, False, True, False, trace=trace)
    fs = cfg.internal_sample_rate
    mid = tone_fir(trace["mid"].smooth, cfg.min_value, fs, 0, tone, **shape)
    side = tone_fir(trace["side"].smooth, cfg.min_value, fs, 1, tone, **shape)
    return mid, side, trace


def response_db(taps, hz, fs):
    """|H| of the taps at arbitrary frequencies, in dB: the plain sum, not an FFT grid."""
    n = np.arange(taps.shape[0], dtype=np.float64)
    hz = np.atleast_1d(np.asarray(hz, dtype=np.float64))
    h = np.exp(-2j * np.pi * np.outer(hz / fs, n)) @ np.asarray(taps, dtype=np.float64)
    return 20.0 * np.log10(np.maximum(np.abs(h), 1e-300))
