"""Float64 numpy restatement of the deliveries' true-peak limiter (include/mgx.h: mgx_tp_limit, mgx_delivery_limit_step)
and of the pipeline ``stages.main`` runs for a delivery that carries one: limit -> ``loudness_oracle.measure`` ->
``delivery_oracle.delivery_gain`` -> ``delivery_oracle.deliver``.  The envelope is the array ``loudness_oracle.peaks`` forms,
the release is the recurrence as it is written, the smoothing one ``numpy.convolve``: nothing here knows about tiles,
aggregates or launches.  Test infrastructure; shared by the CPU and the GPU tests.
"""

import math
from collections import namedtuple

import numpy as np
from scipy.ndimage import maximum_filter1d

import delivery_oracle
import loudness_oracle

Limited = namedtuple("Limited", "out s e max_reduction")
Step = namedtuple("Step", "run pre_gain_db ceiling")
Pipeline = namedtuple("Pipeline", "passes pre_gains_db integrated limited measured gain values max_reduction linear decisions")


def envelope(x, pre_gain):
    """e[m] = g max over the four phases and both channels of the oversampled magnitudes at frame m."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    taps = loudness_oracle.true_peak_taps()
    best = np.zeros(n)
    for c in range(x.shape[1]):
        up = np.zeros(4 * n)
        up[::4] = x[:, c]
        over = np.convolve(up, taps)[24:24 + 4 * n]                      # entry 4 m + p: phase p at frame m
        best = np.maximum(best, np.abs(over).reshape(n, 4).max(axis=1))
    return float(pre_gain) * best


def reduction(e, ceiling):
    """d0: 1 - c / e where e > c, else 0 (a NaN compares false)."""
    d0 = np.zeros(e.shape)
    with np.errstate(invalid="ignore"):
        over = e > ceiling
    d0[over] = 1.0 - ceiling / e[over]
    return d0


def release(d, rho):
    q = np.empty(d.shape)
    last = 0.0
    for m, value in enumerate(d.tolist()):
        last = max(value, rho * last)
        q[m] = last
    return q


def weights(lookahead):
    k = np.arange(-lookahead, lookahead + 1)
    return (lookahead + 1 - np.abs(k)) / float((lookahead + 1) ** 2)


def smoothing(q, lookahead, clamp=True):
    """s[m] = sum w[k] q[clamp(m + k)]; ``clamp=False`` pads with zeros instead (what the definition does NOT do)."""
    padded = np.pad(q, lookahead, mode="edge" if clamp else "constant")
    return np.convolve(padded, weights(lookahead), mode="valid")


def limit(x, pre_gain, ceiling, lookahead, release_frames, clamp=True):
    """mgx_tp_limit of x[n][2] float32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.shape[0]
    if n == 0:
        return Limited(x.copy(), np.zeros(0), np.zeros(0), 0.0)
    e = envelope(x, pre_gain)
    d0 = reduction(e, float(ceiling))
    d = maximum_filter1d(d0, size=2 * lookahead + 1, mode="constant", cval=0.0)
    rho = math.exp(-1.0 / release_frames) if release_frames > 0 else 0.0
    s = smoothing(release(d, rho), lookahead, clamp)
    out = ((x.astype(np.float64) * float(pre_gain)) * (1.0 - s)[:, None]).astype(np.float32)
    return Limited(out, s, e, float(s.max()))


def tolerance(x, pre_gain, want):
    """Per sample, what a float32 d0 plane allows an implementation: 2^-25 on the gain, doubled, and half a float32
    spacing of the oracle's value for the store's rounding."""
    x = np.asarray(x, dtype=np.float64)
    return 2.0 ** -24 * np.abs(x * float(pre_gain)) + 0.5 * np.spacing(np.abs(np.asarray(want, dtype=np.float32))).astype(np.float64)


def room(ceiling_dbtp, bits, kind):
    """The numerator of mgx_delivery_gain's g_peak."""
    margin = 0.0 if bits == 0 else delivery_oracle.interpolator_gain() * delivery_oracle.quantiser_error(bits, kind) / 2.0 ** (bits - 1)
    return 10.0 ** (ceiling_dbtp / 20.0) - margin


def limit_step(target, ceiling, bits, kind, integrated0, true_peak0, pre_gains_db, integrated, max_passes, tolerance_lu):
    """mgx_delivery_limit_step: ``pre_gains_db`` / ``integrated`` of the passes run so far."""
    linear = delivery_oracle.delivery_gain(target, ceiling, bits, kind, integrated0, true_peak0)
    c = room(ceiling, bits, kind)
    passes = len(pre_gains_db)
    has_target = target is not None and not math.isnan(target) and math.isfinite(integrated0)
    if passes == 0:
        if linear.limited_by != 2:
            return Step(False, 0.0, c)
        return Step(True, target - integrated0 if has_target else 0.0, c)
    p, loud = pre_gains_db[-1], integrated[-1]
    if not has_target or target - loud <= tolerance_lu or passes == max_passes or math.isinf(loud):
        return Step(False, p, c)
    slope = 1.0
    if passes >= 2:
        dp, dl = p - pre_gains_db[-2], loud - integrated[-2]
        if dp == 0.0 or not dl / dp >= 0.1:
            return Step(False, p, c)
        slope = min(dl / dp, 1.0)
    return Step(True, p + (target - loud) / slope, c)


def stop_margin(target, tolerance_lu, integrated):
    """Smallest distance in LU of a pass's remaining shortfall from ``tolerance_lu``: how far every stop-or-go decision
    that compares the two sat from the threshold."""
    return min((abs((target - loud) - tolerance_lu) for loud in integrated), default=math.inf)


def pipeline(x, rate, target, ceiling, bits, kind, seed, lookahead, release_frames, max_passes, tolerance_lu, measured=None):
    """A delivery with a limiter, from the rendering x[n][2] float32 to the integer values (or float32 samples) of the
    file.  ``measured``: the rendering's measurement where the caller has it already."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    first = loudness_oracle.measure(x, rate) if measured is None else measured
    linear = delivery_oracle.delivery_gain(target, ceiling, bits, kind, first.integrated, first.true_peak)
    pre, loud, frames, reading, worst = [], [], x, first, 0.0
    while True:
        step = limit_step(target, ceiling, bits, kind, first.integrated, first.true_peak, pre, loud, max_passes, tolerance_lu)
        if not step.run:
            break
        result = limit(x, 10.0 ** (step.pre_gain_db / 20.0), step.ceiling, lookahead, release_frames)
        frames, worst = result.out, result.max_reduction
        reading = loudness_oracle.measure(frames, rate)
        pre.append(step.pre_gain_db)
        loud.append(reading.integrated)
    gain = delivery_oracle.delivery_gain(target, ceiling, bits, kind, reading.integrated, reading.true_peak) if pre else linear
    values = delivery_oracle.deliver(frames, gain.gain, bits, kind, seed)
    return Pipeline(len(pre), pre, loud, frames, reading, gain, values, worst, linear,
                    stop_margin(target, tolerance_lu, loud) if target is not None else math.inf)
