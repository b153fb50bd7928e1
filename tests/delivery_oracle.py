"""Float64 numpy restatement of the delivery renditions (include/mgx.h: mgx_delivery_gain, mgx_deliver): the gain rule, the
Philox4x32-10 generator on ``uint64`` words, the two dithers and the quantiser.  Nothing here knows about quads, grids or
packing beyond the byte order of a 24-bit sample.  Test infrastructure; shared by the CPU and the GPU tests.
"""

import math
from collections import namedtuple

import numpy as np

import loudness_oracle

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
DITHERS = {None: 0, "tpdf": 1, "tpdf_hp": 2}

Gain = namedtuple("Gain", "gain achieved_lufs achieved_true_peak shortfall_lu limited_by")


def philox(counter, key):
    """Philox4x32-10 with Python integers: four counter words, two key words -> four output words."""
    c0, c1, c2, c3 = (int(v) & MASK for v in counter)
    k0, k1 = (int(v) & MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_blocks(quads, stream, seed):
    """Output words of blocks q = 0 .. quads - 1 of ``stream``: uint64 array (quads, 4), vectorised over q."""
    q = np.arange(quads, dtype=np.uint64)
    mask = np.uint64(MASK)
    c0, c1 = q & mask, q >> np.uint64(32)
    c2, c3 = np.full(quads, stream, dtype=np.uint64), np.zeros(quads, dtype=np.uint64)
    k0, k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                   # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & mask,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & mask)
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3], axis=1)


def uniform(samples, stream, seed):
    """U(s, stream) for s = 0 .. samples - 1: ((W >> 8) + 0.5) 2^-24 - 0.5, float64, inside (-1/2, 1/2)."""
    words = philox_blocks((samples + 3) // 4, stream, seed).reshape(-1)[:samples]
    return ((words >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24 - 0.5


def dither(samples, kind, seed):
    """d(s): ``kind`` 0 / None none, 1 / "tpdf", 2 / "tpdf_hp"."""
    kind = DITHERS.get(kind, kind)
    if kind == 0:
        return np.zeros(samples)
    u = uniform(samples, 0, seed)
    if kind == 1:
        return u + uniform(samples, 1, seed)
    before = np.zeros(samples)
    before[2:] = u[:-2]                                                   # the same channel one frame earlier; 0 before the track
    return u - before


def deliver(x, gain, bits, kind=0, seed=0):
    """mgx_deliver of interleaved float32 samples ``x`` (any shape, C order): float32 for bits 0, else the integer values
    as int64 in x's shape."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    flat = x.reshape(-1).astype(np.float64)
    if bits == 0:
        return (flat * float(gain)).astype(np.float32).reshape(x.shape)
    top = float(2 ** (bits - 1) - 1)
    a = (flat * float(gain)) * top
    v = np.clip(np.rint(a + dither(flat.size, kind, seed)), -top - 1.0, top)
    return v.astype(np.int64).reshape(x.shape)


def packed(values, bits):
    """The bytes of a file of that width, little-endian: what the device writes."""
    values = np.asarray(values).reshape(-1)
    if bits == 0:
        return values.astype("<f4").tobytes()
    if bits == 16:
        return values.astype("<i2").tobytes()
    if bits == 32:
        return values.astype("<i4").tobytes()
    return (values.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()


def unpacked(raw, bits, samples):
    """Integer values (int64) or float32 samples of ``samples`` samples from the device's bytes."""
    raw = np.frombuffer(bytes(raw), dtype=np.uint8)
    if bits == 0:
        return raw[:4 * samples].view("<f4").copy()
    if bits == 16:
        return raw[:2 * samples].view("<i2").astype(np.int64)
    if bits == 32:
        return raw[:4 * samples].view("<i4").astype(np.int64)
    b = raw[:3 * samples].reshape(-1, 3).astype(np.int64)
    v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    return v - ((v >> 23) << 24)


def decoded(values, bits):
    """What a reader (and the meter) makes of the file: v / 2^(bits-1); float output as it is."""
    values = np.asarray(values)
    return values.astype(np.float64) if bits == 0 else values.astype(np.float64) / float(2 ** (bits - 1))


def interpolator_gain():
    """A: the largest per-phase sum of the meter's absolute oversampling taps."""
    taps = np.abs(loudness_oracle.true_peak_taps())
    return max(float(taps[p::4].sum()) for p in range(4))


def quantiser_error(bits, kind):
    """e: the most that dither and rounding add to a sample, in LSB."""
    return 0.0 if bits == 0 else (1.5 if DITHERS.get(kind, kind) else 0.5)


def delivery_gain(target, ceiling, bits, kind, integrated, true_peak):
    """mgx_delivery_gain: ``target`` in LUFS and ``ceiling`` in dBTP, None or NaN for "not asked for"."""
    target = math.nan if target is None else float(target)
    ceiling = math.nan if ceiling is None else float(ceiling)
    kind = DITHERS.get(kind, kind)
    if bits not in (0, 16, 24, 32):
        raise ValueError("bits")
    if kind not in (0, 1, 2) or (kind and bits in (0, 32)):
        raise ValueError("dither")
    if math.isinf(target):
        raise ValueError("target_lufs")
    if math.isinf(ceiling) or ceiling > 0.0:
        raise ValueError("ceiling_dbtp")
    if not math.isfinite(true_peak) or true_peak < 0.0:
        raise ValueError("true_peak")
    if math.isnan(integrated) or integrated == math.inf:
        raise ValueError("integrated")
    has_loud = not math.isnan(target) and math.isfinite(integrated)
    g_loud = 10.0 ** ((target - integrated) / 20.0) if has_loud else 1.0
    g_peak = math.inf
    if not math.isnan(ceiling):
        margin = 0.0 if bits == 0 else interpolator_gain() * quantiser_error(bits, kind) / 2.0 ** (bits - 1)
        room = 10.0 ** (ceiling / 20.0) - margin
        if not room > 0.0:
            raise ValueError("ceiling_dbtp")
        if true_peak > 0.0:
            g_peak = room / true_peak
    gain = min(g_loud, g_peak)
    by_peak = g_peak < g_loud
    return Gain(gain, integrated + 20.0 * math.log10(gain) if math.isfinite(integrated) else -math.inf, gain * true_peak,
                20.0 * math.log10(g_loud / gain) if by_peak and has_loud else 0.0, 2 if by_peak else (1 if has_loud else 0))
