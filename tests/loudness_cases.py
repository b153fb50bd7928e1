"""Signals, launch geometry and the bounds shared by tests/test_loudness_host.py (the kernel's phases on the CPU) and
tests/test_gpu_loudness.py (mgx_loudness on the GPU): both run the same shapes against tests/loudness_oracle.py at the
same bounds.  Test infrastructure.
"""

import functools
import math

import numpy as np

import loudness_oracle as oracle

RATES = (8000, 11025, 44100, 48000, 96000, 192000)
TILE, OWN_MAX, WORKGROUPS = 4096, 12, 400          # loudness_plan.h: LOUD_TILE, LOUD_OWN, LOUD_WORKGROUPS


def state_matrix(rate):
    """A of z' = A z + B x, z = (s1, s2, t1, t2) (loudness_plan.h), in extended precision."""
    (b, a), (c, d) = oracle.k_weighting(rate)
    m = np.zeros((4, 4), dtype=np.longdouble)
    m[0, 0], m[0, 1], m[1, 0] = -a[1], 1.0, -a[2]
    m[2, 0], m[2, 2], m[2, 3] = np.longdouble(c[1]) - np.longdouble(d[1]) * c[0], -d[1], 1.0
    m[3, 0], m[3, 2] = np.longdouble(c[2]) - np.longdouble(d[2]) * c[0], -d[2]
    return m


def warmup_poles(rate):
    """ceil(ln 1e-12 / ln rho), rho the largest pole modulus of the two biquads."""
    rho = 0.0
    for _, a in oracle.k_weighting(rate):
        rho = max(rho, float(np.abs(np.roots(a)).max()))
    return int(math.ceil(math.log(1e-12) / math.log(rho)))


@functools.lru_cache(maxsize=None)
def warmup(rate):
    """H: the first k >= warmup_poles at which the largest row sum of |A^k| is at most 1e-12 (loudness_design)."""
    a, least = state_matrix(rate), warmup_poles(rate)
    power, k = np.eye(4, dtype=np.longdouble), 0
    while True:
        power, k = power @ a, k + 1
        if k >= least and np.abs(power).sum(axis=1).max() <= np.longdouble(1e-12):
            return k


def geometry(rate, n):
    """(S, nsub, H, own, workgroups) as loudness_geometry (loudness_plan.cpp) decides them."""
    size = oracle.sub_block_frames(rate)
    nsub = n // size
    own = min(OWN_MAX, max(1, -(-nsub // WORKGROUPS)))
    return size, nsub, warmup(rate), own, max(1, -(-nsub // own))


def workgroup_start(rate, n, wg):
    """First frame workgroup ``wg`` reads (loud_range, loudness_kernel.h): its first sub-block less the warm-up, moved
    back until its last tile ends where its range ends, not below 0.  Its tiles begin every TILE frames from there."""
    size, nsub, h, own, workgroups = geometry(rate, n)
    begin = wg * own * size
    end = n if wg == workgroups - 1 else min((wg + 1) * own, nsub) * size
    latest = max(0, begin - h)
    return max(0, end - -(-(end - latest) // TILE) * TILE)


def zero_slack_length(rate, subs):
    """(n, first frame of the last workgroup's sub-blocks) for a length of ``subs`` whole sub-blocks or a few more and a
    rest chosen so that the LAST workgroup's tiles begin exactly H frames ahead of its first sub-block: the warm-up
    with nothing to spare, where H alone has to do."""
    size, h = oracle.sub_block_frames(rate), warmup(rate)
    for count in range(subs, subs + 64):
        own = geometry(rate, count * size)[3]
        begin = (-(-count // own) - 1) * own * size
        n = count * size + (begin - h - count * size) % TILE
        if n // size == count:
            assert workgroup_start(rate, n, geometry(rate, n)[4] - 1) == begin - h, (rate, count, n)
            return n, begin
    raise AssertionError((rate, subs))


def lengths(rate):
    """The frame counts every rate is run at: around one sub-block, around the first momentary block, around the first
    short-term block -- with one sub-block per workgroup here: 1, 4, 30 workgroups, each but the first two with a
    warm-up that is clipped at frame 0 or reaches over its neighbours."""
    size = oracle.sub_block_frames(rate)
    return [1, size - 1, size, size + 1, 4 * size - 1, 4 * size, 30 * size, 30 * size + 1]


def noise(n, seed, level=0.3, dc=0.0):
    rng = np.random.RandomState(seed)
    return (level * rng.randn(n, 2) + dc).astype(np.float32)


def noise_dc_step(rate, n, step_at, seed=3):
    """Seeded noise plus a DC offset of 0.2, the whole of it 60 dB down from frame ``step_at`` on: the longest transient
    a warm-up has to forget."""
    x = noise(n, seed, 0.3, 0.2).astype(np.float64)
    x[step_at:] *= 1e-3
    return x.astype(np.float32)


def impulses(n, at):
    x = np.zeros((n, 2), dtype=np.float32)
    for k, frame in enumerate(at):
        x[frame, k % 2] = 1.0 if k % 3 else -1.0
    return x


def sine(rate, seconds, dbfs, freq=1000.0, phase=0.0):
    t = np.arange(int(round(seconds * rate)))
    return (10.0 ** (dbfs / 20.0)) * np.sin(2.0 * np.pi * freq * t / rate + phase)


def stereo(mono):
    return np.ascontiguousarray(np.repeat(np.asarray(mono, dtype=np.float32)[:, None], 2, axis=1))


def segments(rate, parts):
    """[(seconds, dBFS), ...] of a 1 kHz stereo sine, phase running on across the joins (EBU Tech 3341 / 3342)."""
    gains = np.concatenate([np.full(int(round(s * rate)), 10.0 ** (db / 20.0)) for s, db in parts])
    t = np.arange(len(gains))
    return stereo(gains * np.sin(2.0 * np.pi * 1000.0 * t / rate))


# (signal, which field, required value, tolerance below, tolerance above): EBU Tech 3341 cases 1-5, Tech 3342 cases 1-3
KNOWN = [
    ("3341-1", [(20, -23)], "integrated", -23.0, 0.1, 0.1),
    ("3341-2", [(20, -33)], "integrated", -33.0, 0.1, 0.1),
    ("3341-3", [(10, -36), (60, -23), (10, -36)], "integrated", -23.0, 0.1, 0.1),
    ("3341-4", [(10, -72), (10, -36), (60, -23), (10, -36), (10, -72)], "integrated", -23.0, 0.1, 0.1),
    ("3341-5", [(20, -26), (20.1, -20), (20, -26)], "integrated", -23.0, 0.1, 0.1),
    ("3342-1", [(20, -20), (20, -30)], "range", 10.0, 1.0, 1.0),
    ("3342-2", [(20, -20), (20, -15)], "range", 5.0, 1.0, 1.0),
    ("3342-3", [(20, -40), (20, -20)], "range", 20.0, 1.0, 1.0),
]


def faded_sine(rate, freq, degrees, amplitude):
    """1 s of a sine with 10 ms linear fades: the true-peak signals of Tech 3341 (cases 15-19 in spirit)."""
    n = rate
    x = amplitude * np.sin(2.0 * np.pi * freq * np.arange(n) / rate + math.radians(degrees))
    fade = int(0.010 * rate)
    ramp = np.linspace(0.0, 1.0, fade)
    x[:fade] *= ramp
    x[-fade:] *= ramp[::-1]
    return stereo(x)


# (frequency as a fraction of the rate, phase in degrees, amplitude, required dBTP, below, above)
TRUE_PEAKS = [(1 / 4, 0.0, 0.5, -6.0, 0.4, 0.2), (1 / 4, 45.0, 0.5, -6.0, 0.4, 0.2), (1 / 6, 60.0, 0.5, -6.0, 0.4, 0.2),
              (1 / 8, 67.5, 0.5, -6.0, 0.4, 0.2), (1 / 4, 45.0, 1.41, 3.0, 0.4, 0.2)]


def assert_measured(x, rate, energy, fields, true_peak, sample_peak, label=""):
    """The bounds of both suites.  Sub-block energies within 1e-9 max(e, 1e-12 S): the warm-up truncates at 1e-12 of the
    state, float64 sums over at most 19200 terms add about 1e-13.  The four loudness fields within 1e-8 LU, which follows
    (10 log10(1 + 1e-9) = 4e-9) PROVIDED no block changes sides of a gate: asserted first, on the oracle, as a condition.
    The peaks within 1e-12 relative (twelve float64 products in another order)."""
    want = oracle.measure(x, rate)
    size = oracle.sub_block_frames(rate)
    margin = oracle.gate_margin(want.sub_energy, rate)
    assert margin > 1e-6, f"{label}: a block lies {margin:.2e} LU from a gate: the signal does not test what it should"
    energy = np.asarray(energy).reshape(-1, 2)
    assert energy.shape == want.sub_energy.shape, (label, energy.shape, want.sub_energy.shape)
    worst = 0.0
    if energy.size:
        worst = float((np.abs(energy - want.sub_energy) / np.maximum(want.sub_energy, 1e-12 * size)).max())
    names = ("integrated", "range", "momentary_max", "short_term_max")
    field_worst = 0.0
    for name, got, expected in zip(names, fields, want[:4]):
        assert not math.isnan(got), (label, name)
        if math.isinf(expected):
            assert got == expected, (label, name, got, expected)
        else:
            field_worst = max(field_worst, abs(got - expected))
    peak_worst = max(abs(true_peak - want.true_peak) / max(want.true_peak, 1e-300),
                     abs(sample_peak - want.sample_peak) / max(want.sample_peak, 1e-300))
    print(f"{label}: {energy.shape[0]} sub-blocks, energy {worst:.2e} (1e-9), loudness {field_worst:.2e} LU (1e-8), "
          f"peaks {peak_worst:.2e} (1e-12), nearest gate {margin:.2e} LU")
    assert worst <= 1e-9, (label, worst)
    assert field_worst <= 1e-8, (label, field_worst)
    assert peak_worst <= 1e-12, (label, peak_worst)
    return want
