"""The clip repair's definition (include/mgx.h, mgx_declip) as literal float64 loops in numpy, counters included: what
the kernel's phase functions (tests/test_declip_emu.py) and the kernel (tests/test_gpu_declip.py) are held to bit for
bit.  Test infrastructure."""
import numpy as np

FIELDS = ("runs_repaired", "samples_repaired", "samples_raised", "longest_repaired", "first_repaired", "runs_short",
          "runs_long", "runs_edge", "peak_before", "peak_after")
MAX_RUN = 512


def _classes(x, level):
    """+1 high, -1 low, 0 neither, per sample of one channel (float32)."""
    xd = x.astype(np.float64)
    finite = np.isfinite(x)
    with np.errstate(invalid="ignore"):
        return np.where(finite & (xd >= level), 1, np.where(finite & (xd <= -level), -1, 0)).astype(np.int8)


def _peak(x):
    finite = np.isfinite(x)
    return float(np.max(np.abs(x[finite]).astype(np.float64))) if finite.any() else 0.0


def declip_channel(x, level, min_run=2, max_run=32, max_rise=2.0, cap=True):
    """One channel: (out float32, dict of the report's fields).  ``cap=False`` leaves max_rise out (for readings only)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.size
    level, max_rise = float(level), float(max_rise)
    ceiling = max_rise * level
    cls = _classes(x, level)
    out = x.copy()
    rep = dict(runs_repaired=0, samples_repaired=0, samples_raised=0, longest_repaired=0, first_repaired=-1, runs_short=0,
               runs_long=0, runs_edge=0)
    i = 0
    while i < n:
        c = int(cls[i])
        if c == 0:
            i += 1
            continue
        a = i
        while i < n and cls[i] == c:
            i += 1
        b = i
        r = b - a
        if r < min_run:
            rep["runs_short"] += 1
            continue
        if r > max_run:
            rep["runs_long"] += 1
            continue
        if a < 2 or b + 1 > n - 1 or not all(np.isfinite(x[j]) for j in (a - 2, a - 1, b, b + 1)):
            rep["runs_edge"] += 1
            continue
        rep["runs_repaired"] += 1
        rep["samples_repaired"] += r
        rep["longest_repaired"] = max(rep["longest_repaired"], r)
        if rep["first_repaired"] < 0:
            rep["first_repaired"] = a
        h = float(r + 1)
        p0, p1 = float(x[a - 1]), float(x[b])
        m0 = h * (p0 - float(x[a - 2]))
        m1 = h * (float(x[b + 1]) - p1)
        for k in range(1, r + 1):
            j = a - 1 + k
            xd = float(x[j])
            t = k / h
            t2 = t * t
            t3 = t2 * t
            y = ((2 * t3 - 3 * t2 + 1) * p0 + (t3 - 2 * t2 + t) * m0) + ((3 * t2 - 2 * t3) * p1 + (t3 - t2) * m1)
            if c > 0:
                if cap and y > ceiling:
                    y = ceiling
                if y > xd:
                    with np.errstate(over="ignore"):
                        out[j] = np.float32(y)
            else:
                if cap and y < -ceiling:
                    y = -ceiling
                if y < xd:
                    with np.errstate(over="ignore"):
                        out[j] = np.float32(y)
    rep["samples_raised"] = int(np.count_nonzero(out.view(np.uint32) != x.view(np.uint32)))
    rep["peak_before"] = _peak(x)
    rep["peak_after"] = _peak(out)
    return out, rep


def declip(frames, level, min_run=2, max_run=32, max_rise=2.0, cap=True):
    """(n, 2) float32 -> (out (n, 2) float32, report): every field of the report a (left, right) tuple."""
    frames = np.ascontiguousarray(frames, dtype=np.float32).reshape(-1, 2)
    out = np.empty_like(frames)
    reps = []
    for c in range(2):
        out[:, c], rep = declip_channel(frames[:, c], level, min_run, max_run, max_rise, cap)
        reps.append(rep)
    return out, {k: (reps[0][k], reps[1][k]) for k in FIELDS}


# ---- tracks with the border cases the tests share ---------------------------------------------------------------------
def quiet(n, seed=0, scale=0.3):
    """(n, 2) float32 noise well under any level the tests use."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-scale, scale, (n, 2))).astype(np.float32)


def put_run(x, channel, a, b, value):
    """Samples [a, b) of a channel at ``value`` (clipped to the track)."""
    a, b = max(a, 0), min(b, x.shape[0])
    if b > a:
        x[a:b, channel] = value
    return x


def random_track(n, seed, level=0.8, density=0.02, longest=40, nonfinite=0):
    """Noise with runs of random length and sign at random places in both channels (some adjacent), and a few samples
    that are not finite."""
    rng = np.random.default_rng(seed)
    x = quiet(n, seed + 1000, 0.75)
    if n == 0:
        return x
    for c in range(2):
        for _ in range(max(1, int(n * density / 4))):
            a = int(rng.integers(0, n))
            r = int(rng.integers(1, longest + 1))
            sign = 1.0 if rng.random() < 0.5 else -1.0
            put_run(x, c, a, a + r, np.float32(sign * level * (1.0 + 0.1 * rng.random())))
            if rng.random() < 0.3:
                r2 = int(rng.integers(1, longest + 1))
                put_run(x, c, a + r, a + r + r2, np.float32(-sign * level))
    for _ in range(nonfinite):
        x[int(rng.integers(0, n)), int(rng.integers(0, 2))] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32))
    return x


def adjacent(a, r, tail=3):
    """A run of r samples at frame a in both channels, a run of the other sign touching it: in the left channel a high
    run with a low one of ``tail`` samples behind it, in the right a low run with a high one in front of it."""
    return [(0, a, r, 1), (0, a + r, tail, -1), (1, a, r, -1), (1, a - tail, tail, 1)]


def track_with(n, runs, level=0.8, seed=7):
    """Quiet noise with the runs (channel, first frame, length, sign) put at ``level``."""
    x = quiet(n, seed)
    for c, a, r, sign in runs:
        put_run(x, c, a, a + r, np.float32(sign * level))
    return x


def border_cases(S, max_run, min_run=2):
    """name -> (n, runs): the placements around the border at frame S that a segment-by-segment evaluation can get
    wrong, and the track's ends."""
    n = 2 * S + 517
    cases = {
        "ends_at_border": adjacent(S - 4, 4),
        "starts_at_border": adjacent(S, 4),
        "starts_behind_border": adjacent(S + 1, 4),
        "spans_border": adjacent(S - 6, 12),
        "max_run_across": adjacent(S - max_run // 2, max_run),
        "max_run_plus_one_across": adjacent(S - max_run // 2, max_run + 1),
        "max_run_from_last_frame": adjacent(S - 1, max_run),
        "max_run_to_first_frame": adjacent(S + 1 - max_run, max_run),
        "min_run": adjacent(S - 1, min_run, tail=min_run),
        "track_ends": [(0, 0, 3, 1), (1, 1, 3, -1), (0, n - 3, 3, -1), (1, n - 4, 3, 1)],
        "second_frame_and_last_but_one": [(0, 2, 3, 1), (1, 2, 4, -1), (0, n - 5, 3, 1), (1, n - 6, 4, -1)],
    }
    if min_run > 1:
        cases["min_run_less_one"] = adjacent(S - 1, min_run - 1, tail=min_run - 1)
    return {name: (n, runs) for name, runs in cases.items()}

