"""The audit's definitions (include/mgx.h, mgx_audit) in plain numpy float64: run lengths by ``np.diff`` on the
predicate, ``math.fsum`` for the sums.  The yardstick of tests/test_audit_host.py and tests/test_gpu_audit.py; the
reference project has nothing of the kind, so there is no golden file."""
import math

import numpy as np

WINDOW = 30                     # sub-blocks of a correlation window
QUIET = 1e-7                    # mean power below which a window is skipped: 10^(-70 / 10)


def values(x, bits):
    """(n, 2) float64 values of float32 frames (bits 0) or of file PCM: int16, int32 (n, 2), packed 24-bit uint8 (n, 6)."""
    x = np.asarray(x)
    if bits == 0:
        return x.astype(np.float32).astype(np.float64).reshape(-1, 2)
    if bits == 24:
        b = x.reshape(-1, 3).astype(np.int64)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        return (v.astype(np.float64) / float(1 << 23)).reshape(-1, 2)
    return x.astype(np.float64).reshape(-1, 2) / float(1 << (bits - 1))


def runs(predicate):
    """[(start, length)] of the maximal runs of True."""
    p = np.concatenate(([0], np.asarray(predicate, dtype=np.int8), [0]))
    edges = np.diff(p)
    starts, ends = np.flatnonzero(edges == 1), np.flatnonzero(edges == -1)
    return [(int(s), int(e - s)) for s, e in zip(starts, ends)]


def clip_fields(predicate, clip_run):
    """(events, samples, longest, first) of one channel's at-rail predicate."""
    found = runs(predicate)
    events = [(s, n) for s, n in found if n >= clip_run]
    return (len(events), sum(n for _, n in events), max((n for _, n in found), default=0),
            events[0][0] if events else -1)


def silence_fields(silent):
    """(head, tail, gap_longest, gap_at) of the silent-frame predicate."""
    n = len(silent)
    loud = np.flatnonzero(~np.asarray(silent, dtype=bool))
    if loud.size == 0:
        return n, n, 0, -1
    first, last = int(loud[0]), int(loud[-1])
    inner = [(s, m) for s, m in runs(silent) if s > first and s + m - 1 < last]
    longest, at = 0, -1
    for s, m in inner:
        if m > longest:
            longest, at = m, s
    return first, n - 1 - last, longest, at


def sub_block_frames(rate):
    return (rate + 5) // 10


def _ratio(a, b):
    return a / b if b != 0.0 else math.nan


def _log10(v):
    return math.log10(v) if v > 0.0 else -math.inf


def gate(sub_sums, n, rate, total, sumsq, sum_lr):
    """mgx_audit_gate: the derived figures from the report's sums and the (count, 3) sub-block sums."""
    B = sub_block_frames(rate)
    ll, rr, lr = sumsq[0], sumsq[1], sum_lr
    out = {
        "dc": tuple(_ratio(total[c], float(n)) for c in range(2)),
        "rms": tuple(math.sqrt(sumsq[c] / n) if n else math.nan for c in range(2)),
        "balance_db": 10.0 * _log10(ll / rr) if rr != 0.0 else math.nan,
        "correlation": _ratio(lr, math.sqrt(ll * rr)),
        "mono_loss_db": 10.0 * _log10(max(ll + rr + 2.0 * lr, 0.0) / (2.0 * (ll + rr))) if ll + rr != 0.0 else math.nan,
    }
    sub_sums = np.asarray(sub_sums, dtype=np.float64).reshape(-1, 3)
    count = sub_sums.shape[0]
    width = min(count, WINDOW)
    least, at = math.nan, -1
    for k in range(count - width + 1 if count else 0):
        s = [math.fsum(sub_sums[k:k + width, c]) for c in range(3)]
        frames = min(n, (k + width) * B) - k * B
        if not (s[0] + s[1]) / (2.0 * frames) >= QUIET or s[0] == 0.0 or s[1] == 0.0:
            continue
        r = s[2] / math.sqrt(s[0] * s[1])
        if at < 0 or r < least:
            least, at = r, k
    out["correlation_min"], out["correlation_min_at"] = least, at
    return out


def audit(x, bits, rate, clip_level=1 - 2 ** -15, clip_run=3, silence_level=10.0 ** (-90.0 / 20.0)):
    """Every field of mgx_audit_report as a dict, plus "sub_sums" (count, 3) and, for the tests' bounds, "terms": for each
    of sum0, sum1, sumsq0, sumsq1, sum_lr the pair (number of terms, sum of their magnitudes), and "sub_terms"
    (count, 3) the sums of the magnitudes of every sub-block sum's terms."""
    v = values(x, bits)
    n = v.shape[0]
    finite = np.isfinite(v)
    z = np.where(finite, v, 0.0)
    mag = np.abs(z)
    rail = finite & (mag >= clip_level)
    silent = finite.all(axis=1) & (mag <= silence_level).all(axis=1)
    ll, rr, lr = z[:, 0] * z[:, 0], z[:, 1] * z[:, 1], z[:, 0] * z[:, 1]
    B = sub_block_frames(rate)
    count = -(-n // B)
    out = {"frames": n, "bits": bits, "sub_blocks": count, "sub_block_frames": B,
           "nonfinite": tuple(int((~finite[:, c]).sum()) for c in range(2)),
           "sum": tuple(math.fsum(z[:, c]) for c in range(2)),
           "sumsq": (math.fsum(ll), math.fsum(rr)), "sum_lr": math.fsum(lr),
           "peak": tuple(float(mag[:, c].max()) if n else 0.0 for c in range(2))}
    clips = [clip_fields(rail[:, c], clip_run) for c in range(2)]
    for i, name in enumerate(("clip_events", "clip_samples", "clip_longest", "clip_first")):
        out[name] = tuple(clips[c][i] for c in range(2))
    out["head_silence"], out["tail_silence"], out["gap_longest"], out["gap_at"] = silence_fields(silent)
    out["sub_sums"] = np.array([[math.fsum(t[k * B:(k + 1) * B]) for t in (ll, rr, lr)] for k in range(count)]).reshape(count, 3)
    out["terms"] = {"sum0": (n, math.fsum(mag[:, 0])), "sum1": (n, math.fsum(mag[:, 1])), "sumsq0": (n, math.fsum(ll)),
                    "sumsq1": (n, math.fsum(rr)), "sum_lr": (n, math.fsum(np.abs(lr)))}
    out["sub_terms"] = np.array([[math.fsum(np.abs(t[k * B:(k + 1) * B])) for t in (ll, rr, lr)]
                                 for k in range(count)]).reshape(count, 3)
    out.update(gate(out["sub_sums"], n, rate, out["sum"], out["sumsq"], out["sum_lr"]))
    return out
