"""The audit without a GPU: ``mgx_audit_gate`` through the real libmgx.so against the windowing of tests/audit_oracle.py
on hand-made sub-block sums, what it refuses, ``AuditLimits`` and ``Audit.findings``, and the run monoid of
csrc/audit_kernel.h folded on the host (tests/emu/emu_audit.cpp) in random associations against the oracle's run
lengths; its stand-alone program under the sanitizers.
"""

import ctypes
import math
import subprocess

import numpy as np
import pytest

import audit_emu
import audit_oracle as oracle
import emu_build
from matchering_amd import _native
from matchering_amd.qc import Audit, AuditLimits, from_report

RATE = 48000
B = 4800


def gate(sub_sums, n, rate=RATE, sums=None):
    """mgx_audit_gate of the real library: the report, its sums taken from the sub-block sums unless given."""
    lib = _native.library()
    sub = np.ascontiguousarray(sub_sums, dtype=np.float64).reshape(-1, 3)
    report = _native.MgxAuditReport()
    total = sub.sum(axis=0) if sums is None else sums
    report.sumsq[0], report.sumsq[1], report.sum_lr = (float(v) for v in total)
    report.clip_events[1] = 7                                       # a measured field: not this call's
    rc = lib.mgx_audit_gate(sub.ctypes.data_as(_native.c_double_p), sub.shape[0], n, rate, ctypes.byref(report))
    assert rc == 0, lib.mgx_last_error()
    assert report.frames == n and report.sub_blocks == sub.shape[0] and report.sub_block_frames == (rate + 5) // 10
    assert report.clip_events[1] == 7
    return report


def same(a, b, rel=1e-12):
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= rel * abs(b)


def against_oracle(sub, n, rate=RATE):
    sub = np.asarray(sub, dtype=np.float64).reshape(-1, 3)
    total = sub.sum(axis=0)
    report = gate(sub, n, rate)
    want = oracle.gate(sub, n, rate, (0.0, 0.0), (total[0], total[1]), total[2])
    assert report.correlation_min_at == want["correlation_min_at"]
    for name in ("balance_db", "correlation", "mono_loss_db", "correlation_min"):
        assert same(getattr(report, name), want[name]), (name, getattr(report, name), want[name])
    return report


def noise_sums(count, seed, level=0.01):
    rng = np.random.default_rng(seed)
    ll, rr = level * (0.5 + rng.random(count)), level * (0.5 + rng.random(count))
    return np.stack([ll * B, rr * B, (rng.random(count) - 0.5) * np.sqrt(ll * rr) * B], axis=1)


# ---- the gate rule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 7, 29, 30, 31, 64])
def test_gate_windows_against_the_oracle(count):
    """fewer than 30 sub-blocks (one window of all of them), exactly 30 (one window), more (hop of one)"""
    for seed in range(3):
        sub = noise_sums(count, seed)
        report = against_oracle(sub, count * B)
        assert 0 <= report.correlation_min_at <= max(0, count - 30)
    # a last, partial sub-block: n implies its length
    sub = noise_sums(count, 9)
    against_oracle(sub, (count - 1) * B + 17)


def test_gate_skips_a_quiet_window_and_answers_nan_when_all_are():
    sub = noise_sums(70, 1)
    sub[:, 2] = 0.5 * np.sqrt(sub[:, 0] * sub[:, 1])
    sub[:35] *= 1e-9                                                # -110 dB: every window inside the quiet half is skipped
    sub[:35, 2] *= -1.0                                             # ... although its correlation would be the least
    report = against_oracle(sub, 70 * B)
    assert report.correlation_min_at > 5 and report.correlation_min > -0.49
    report = against_oracle(sub[:35], 35 * B)
    assert math.isnan(report.correlation_min) and report.correlation_min_at == -1
    # a channel whose window sum is zero is skipped too
    sub = noise_sums(40, 2)
    sub[:, 1] = 0.0
    sub[:, 2] = 0.0
    report = against_oracle(sub, 40 * B)
    assert math.isnan(report.correlation_min) and report.correlation_min_at == -1
    assert math.isnan(report.correlation) and math.isnan(report.balance_db)


def test_gate_finds_an_anti_phase_second_half():
    sub = np.zeros((90, 3))
    sub[:, 0] = sub[:, 1] = 48.0                                    # (every partial sum is exact)
    sub[:45, 2] = 48.0                                              # L = R
    sub[45:, 2] = -48.0                                             # L = -R
    report = against_oracle(sub, 90 * B)
    assert report.correlation_min == -1.0 and report.correlation_min_at == 45      # the first window wholly in anti-phase
    assert report.correlation == 0.0


def test_gate_mono_loss_at_the_extremes():
    sub = np.full((10, 3), 0.02 * B)                                # L = R
    report = gate(sub, 10 * B)
    assert report.mono_loss_db == 0.0 and report.correlation == 1.0 and report.balance_db == 0.0
    sub[:, 2] *= -1.0                                               # L = -R
    report = gate(sub, 10 * B)
    assert report.mono_loss_db == -math.inf and report.correlation == -1.0
    empty = gate(np.zeros((0, 3)), 0)
    assert all(math.isnan(v) for v in (empty.dc[0], empty.rms[1], empty.balance_db, empty.correlation, empty.mono_loss_db,
                                       empty.correlation_min)) and empty.correlation_min_at == -1


def test_gate_dc_and_rms():
    report = gate(noise_sums(3, 4), 3 * B, sums=(2.0, 8.0, 0.0))
    report.sum[0], report.sum[1] = 3.0, -6.0
    lib = _native.library()
    sub = noise_sums(3, 4)
    assert lib.mgx_audit_gate(sub.ctypes.data_as(_native.c_double_p), 3, 3 * B, RATE, ctypes.byref(report)) == 0
    assert report.dc[0] == 3.0 / (3 * B) and report.dc[1] == -6.0 / (3 * B)
    assert report.rms[0] == math.sqrt(2.0 / (3 * B)) and report.rms[1] == math.sqrt(8.0 / (3 * B))


def test_gate_refusals():
    lib = _native.library()
    sub = noise_sums(3, 5)
    ptr = sub.ctypes.data_as(_native.c_double_p)
    report = _native.MgxAuditReport()
    for args, word in (((ptr, 3, 3 * B, RATE, None), "report"),
                       ((ptr, -1, 3 * B, RATE, ctypes.byref(report)), "count"),
                       ((ptr, 3, -1, RATE, ctypes.byref(report)), "n_frames"),
                       ((None, 3, 3 * B, RATE, ctypes.byref(report)), "sub_sums"),
                       ((ptr, 3, 3 * B, 7999, ctypes.byref(report)), "sample_rate"),
                       ((ptr, 3, 3 * B + 1, RATE, ctypes.byref(report)), "count"),
                       ((ptr, 2, 3 * B, RATE, ctypes.byref(report)), "count")):
        assert lib.mgx_audit_gate(*args) == _native.ERR_ARGUMENT, word
        assert lib.mgx_last_error().decode().startswith(word + ":"), (word, lib.mgx_last_error())
    assert lib.mgx_audit_gate(ptr, 3, 3 * B - 1, RATE, ctypes.byref(report)) == 0       # a partial last sub-block


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_audit_limits_validation():
    limits = AuditLimits()
    assert limits.clip_level == 1 - 2 ** -15 and limits.clip_run == 3 and limits.silence_db == -90.0
    assert abs(limits.silence_level - 10 ** -4.5) < 1e-20
    assert AuditLimits(silence_db=-math.inf).silence_level == 0.0
    native = AuditLimits(0.5, 2, -60.0).native()
    assert (native.clip_level, native.clip_run) == (0.5, 2) and abs(native.silence_level - 1e-3) < 1e-18
    for bad in (dict(clip_level=0.0), dict(clip_level=-1.0), dict(clip_level=math.inf), dict(clip_level=math.nan),
                dict(clip_run=0), dict(clip_run=1.5), dict(silence_db=math.nan), dict(silence_db=math.inf)):
        with pytest.raises(ValueError):
            AuditLimits(**bad)
    with pytest.raises(Exception):
        limits.clip_run = 4                                         # frozen


def constructed(**changes):
    report = _native.MgxAuditReport()
    report.frames, report.sub_block_frames, report.sub_blocks = 96000, 4800, 20
    report.clip_first[0] = report.clip_first[1] = report.gap_at = report.correlation_min_at = -1
    report.peak[0] = report.peak[1] = 0.5
    report.dc[0], report.dc[1] = 1e-5, -1e-5
    report.correlation = report.correlation_min = 0.8
    report.correlation_min_at = 0
    for name, value in changes.items():
        if isinstance(value, tuple):
            for c in range(2):
                getattr(report, name)[c] = value[c]
        else:
            setattr(report, name, value)
    return from_report(report, 48000)


def test_findings_on_constructed_reports():
    clean = constructed()
    assert isinstance(clean, Audit) and clean.findings() == []
    assert clean.duration_s == 2.0 and clean.gap_at_s is None and clean.clip_first_s == (None, None)
    assert clean.peak_db == (20 * math.log10(0.5),) * 2 and abs(clean.dc_db[1] + 100.0) < 1e-9
    assert len(str(clean).splitlines()) in (2, 3)
    assert constructed(nonfinite=(0, 2)).findings() == [("nonfinite", 2, 0)]
    assert constructed(clip_events=(1, 2), clip_samples=(3, 9), clip_longest=(3, 5), clip_first=(10, 4800)).findings() == \
        [("clipping", 3, 0)]
    assert constructed(clip_longest=(2, 2)).findings() == []        # runs under clip_run are no events
    found = constructed(dc=(0.0, -0.01)).findings()
    assert [f[0] for f in found] == ["dc_offset"] and abs(found[0][1] + 40.0) < 1e-9 and found[0][2] == -60.0
    assert constructed(dc=(0.0, -0.01)).findings(dc_db=-30.0) == []
    assert constructed(correlation_min=-0.25, correlation_min_at=12).findings() == [("out_of_phase", -0.25, 0.0)]
    assert constructed(correlation_min=-0.25, correlation_min_at=12).correlation_min_at_s == 1.2
    assert constructed(correlation_min=math.nan, correlation_min_at=-1).findings() == []
    gap = constructed(gap_longest=4800, gap_at=24000)
    assert gap.findings() == [("dropout", 0.1, 0.05)] and gap.gap_at_s == 0.5 and gap.findings(gap_s=0.1) == []
    quiet = constructed(head_silence=48000, tail_silence=24000)
    assert quiet.findings() == [] and quiet.findings(head_s=0.5, tail_s=0.5) == [("head_silence", 1.0, 0.5)]
    assert quiet.findings(tail_s=0.25) == [("tail_silence", 0.5, 0.25)]
    every = constructed(nonfinite=(1, 0), clip_events=(1, 0), dc=(0.5, 0.0), correlation_min=-1.0, gap_longest=48000)
    assert [f[0] for f in every.findings(head_s=0.0)] == ["nonfinite", "clipping", "dc_offset", "out_of_phase", "dropout"]
    assert every.as_dict()["nonfinite"] == [1, 0] and every.as_dict()["sample_rate"] == 48000


# ---- the run monoid ----------------------------------------------------------------------------------------------------
def folded(pieces, min_run, rng):
    """The records of consecutive pieces folded in a random association."""
    while len(pieces) > 1:
        i = int(rng.integers(len(pieces) - 1))
        pieces[i:i + 2] = [audit_emu.combine(pieces[i], pieces[i + 1], min_run)]
    return pieces[0]


def test_run_monoid_in_any_association():
    """A few hundred seeded predicate sequences of length <= 64, cut at random places (empty and length-1 pieces
    included), each piece a record, the records folded in a random association: events, samples, longest and first as
    the oracle's run lengths give them, and the silence fields from the unfinished total."""
    rng = np.random.default_rng(20261021)
    cases = 0
    for case in range(400):
        n = int(rng.integers(0, 65))
        density = (0.1, 0.5, 0.9, 1.0, 0.0)[case % 5]
        p = rng.random(n) < density
        min_run = int(rng.integers(1, 5))
        cuts = sorted(int(c) for c in rng.integers(0, n + 1, size=int(rng.integers(0, 9))))
        if case % 3 == 0 and n:
            cuts = sorted(cuts + [cuts[0] if cuts else 0, min(n, (cuts[0] if cuts else 0) + 1)])   # an empty and a length-1 piece
        edges = [0] + cuts + [n]
        pieces = [audit_emu.leaf(p[a:b], a, min_run) for a, b in zip(edges[:-1], edges[1:])]
        total = folded(pieces, min_run, rng)
        whole = audit_emu.fields(audit_emu.leaf(p, 0, min_run))
        assert audit_emu.fields(total) == whole, (case, p, cuts)
        done = audit_emu.finish(total, min_run)
        assert (done["events"], done["samples"], done["best"], done["first"]) == oracle.clip_fields(p, min_run), (case, p, cuts)
        raw = audit_emu.fields(total)
        if n:
            assert (raw["prefix"], raw["suffix"], raw["best"], raw["best_at"]) == oracle.silence_fields(p), (case, p, cuts)
        cases += 1
    assert cases == 400


def test_run_monoid_ties_and_borders():
    """Of equal runs the earliest wins, wherever the cuts fall; a run across a border is one run."""
    p = np.array([0, 1, 1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 1, 1, 0], dtype=bool)
    for cut in range(len(p) + 1):
        for cut2 in range(cut, len(p) + 1):
            pieces = [audit_emu.leaf(p[:cut], 0, 2), audit_emu.leaf(p[cut:cut2], cut, 2), audit_emu.leaf(p[cut2:], cut2, 2)]
            left = audit_emu.combine(audit_emu.combine(pieces[0], pieces[1], 2), pieces[2], 2)
            right = audit_emu.combine(pieces[0], audit_emu.combine(pieces[1], pieces[2], 2), 2)
            assert audit_emu.fields(left) == audit_emu.fields(right)
            done = audit_emu.finish(left, 2)
            assert (done["events"], done["samples"], done["best"], done["best_at"], done["first"]) == (4, 10, 3, 8, 1)


def test_kernel_constants():
    c = audit_emu.constants()
    assert c["segment"] == c["threads"] * c["run"] == 4096
    assert c["segment"] % 4410 and c["segment"] % 4800               # deliberately no multiple of a sub-block
    assert c["subs_max"] == c["segment"] // 800 + 2 and c["merge_threads"] % 64 == 0


def test_standalone_monoid_program_under_sanitizers(tmp_path):
    out = str(tmp_path / "emu_audit_driver")
    emu_build.build_driver(audit_emu.NAME, out, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    done = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip() == "ok", done.stdout + done.stderr
