"""A call's context is released behind round 0 of its level correction: the front half of call k + 2
may run while the tail, the scale kernel and the limiter of call k still work, which from round 0 on read and write the
handle's back state alone (csrc/correction_kernels.h, BackState) and nothing of the context.

As in tests/test_gpu_pipelined_calls.py every comparison is ``np.array_equal`` against the same calls on a handle that
does not pipeline (an idle sibling handle is alive beside it), and every scenario runs in a child process of its own:
this file, run as a script with the scenario's name.  Pairs of 1-6 s at 44.1 kHz, ``max_piece_size=1.0``; ``fft_size``
4096 runs ``k_conv_wide``, 1024 is a quick second route.  The pairs differ strongly in level, so that the reference's
match RMS and amplitude coefficient and the correction gain of consecutive calls differ by tens of percent: a scalar
that is stale, or overwritten early by the call after next, changes many samples and not the last bit
(``check_levels_differ`` holds the pairs to that).  No test forces a device-side wait to expire.
"""

import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_pipelined_calls import Address, resident, takes_contexts_in_turn  # noqa: E402

# name -> (seconds, target_gain, reference_gain): from a quiet reference under the threshold (the final-amplitude branch)
# to a hot one that the limiter works on in several percent of the frames
PAIRS = {"long": (6.0, 0.5, 2.5), "long2": (6.0, 0.2, 6.0), "s1": (1.0, 0.15, 0.6), "s2": (1.0, 0.9, 6.0),
         "s3": (1.0, 0.3, 1.2), "A": (4.0, 0.9, 0.5), "B": (5.0, 0.25, 3.0), "C": (3.0, 0.6, 1.2)}


def native(fft_size=4096, steps=4):
    import matchering_amd as mg

    return mg.Config(fft_size=fft_size, max_piece_size=1.0, rms_correction_steps=steps).to_native()


def queue(dev, r, names, cfg, kind="limited"):
    """One call per name, queued without synchronisation, each into buffers of its own.  ``kind``: which outputs."""
    outs = []
    for name in names:
        t, n, ref, nr = r[name]
        bufs = {}
        if kind in ("limited", "both"):
            bufs["result"] = dev.alloc(n * 8)
        if kind in ("unlimited", "both"):
            bufs["result_no_limiter"] = dev.alloc(n * 8)
        if kind == "both":
            bufs["result_no_limiter_normalized"] = dev.alloc(n * 8)
        dev.master(t, n, ref, nr, cfg, want_report=False, **bufs)
        outs += [(b, n) for b in bufs.values()]
    return outs


def fetch(dev, outs):
    dev.synchronize()
    return [dev.download(o, (n, 2)) for o, n in outs]


LONG_SHORT = ["long", "s1", "s2", "s3", "long2", "s3", "s2", "s1"]


# ---- the scenarios: (dev, pairs) -> a list of arrays ------------------------------------------------------------------
def long_then_short(dev, pairs, fft_size=4096):
    """A 6 s call, then 1 s calls: the whole front half of call k + 2 fits under the limiter of call k."""
    r = resident(dev, pairs, set(LONG_SHORT))
    return fetch(dev, queue(dev, r, LONG_SHORT, native(fft_size)))


def long_then_short_1024(dev, pairs):
    return long_then_short(dev, pairs, 1024)


def long_then_short_no_tail(dev, pairs):
    """(the child process of this one runs with MGX_NO_TAIL=1: one launch per correction round)"""
    assert os.environ.get("MGX_NO_TAIL") == "1"
    return long_then_short(dev, pairs)


def short_then_long(dev, pairs):
    r = resident(dev, pairs, set(LONG_SHORT))
    return fetch(dev, queue(dev, r, LONG_SHORT[::-1], native()))


def check_levels_differ(got):
    """The scenarios above: consecutive results differ in level by tens of percent, so a neighbour's scalar would show."""
    rms = [float(np.sqrt(np.mean(np.square(g, dtype=np.float64)))) for g in got]
    assert all(v > 0.01 for v in rms)
    assert sum(abs(a / b - 1.0) > 0.2 for a, b in zip(rms, rms[1:])) >= len(rms) - 3, rms


check_long_then_short = check_long_then_short_1024 = check_long_then_short_no_tail = check_short_then_long = check_levels_differ


def all_routes(dev, pairs):
    """Pair, profile and given FIR in turn, three times round."""
    import matchering_amd as mg
    from matchering_amd.profile import ReferenceProfile

    r = resident(dev, pairs, ["long", "s1", "s2", "A", "B", "C"])
    cfg = native()
    config = mg.Config(fft_size=4096, max_piece_size=1.0)
    profiles = [ReferenceProfile.analyze(pairs[name][1], config, device=dev).resident(dev) for name in ("s2", "B", "long")]
    firs = []
    for name in ("s1", "C"):                                # two FIR pairs of the caller's: designed here, copied out
        t, n, ref, nr = r[name]
        scratch = dev.alloc(n * 8)
        dev.master(t, n, ref, nr, cfg, result=scratch, want_report=False)
        ptr, taps = dev.last_fir()
        firs.append(dev.upload(dev.download(Address(ptr), (2, taps))))
    dev.synchronize()
    outs = []
    for k, names in enumerate([("long", "s1", "s2"), ("A", "s2", "C"), ("s1", "B", "long")]):
        t, n, ref, nr = r[names[0]]
        outs.append((dev.alloc(n * 8), n))
        dev.master(t, n, ref, nr, cfg, result=outs[-1][0], want_report=False)
        t, n, _, _ = r[names[1]]
        outs.append((dev.alloc(n * 8), n))
        dev.master(t, n, None, 0, cfg, result=outs[-1][0], want_report=False, profile=profiles[k])
        t, n, ref, nr = r[names[2]]
        outs.append((dev.alloc(n * 8), n))
        dev.master(t, n, ref, nr, cfg, result=outs[-1][0], want_report=False, fir=firs[k % 2])
    return fetch(dev, outs)


def outputs_limited(dev, pairs):
    r = resident(dev, pairs, set(LONG_SHORT))
    return fetch(dev, queue(dev, r, LONG_SHORT[:6], native(), "limited"))


def outputs_unlimited(dev, pairs):
    r = resident(dev, pairs, set(LONG_SHORT))
    return fetch(dev, queue(dev, r, LONG_SHORT[:6], native(), "unlimited"))


def outputs_both(dev, pairs):
    r = resident(dev, pairs, set(LONG_SHORT))
    return fetch(dev, queue(dev, r, LONG_SHORT[:6], native(), "both"))


def outputs_mixed(dev, pairs):
    """... and the three kinds in turn in one queue."""
    r = resident(dev, pairs, set(LONG_SHORT))
    outs = []
    for k, name in enumerate(LONG_SHORT):
        outs += queue(dev, r, [name], native(), ("limited", "unlimited", "both")[k % 3])
    return fetch(dev, outs)


def steps_0(dev, pairs):
    r = resident(dev, pairs, set(LONG_SHORT))
    return fetch(dev, queue(dev, r, LONG_SHORT[:6], native(steps=0), "both"))


def steps_1(dev, pairs):
    r = resident(dev, pairs, set(LONG_SHORT))
    return fetch(dev, queue(dev, r, LONG_SHORT[:6], native(steps=1), "both"))


def steps_mixed(dev, pairs):
    """0, 1 and 4 rounds in turn in one queue, fft_size 1024: each kind of first launch fills the back state."""
    r = resident(dev, pairs, set(LONG_SHORT))
    outs = []
    for k, name in enumerate(LONG_SHORT):
        outs += queue(dev, r, [name], native(1024, steps=(4, 0, 1)[k % 3]), "both" if k % 2 else "limited")
    return fetch(dev, outs)


def report_after_six(dev, pairs):
    """Six pipelined calls, then a call with a report: its numbers come from the back state."""
    r = resident(dev, pairs, set(LONG_SHORT))
    cfg = native()
    outs = queue(dev, r, LONG_SHORT[:6], cfg)
    t, n, ref, nr = r["s2"]
    outs.append((dev.alloc(n * 8), n))
    normalized = dev.alloc(n * 8)
    report = dev.master(t, n, ref, nr, cfg, result=outs[-1][0], result_no_limiter_normalized=normalized, want_report=True)
    numbers = np.array([report.final_amplitude_coefficient, report.target_match_rms, report.reference_match_rms,
                        report.rms_coefficient, report.normalize_coefficient, report.result_peak, report.limiter_active,
                        report.target_divisions, report.reference_divisions] + list(report.correction_coefficients))
    return [numbers] + fetch(dev, outs + [(normalized, n)])


def check_report_after_six(got):
    numbers = got[0]
    assert np.isfinite(numbers).all() and numbers[5] > 0.5 and numbers[6] == 1      # the hot pair: a peak, a working limiter
    assert np.count_nonzero(numbers[9:]) == 4 and abs(numbers[9] - 1.0) > 1e-6      # four correction coefficients


def output_two_calls_back(dev, pairs):
    """The output of call k as the target of call k + 2, and as the reference of call k + 2."""
    r = resident(dev, pairs, ["A", "B", "C", "s1"])
    cfg = native()
    ta, na, ra, nra = r["A"]
    tb, nb, rb, nrb = r["B"]
    tc, nc, rc, nrc = r["C"]
    ts, ns, rs, nrs = r["s1"]
    outs = [(dev.alloc(na * 8), na), (dev.alloc(ns * 8), ns), (dev.alloc(na * 8), na), (dev.alloc(nb * 8), nb),
            (dev.alloc(nc * 8), nc), (dev.alloc(ns * 8), ns), (dev.alloc(nb * 8), nb)]
    dev.master(ta, na, ra, nra, cfg, result=outs[0][0], want_report=False)                 # 0 (long)
    dev.master(ts, ns, rs, nrs, cfg, result=outs[1][0], want_report=False)                 # 1 (short)
    dev.master(outs[0][0], na, rb, nrb, cfg, result=outs[2][0], want_report=False)         # 2: target = output of 0
    dev.master(tb, nb, rb, nrb, cfg, result=outs[3][0], want_report=False)                 # 3
    dev.master(tc, nc, outs[2][0], na, cfg, result=outs[4][0], want_report=False)          # 4: reference = output of 2
    dev.master(ts, ns, outs[3][0], nb, cfg, result=outs[5][0], want_report=False)          # 5: reference = output of 3
    dev.master(outs[3][0], nb, ra, nra, cfg, result=outs[6][0], want_report=False)         # 6: target = output of 3 (three back)
    return fetch(dev, outs)


def synchronize_in_the_middle(dev, pairs):
    r = resident(dev, pairs, set(LONG_SHORT))
    cfg = native()
    outs = queue(dev, r, LONG_SHORT[:3], cfg)
    dev.synchronize()
    outs += queue(dev, r, LONG_SHORT[3:], cfg)
    return fetch(dev, outs)


SCENARIOS = [long_then_short, long_then_short_1024, long_then_short_no_tail, short_then_long, all_routes, outputs_limited,
             outputs_unlimited, outputs_both, outputs_mixed, steps_0, steps_1, steps_mixed, report_after_six,
             output_two_calls_back, synchronize_in_the_middle]


def child(name):
    """The reference handle beside an idle sibling (it stays on its one stream), then the pipelined handle alone."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from matchering_amd.device import Device
    from matchering_amd.synth import make_pair

    scenario = globals()[name]
    pairs = {key: make_pair(s, 44100, pair=11 + k, reference_seconds=s * 0.9, target_gain=tg, reference_gain=rg)
             for k, (key, (s, tg, rg)) in enumerate(PAIRS.items())}
    results = []
    for alone in (False, True):
        sibling = None if alone else Device(0)
        dev = Device(0)
        results.append(scenario(dev, pairs))
        pipelines = takes_contexts_in_turn(dev, {"C": pairs["C"]})
        assert pipelines == alone, "the handle that is alone must pipeline, the other must not"
        dev.close()
        if sibling is not None:
            sibling.close()
    want, got = results
    assert len(want) == len(got) and len(want) > 0
    for k, (a, b) in enumerate(zip(want, got)):
        assert a.shape == b.shape and np.array_equal(a, b), f"array {k} differs from the handle's that does not pipeline"
    check = globals().get("check_" + name)
    if check:
        check(got)
    print("RELEASED CONTEXT EQUALS SERIAL", name, len(got))


@pytest.mark.gpu
@pytest.mark.parametrize("scenario", [s.__name__ for s in SCENARIOS])
def test_calls_with_an_early_released_context_equal_serial_calls(scenario):
    env = dict(os.environ)
    if scenario.endswith("_no_tail"):
        env["MGX_NO_TAIL"] = "1"
    done = subprocess.run([sys.executable, os.path.abspath(__file__), scenario], capture_output=True, text=True, timeout=300,
                          env=env)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    assert f"RELEASED CONTEXT EQUALS SERIAL {scenario}" in done.stdout


if __name__ == "__main__":
    child(sys.argv[1])
