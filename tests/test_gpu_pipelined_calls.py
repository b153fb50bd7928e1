"""Pipelined master calls: the front half of call k + 1 on the handle's front stream under the back half
of call k.  Every comparison is ``np.array_equal`` against the same calls on a handle that does not pipeline: one
context, one stream, the library as it was.  Pairs of 1-6 s at 44.1 kHz, default limiter; ``fft_size`` 4096 runs
``k_conv_wide``, 1024 is a quick second route.  No test forces a device-side wait to expire.

A handle pipelines only while it is its device's only live handle, and that is also how the tests get their reference
(the library's set of environment switches is fixed by tests/test_abi.py, so there is none for this): the reference
handle runs the scenario while an idle sibling handle is alive, the pipelined one runs it alone.  A pytest process keeps
other handles alive (the default device, the batch lanes), so every scenario runs in a child process of its own -- this
file, run as a script with the scenario's name.
"""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

SECONDS = {"A": 4.0, "B": 5.0, "C": 3.0, "short": 1.0, "long": 6.0}


class Address:
    """A raw device address where ``Device.master`` takes a buffer (``mgx_last_fir``'s pointer)."""

    def __init__(self, ptr):
        self.ptr = ptr


def native(fft_size=4096):
    import matchering_amd as mg

    return mg.Config(fft_size=fft_size, max_piece_size=1.0).to_native()


def resident(dev, pairs, names):
    """name -> (target buffer, frames, reference buffer, frames), uploaded and waited for."""
    out = {}
    for name in names:
        target, reference = pairs[name]
        out[name] = (dev.upload(target), target.shape[0], dev.upload(reference), reference.shape[0])
    dev.synchronize()
    return out


# ---- the scenarios: (dev, pairs) -> a list of arrays; check_<name>(arrays) looks at the pipelined handle's --------------
def six_buffers(dev, pairs, fft_size=4096):
    """Six calls over three pairs (A, B, C, A, B, C), queued without a synchronisation into six output buffers."""
    r = resident(dev, pairs, "ABC")
    cfg = native(fft_size)
    outs = []
    for k in range(6):
        t, n, ref, nr = r["ABC"[k % 3]]
        outs.append((dev.alloc(n * 8), n))
        dev.master(t, n, ref, nr, cfg, result=outs[-1][0], want_report=False)
    dev.synchronize()
    return [dev.download(o, (n, 2)) for o, n in outs]


def six_buffers_1024(dev, pairs):
    return six_buffers(dev, pairs, 1024)


def check_six_buffers(got):
    for k in range(3):
        assert np.array_equal(got[k], got[k + 3]) and np.abs(got[k]).max() > 0.1


check_six_buffers_1024 = check_six_buffers


def one_buffer(dev, pairs):
    """The same six calls into ONE output buffer, as bench.py does: it holds the last call's result."""
    r = resident(dev, pairs, "ABC")
    cfg = native()
    out = dev.alloc(max(v[1] for v in r.values()) * 8)
    for k in range(6):
        t, n, ref, nr = r["ABC"[k % 3]]
        dev.master(t, n, ref, nr, cfg, result=out, want_report=False)
    return [dev.download(out, (r["C"][1], 2))]


def result_is_next_target(dev, pairs):
    """The alias rule: call k + 1 reads what call k writes."""
    r = resident(dev, pairs, "AB")
    cfg = native()
    t, n, ref, nr = r["A"]
    first, second, third = dev.alloc(n * 8), dev.alloc(n * 8), dev.alloc(n * 8)
    dev.master(t, n, ref, nr, cfg, result=first, want_report=False)
    dev.master(first, n, r["B"][2], r["B"][3], cfg, result=second, want_report=False)
    dev.master(second, n, first, n, cfg, result=third, want_report=False)         # ... and the one before as the reference
    return [dev.download(b, (n, 2)) for b in (first, second, third)]


def upload_between_calls(dev, pairs):
    """RAW: the second call reads the audio uploaded behind the first; WAR: that upload does not overtake the first
    call's reads."""
    from matchering_amd._native import library
    from matchering_amd.device import pinned

    r = resident(dev, pairs, "A")
    cfg = native()
    t, n, ref, nr = r["A"]
    host = pinned.empty((n, 2), np.float32)
    host[:] = pairs["B"][0][:n]
    outs = [dev.alloc(n * 8) for _ in range(3)]
    dev.master(t, n, ref, nr, cfg, result=outs[0], want_report=False)
    assert library().mgx_memcpy_h2d_async(dev.handle, ctypes.c_void_p(t.ptr), host.ctypes.data_as(ctypes.c_void_p),
                                          host.nbytes) == 0
    dev.master(t, n, ref, nr, cfg, result=outs[1], want_report=False)
    dev.master(t, n, ref, nr, cfg, result=outs[2], want_report=False)
    dev.synchronize()
    return [dev.download(o, (n, 2)) for o in outs]


def check_upload_between_calls(got):
    assert not np.array_equal(got[0], got[1]) and np.array_equal(got[1], got[2])


def interleaved_routes(dev, pairs):
    """Pair route, profile route and mgx_master_with_fir (fir_given a buffer of the caller's, and mgx_last_fir's own
    pointer); limiter on and result_no_limiter only; fft_size 4096, 1024, 4096."""
    import matchering_amd as mg
    from matchering_amd.profile import ReferenceProfile

    r = resident(dev, pairs, "ABC")
    cfg = {f: native(f) for f in (4096, 1024)}
    profiles = {f: ReferenceProfile.analyze(pairs["B"][1], mg.Config(fft_size=f, max_piece_size=1.0), device=dev).resident(dev)
                for f in (4096, 1024)}
    outs = []

    def out(n):
        outs.append((dev.alloc(n * 8), n))
        return outs[-1][0]

    ta, na, ra, nra = r["A"]
    tb, nb, rb, nrb = r["B"]
    tc, nc, rc, nrc = r["C"]
    dev.master(ta, na, ra, nra, cfg[4096], result=out(na), want_report=False)
    dev.master(tb, nb, None, 0, cfg[4096], result=out(nb), want_report=False, profile=profiles[4096])
    dev.master(tc, nc, rc, nrc, cfg[1024], result=None, result_no_limiter=out(nc), want_report=False)
    dev.master(ta, na, None, 0, cfg[1024], result=out(na), want_report=False, profile=profiles[1024])
    dev.master(tb, nb, rb, nrb, cfg[4096], result=out(nb), result_no_limiter=out(nb), want_report=False)
    ptr, taps = dev.last_fir()
    assert taps == 4096
    dev.master(tc, nc, rc, nrc, cfg[4096], result=out(nc), want_report=False, fir=Address(ptr))
    dev.master(ta, na, ra, nra, cfg[4096], result=None, result_no_limiter=out(na), want_report=False, fir=Address(ptr))
    fir = dev.download(Address(ptr), (2, 4096))             # a FIR pair of the caller's: the last one, copied out
    dev.master(ta, na, ra, nra, cfg[4096], result=out(na), want_report=False)
    dev.master(tb, nb, rb, nrb, cfg[4096], result=out(nb), want_report=False, fir=dev.upload(fir))
    dev.master(tc, nc, rc, nrc, cfg[4096], result=out(nc), want_report=False)
    dev.synchronize()
    return [fir] + [dev.download(o, (n, 2)) for o, n in outs]


def regrow(dev, pairs):
    """1 s, 6 s, 1 s, 6 s on a fresh handle: its buffers are freed and allocated again while calls are in flight on two
    streams."""
    r = resident(dev, pairs, ["short", "long"])
    cfg = native()
    outs = []
    for name in ("short", "long", "short", "long"):
        t, n, ref, nr = r[name]
        outs.append((dev.alloc(n * 8), n))
        dev.master(t, n, ref, nr, cfg, result=outs[-1][0], want_report=False)
    return [dev.download(o, (n, 2)) for o, n in outs]


def check_regrow(got):
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[3])


def stage_timing(dev, pairs):
    """Stage timing on for the middle calls of a sequence; the last array holds their stage times."""
    r = resident(dev, pairs, "AB")
    cfg = native()
    outs, times = [], []
    for k in range(6):
        t, n, ref, nr = r["AB"[k % 2]]
        outs.append((dev.alloc(n * 8), n))
        if k == 2:
            dev.stage_timing(True)
        dev.master(t, n, ref, nr, cfg, result=outs[-1][0], want_report=False)
        if k in (2, 3):
            row = dev.stage_times()
            for stage in ("analyze", "design_fir", "filter_spectra", "convolve", "correct_levels", "limit"):
                assert row[stage] is not None and row[stage] > 0.0, row
            assert all(v is None or v > 0.0 for v in row.values()), row
            times.append(row)
        if k == 3:
            dev.stage_timing(False)
    assert len(times) == 2
    return [dev.download(o, (n, 2)) for o, n in outs]


def nan_in_third_of_five(dev, pairs):
    """A NaN in call 3 of 5: the next blocking call fails with MGX_ERR_ARGUMENT as ever; the handle masters correctly
    afterwards; and mgx_last_fir and a report behind a pipelined sequence describe the last call."""
    from matchering_amd._native import ERR_ARGUMENT, MgxError

    r = resident(dev, pairs, "AB")
    cfg = native()
    t, n, ref, nr = r["A"]
    bad = np.array(pairs["A"][0])
    bad[n // 2, 1] = np.nan
    bad_dev = dev.upload(bad)
    out = dev.alloc(max(n, r["B"][1]) * 8)
    for k in range(5):
        dev.master(bad_dev if k == 2 else t, n, ref, nr, cfg, result=out, want_report=False)
    with pytest.raises(MgxError, match="not finite") as caught:
        dev.synchronize()
    assert caught.value.code == ERR_ARGUMENT
    dev.master(t, n, ref, nr, cfg, result=out, want_report=False)
    good = dev.download(out, (n, 2))
    tb, nb, rb, nrb = r["B"]
    dev.master(t, n, ref, nr, cfg, result=out, want_report=False)
    dev.master(tb, nb, rb, nrb, cfg, result=out, want_report=False)
    ptr, taps = dev.last_fir()
    fir_b = dev.download(Address(ptr), (2, taps))
    report = dev.master(tb, nb, rb, nrb, cfg, result=out, want_report=True)
    ptr, taps = dev.last_fir()
    fir_b_again = dev.download(Address(ptr), (2, taps))
    numbers = np.array([report.target_match_rms, report.reference_match_rms, report.rms_coefficient, report.result_peak,
                        report.target_divisions, report.reference_divisions, report.limiter_active]
                       + list(report.correction_coefficients))
    return [good, fir_b, fir_b_again, numbers, dev.download(out, (nb, 2))]


def check_nan_in_third_of_five(got):
    assert np.isfinite(got[0]).all() and np.array_equal(got[1], got[2])
    assert got[3][4] >= 1 and np.abs(got[1]).max() > 0


SCENARIOS = [six_buffers, six_buffers_1024, one_buffer, result_is_next_target, upload_between_calls, interleaved_routes,
             regrow, stage_timing, nan_in_third_of_five]


def takes_contexts_in_turn(dev, pairs):
    """Whether ``dev`` pipelines, by the one thing the ABI shows of it: consecutive pipelined calls design their FIRs into
    the handle's two contexts in turn, so mgx_last_fir's address changes from one call to the next; calls on main alone
    stay in one context."""
    r = resident(dev, pairs, "C")
    t, n, ref, nr = r["C"]
    out = dev.alloc(n * 8)
    seen = []
    for _ in range(3):
        dev.master(t, n, ref, nr, native(), result=out, want_report=False)
        seen.append(dev.last_fir()[0])
    dev.synchronize()
    return seen[0] != seen[1] and seen[1] != seen[2] and seen[0] == seen[2]


def child(name):
    """The reference handle beside an idle sibling (it stays on its one stream), then the pipelined handle alone."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from matchering_amd.device import Device
    from matchering_amd.synth import make_pair

    scenario = globals()[name]
    pairs = {key: make_pair(s, 44100, pair=3 + k, reference_seconds=s * 0.9) for k, (key, s) in enumerate(SECONDS.items())}
    results = []
    for alone in (False, True):
        sibling = None if alone else Device(0)
        dev = Device(0)
        results.append(scenario(dev, pairs))
        # (without this every comparison below could hold trivially, between two handles that both stayed on main)
        assert takes_contexts_in_turn(dev, pairs) == alone, "the handle that is alone must pipeline, the other must not"
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
    print("PIPELINED EQUALS SERIAL", name, len(got))


@pytest.mark.gpu
@pytest.mark.parametrize("scenario", [s.__name__ for s in SCENARIOS])
def test_pipelined_calls_equal_serial_calls(scenario):
    done = subprocess.run([sys.executable, os.path.abspath(__file__), scenario], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    assert f"PIPELINED EQUALS SERIAL {scenario}" in done.stdout


if __name__ == "__main__":
    child(sys.argv[1])
