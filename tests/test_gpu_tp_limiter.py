"""The deliveries' true-peak limiter on the MI355X: ``mgx_tp_limit`` against tests/tp_limiter_oracle.py at the edges of its
tiles, look-aheads and releases, the release carried across many workgroups, identity, determinism and refusals; and a
delivery that carries a limiter through ``stages.main`` / ``process`` / ``process_batch`` on the 3-second synthetic pair:
the device's passes are the oracle pipeline's on the downloaded rendering, the written file holds its ceiling and its
predicted loudness as the oracle's meter reads it back, and falls less short of the target than the linear delivery.
The signals and the oracle's answers are tests/tp_limiter_cases.py's, shared with the CPU suite.
"""

import ctypes

import numpy as np
import pytest

import delivery_oracle
import loudness_oracle
import matchering_amd as mg
import tp_limiter_cases as cases
import tp_limiter_oracle as oracle
from matchering_amd import _native, audio_io, stages
from matchering_amd.delivery import Delivery, DeliveryRequest, TruePeakLimiter, delivery_gain
from matchering_amd.synth import make_pair

pytestmark = pytest.mark.gpu

RATE = 44100


@pytest.fixture(scope="module")
def dev():
    from matchering_amd.device import default_device

    return default_device()


def limited(dev, x, pre_gain, ceiling, lookahead, release):
    """(frames, max_reduction) of one call on frames uploaded for it."""
    n = x.shape[0]
    with dev.lock:
        buf = dev.upload(x)
        out = None
        try:
            out, worst = dev.tp_limit(buf, n, pre_gain, ceiling, lookahead, release)
            return dev.download(out, (n, 2)), worst
        finally:
            buf.release()
            if out is not None:
                out.release()


@pytest.mark.parametrize("lookahead", cases.LOOKAHEADS)
def test_device_against_the_oracle_at_the_edges(dev, lookahead):
    """Per sample 2^-24 |g x| + half a float32 spacing of the oracle's value (tp_limiter_oracle.tolerance)."""
    worst = 0.0
    for n in cases.edge_sizes(lookahead):
        for release in cases.RELEASES:
            x, want = cases.edge_case(n, lookahead, release)
            got, reduction = limited(dev, x, cases.PRE_GAIN, cases.CEILING, lookahead, release)
            ok, ratio = cases.within(got, x, cases.PRE_GAIN, want.out)
            worst = max(worst, ratio)
            assert ok, (n, lookahead, release, ratio)
            assert abs(reduction - want.max_reduction) <= 2.0 ** -24, (n, lookahead, release)
    print("look-ahead", lookahead, "largest error / tolerance:", worst)


def test_the_release_is_carried_across_many_workgroups(dev):
    x, want = cases.carry_case()
    c = cases.CARRY
    got, reduction = limited(dev, x, c["pre_gain"], c["ceiling"], c["lookahead"], c["release"])
    ok, ratio = cases.within(got, x, c["pre_gain"], want.out)
    print("largest error / tolerance:", ratio)
    assert ok, ratio
    assert want.s[5 * cases.TILE] > 1e3 * 2.0 ** -24 and want.s[-1] < 2.0 ** -24     # eleven tiles of recovery to see
    loud = np.abs(x[:, 0]) > 1e-3
    gain = got[loud, 0].astype(np.float64) / (c["pre_gain"] * x[loud, 0].astype(np.float64))
    assert np.abs(gain - (1.0 - want.s[loud])).max() <= 2.0 ** -23                   # (a float32 quotient: 2^-24 of its own on top)
    assert abs(reduction - want.max_reduction) <= 2.0 ** -24


def test_identity_below_the_ceiling_and_determinism(dev):
    for n in (1, 513, cases.TILE + 5):
        x = cases.quiet_signal(n)
        got, reduction = limited(dev, x, 1.7, 0.5, 66, 2205)
        assert reduction == 0.0
        assert got.tobytes() == (x.astype(np.float64) * 1.7).astype(np.float32).tobytes()
    x, _ = cases.edge_case(2 * cases.TILE + 3, 66, 2205)
    first, a = limited(dev, x, cases.PRE_GAIN, cases.CEILING, 66, 2205)
    second, b = limited(dev, x, cases.PRE_GAIN, cases.CEILING, 66, 2205)
    assert first.tobytes() == second.tobytes() and a == b and a > 0.0


def test_refusals_leave_the_handle_usable(dev):
    lib = _native.library()
    n = 700
    x, want = cases.edge_case(n, 8, 32)
    with dev.lock:
        buf, out = dev.upload(x), dev.alloc(n * 8)
        try:
            def call(handle=dev.handle, x_ptr=buf.ptr, frames=n, pre_gain=cases.PRE_GAIN, ceiling=cases.CEILING, lookahead=8,
                     release=32.0, out_ptr=out.ptr, worst=None):
                return lib.mgx_tp_limit(handle, ctypes.c_void_p(x_ptr), frames, pre_gain, ceiling, lookahead, release,
                                        ctypes.c_void_p(out_ptr), worst)

            refused = [call(handle=None), call(x_ptr=None), call(out_ptr=None), call(frames=-1), call(out_ptr=buf.ptr),
                       call(out_ptr=buf.ptr + 8 * (n - 1)), call(x_ptr=buf.ptr + 4), call(out_ptr=out.ptr + 4),
                       call(pre_gain=0.0), call(pre_gain=float("nan")), call(ceiling=-0.5), call(ceiling=float("inf")),
                       call(lookahead=0), call(lookahead=2049), call(release=-1.0), call(release=float("nan")),
                       call(release=2.0 ** 22 + 1.0)]
            assert refused == [_native.ERR_ARGUMENT] * len(refused)
            assert lib.mgx_last_error()
            assert call(frames=0) == 0                                       # nothing to do: a success
            worst = ctypes.c_double(-1.0)
            assert call(worst=ctypes.byref(worst)) == 0
            got = dev.download(out, (n, 2))
            assert cases.within(got, x, cases.PRE_GAIN, want.out)[0] and abs(worst.value - want.max_reduction) <= 2.0 ** -24
        finally:
            buf.release()
            out.release()


# ---- a delivery with a limiter through stages.main, process and process_batch ------------------------------------------------
# The 3-second pair's unlimited rendering measures about -6.0 LUFS with a true peak of 1.76: under -1 dBTP linear gain
# reaches -11.9 LUFS.  Three LU above that the limiter's second pass lands 0.04 LU short -- 0.06 LU inside the tolerance,
# the first 0.1 LU outside it; the limited rendering is dense already (a sample-peak limiter made it): there the search
# ends on its slope rule.  Both are figures of the oracle's pipeline on oracle/mastering_oracle.py's renderings; the
# test computes its own from the device's.
LIMITER = TruePeakLimiter()
CEILING_DB = -1.0
BOOST = 3.0
PLAN = {"open.wav": (1, "PCM_16", "tpdf_hp", 2 ** 40 + 3), "dense.wav": (0, "PCM_24", None, 0)}


@pytest.fixture(scope="module")
def pair():
    return make_pair(3.0)


@pytest.fixture(scope="module")
def mastered(dev, pair):
    """The renderings, and per delivery of PLAN: the linear delivery's record at a target far out of reach, from which the
    test takes the loudness linear gain reaches."""
    target, reference = pair
    request = DeliveryRequest([(name, slot, subtype, Delivery(loudness=0.0, true_peak=CEILING_DB, dither=dither, seed=seed))
                               for name, (slot, subtype, dither, seed) in PLAN.items()])
    renderings = stages.main(target, reference, mg.Config(), True, True, False, device=dev, deliveries=request)
    return renderings, request


def specs(mastered, limiter=LIMITER):
    _, linear = mastered
    return {name: Delivery(loudness=linear.delivered[name].achieved_lufs + BOOST, true_peak=CEILING_DB, dither=dither, seed=seed,
                           limiter=limiter)
            for name, (slot, subtype, dither, seed) in PLAN.items()}


def read_back(array, bits):
    if array.dtype.kind in "iu":
        array = delivery_oracle.decoded(delivery_oracle.unpacked(array.tobytes(), bits, array.nbytes * 8 // bits).reshape(-1, 2), bits)
    return loudness_oracle.measure(np.asarray(array, dtype=np.float64), RATE)


def check_record(name, record, array, spec, want):
    from dataclasses import replace

    bits = int(PLAN[name][1][4:])
    linear = delivery_gain(replace(spec, limiter=None), bits, record.measured)            # the same target without the limiter
    measured = read_back(array, bits)
    print(name, record, "| oracle:", want.passes, want.pre_gains_db, want.integrated, "margin", want.decisions, "| read back:",
          measured.integrated, "LUFS, true peak", measured.true_peak)
    # every stop decision of the oracle sits clear of the tolerance: the device's 1e-6 LU cannot turn one
    assert want.decisions >= 0.02, name
    assert record.limiter_passes == want.passes >= 2 and record.bits == bits and record.delivery == spec
    # (the device's limited frames are the oracle's to 2^-24 of each sample: 5e-7 LU at the very most on a loudness; the
    #  secant step multiplies that by 1 / slope + (T - I) / (slope^2 dp), some 50 on the dense rendering)
    assert abs(record.pre_gain_db - want.pre_gains_db[-1]) <= 1e-4, name
    assert abs(record.limited.integrated - want.integrated[-1]) <= 1e-4 and abs(record.gain - want.gain.gain) <= 1e-6 * want.gain.gain
    assert abs(record.max_reduction_db - 20.0 * np.log10(1.0 - want.max_reduction)) <= 1e-4
    assert record.measured.true_peak > 10.0 ** (CEILING_DB / 20.0)
    # the written file: under the ceiling, at the record's loudness (test_gpu_delivery.py's tolerances)
    assert measured.true_peak <= 10.0 ** (CEILING_DB / 20.0) * (1.0 + 1e-9), name
    assert abs(measured.integrated - record.achieved_lufs) <= 0.01, name
    assert abs(spec.loudness - record.shortfall_lu - record.achieved_lufs) < 1e-9
    assert abs(linear.shortfall_lu - BOOST) <= 1e-9 and record.shortfall_lu < linear.shortfall_lu, name
    return measured


def test_main_limits_where_the_ceiling_binds(dev, pair, mastered):
    target, reference = pair
    renderings, _ = mastered
    spec = specs(mastered)
    request = DeliveryRequest([(name, PLAN[name][0], PLAN[name][1], spec[name]) for name in PLAN])
    seen = []
    again = stages.main(target, reference, mg.Config(), True, True, False, device=dev, deliveries=request,
                        loudness=lambda name, value: seen.append((name, value)))
    assert all(np.array_equal(a, b) for a, b in zip(again[:2], renderings[:2]))          # the renderings are not touched
    assert [name for name, _ in seen][-2:] == ["delivered:open.wav", "delivered:dense.wav"]
    assert seen[-2][1] is request.delivered["open.wav"]
    for name, (slot, subtype, dither, seed) in PLAN.items():
        bits = int(subtype[4:])
        record = request.delivered[name]
        want = oracle.pipeline(renderings[slot], RATE, spec[name].loudness, CEILING_DB, bits, dither, seed,
                               *LIMITER.frames(RATE), LIMITER.max_passes, LIMITER.tolerance_lu)
        check_record(name, record, request.arrays[name], spec[name], want)
        assert "limited in" in str(record)
        # the file's values are the oracle's deliver of the oracle's limited frames, as far as the limiter's own tolerance
        # lets them be: that tolerance in LSB after the trim, and one more for a rounding it turns
        values = delivery_oracle.unpacked(request.arrays[name].tobytes(), bits, 2 * target.shape[0]).reshape(-1, 2)
        slack = oracle.tolerance(renderings[slot], 10.0 ** (want.pre_gains_db[-1] / 20.0), want.limited)
        assert np.all(np.abs(values - want.values) <= np.ceil(slack * want.gain.gain * 2.0 ** (bits - 1)) + 1), name
    assert request.delivered["open.wav"].shortfall_lu < LIMITER.tolerance_lu             # the search converged here ...
    assert request.delivered["dense.wav"].limiter_passes < LIMITER.max_passes           # ... and gave up there, before max_passes


def test_the_same_bytes_where_the_ceiling_does_not_bind(dev, pair, mastered):
    target, reference = pair
    renderings, _ = mastered
    quiet = dict(loudness=-20.0, true_peak=CEILING_DB, dither="tpdf", seed=11)
    request = DeliveryRequest([("with", 1, "PCM_16", Delivery(limiter=LIMITER, **quiet)), ("without", 1, "PCM_16", Delivery(**quiet))])
    stages.main(target, reference, mg.Config(), False, True, False, device=dev, deliveries=request)
    assert request.arrays["with"].tobytes() == request.arrays["without"].tobytes()
    assert request.delivered["with"].limiter_passes == 0 and request.delivered["with"].limited_by == "loudness"
    assert request.delivered["with"].gain == request.delivered["without"].gain


def test_process_and_a_batch_job_write_the_same_limited_file(dev, pair, mastered, tmp_path):
    target, reference = pair
    spec = specs(mastered)["open.wav"]
    audio_io.save(str(tmp_path / "target.wav"), target, RATE, "FLOAT")
    audio_io.save(str(tmp_path / "reference.wav"), reference, RATE, "FLOAT")
    one, two = str(tmp_path / "process.wav"), str(tmp_path / "batch.wav")
    records = {}
    mg.process(str(tmp_path / "target.wav"), str(tmp_path / "reference.wav"),
               [mg.Result(one, "PCM_16", use_limiter=False, normalize=False, delivery=spec)],
               loudness=lambda name, value: records.__setitem__(name, value))
    record = records["delivered:" + one]
    assert record.limiter_passes >= 2 and record.shortfall_lu < LIMITER.tolerance_lu
    got, rate = audio_io.read_wav(one)
    measured = loudness_oracle.measure(np.asarray(got, dtype=np.float64), RATE)
    assert rate == RATE and measured.true_peak <= 10.0 ** (CEILING_DB / 20.0) * (1.0 + 1e-9)
    assert abs(measured.integrated - record.achieved_lufs) <= 0.01
    # a batch job names the limiter in its JSON form
    job = {"target": str(tmp_path / "target.wav"), "reference": str(tmp_path / "reference.wav"),
           "results": [{"file": two, "subtype": "PCM_16", "use_limiter": False, "normalize": False,
                        "delivery": {"loudness": spec.loudness, "true_peak": CEILING_DB, "dither": "tpdf_hp", "seed": 2 ** 40 + 3,
                                     "limiter": True}}]}
    import json

    from matchering_amd import batch

    with open(tmp_path / "jobs.json", "w") as fh:
        json.dump([job], fh)
    jobs = batch.jobs_from_json(str(tmp_path / "jobs.json"))
    assert jobs[0]["results"][0].delivery == spec
    done = mg.process_batch(jobs, rank=0, world_size=1, lanes=1)
    assert done == [0]
    assert open(one, "rb").read() == open(two, "rb").read()
