"""The deliveries' true-peak limiter without a GPU: the frame bound and the identity on the numpy oracle
(tests/tp_limiter_oracle.py), the kernels' phase functions (csrc/tp_limit_kernel.h) driven on the CPU by
tests/emu/libmgx_emu_tp_limit.so against the oracle at the shapes the GPU tests use, the policy ``mgx_delivery_limit_step``
(the real libmgx.so through ctypes) against hand-computed sequences and the oracle, the oracle's pipeline down to the written
file, and the Python surface.
"""

import ctypes
import math
import os
import re

import numpy as np
import pytest

import delivery_oracle
import emu_build
import loudness_oracle
import matchering_amd as mg
import tp_limiter_cases as cases
import tp_limiter_oracle as oracle
from conftest import ROOT
from matchering_amd import _native
from matchering_amd.delivery import Delivered, Delivery, TruePeakLimiter, delivery_gain, limit_step
from matchering_amd.loudness import Loudness
from matchering_amd.synth import synth

P = ctypes.c_void_p
FORMATS = [(0, 0), (16, 0), (16, 1), (16, 2), (24, 0), (24, 1), (24, 2), (32, 0)]      # (bits, dither) that exist
RATE = 44100


@pytest.fixture(scope="module")
def emu():
    lib = emu_build.load("tp_limit")
    lib.emu_tp_limit_constants.argtypes = [ctypes.c_int, P]
    lib.emu_tp_limit.restype = ctypes.c_double
    lib.emu_tp_limit.argtypes = [P, ctypes.c_longlong, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_double, P, P,
                                 ctypes.c_int]
    return lib


def emulated(emu, x, pre_gain, ceiling, lookahead, release, lookback=-1):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out, d0 = np.empty_like(x), np.empty(x.shape[0], dtype=np.float32)
    worst = emu.emu_tp_limit(x.ctypes.data, x.shape[0], pre_gain, ceiling, lookahead, float(release), out.ctypes.data,
                             d0.ctypes.data, lookback)
    return out, worst, d0


def test_version():
    assert _native.library().mgx_version() >= 106


# ---- the definition, on the oracle --------------------------------------------------------------------------------------

def guarantee_signals(n=3000):
    rng = np.random.RandomState(11)
    t = np.arange(n)
    noise = 0.7 * rng.standard_normal((n, 2))
    bursts = 0.1 * rng.standard_normal((n, 2))
    bursts[700:760] *= 12.0
    bursts[2100:2103] *= 20.0
    square = np.where((t // 37) % 2 == 0, 1.0, -1.0)[:, None] * np.ones((1, 2))
    alternating = np.where(t % 2 == 0, 0.998, -0.998)[:, None] * np.array([[1.0, -1.0]])
    first, last = np.zeros((n, 2)), np.zeros((n, 2))
    first[0], last[n - 1] = (1.0, 0.5), (-0.3, 1.0)
    return {"noise": noise, "bursts": bursts, "square": square, "alternating": alternating, "impulse at 0": first,
            "impulse at n - 1": last}


def test_the_oracle_holds_the_frame_bound():
    """(1 - s[m]) e[m] <= c (1 + 1e-12) for every frame; the largest value seen is 1 + 1e-15, rounding of the product."""
    worst = 0.0
    for name, x in guarantee_signals().items():
        x = x.astype(np.float32)
        for lookahead in (1, 8, 66):
            for release in (0, 32, 2205):
                for pre_gain, ceiling in ((1.0, 0.5), (2.0, 0.891)):
                    got = oracle.limit(x, pre_gain, ceiling, lookahead, release)
                    held = float(((1.0 - got.s) * got.e).max()) / ceiling
                    worst = max(worst, held)
                    assert held <= 1.0 + 1e-12, (name, lookahead, release, held)
                    assert got.max_reduction > 0.0 and np.all(got.s >= 0.0) and np.all(got.s < 1.0)
    print("largest (1 - s) e / c:", worst)


def test_zero_padding_would_break_the_bound_at_the_edges():
    """Why step 5 repeats the edge frames: with zeros beyond the track a peak at frame 3 comes out over the ceiling."""
    x = np.zeros((400, 2), dtype=np.float32)
    x[3] = (1.0, 1.0)
    padded = oracle.limit(x, 1.0, 0.5, 8, 32, clamp=False)
    clamped = oracle.limit(x, 1.0, 0.5, 8, 32)
    assert ((1.0 - padded.s) * padded.e).max() > 0.5 * 1.05
    assert ((1.0 - clamped.s) * clamped.e).max() <= 0.5 * (1.0 + 1e-12)


def test_the_envelope_is_the_meters_true_peak():
    x = cases.edge_signal(777)
    e = oracle.envelope(x, 1.0)
    assert e.max() == loudness_oracle.peaks(x)[0]
    # phase 0 is the frame itself (numpy.sinc of a whole number is 4e-17, not 0: an ulp of room)
    assert np.all(e >= np.abs(x.astype(np.float64)).max(axis=1) * (1.0 - 1e-15))


def test_below_the_ceiling_the_oracle_is_the_pre_gain_alone():
    x = cases.quiet_signal(1000)
    got = oracle.limit(x, 1.7, 0.5, 66, 2205)
    assert not got.s.any() and got.max_reduction == 0.0
    assert np.array_equal(got.out, (x.astype(np.float64) * 1.7).astype(np.float32))


# ---- the kernels' phases on the CPU -----------------------------------------------------------------------------------------

def test_the_shared_constants_are_the_headers(emu):
    text = open(os.path.join(ROOT, "matchering_amd", "csrc", "tp_limit_kernel.h")).read()
    assert re.search(r"TPL_THREADS = 256;", text) and re.search(r"TPL_RUN = 16;", text)
    assert re.search(r"TPL_TILE = TPL_THREADS \* TPL_RUN;", text) and re.search(r"TPL_BLOCK = TPL_TILE;", text)
    assert re.search(r"TPL_LOOKAHEAD_MAX = 2048;", text)
    out = (ctypes.c_longlong * 7)()
    emu.emu_tp_limit_constants(cases.LOOKAHEAD_MAX, out)
    assert list(out)[:4] == [cases.TILE, cases.BLOCK, cases.THREADS, cases.LOOKAHEAD_MAX]
    assert out[4] <= 150 * 1024                                  # the largest look-ahead's workgroup fits a CU's LDS
    from matchering_amd import delivery

    assert delivery.LOOKAHEAD_MAX == cases.LOOKAHEAD_MAX and delivery.PASSES_MAX == _native.LIMIT_PASSES_MAX == 16
    header = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert re.search(r"#define MGX_LIMIT_PASSES_MAX 16\b", header)


@pytest.mark.parametrize("lookahead", cases.LOOKAHEADS)
def test_emulation_against_the_oracle_at_the_edges(emu, lookahead):
    """Per sample 2^-24 |g x| + half a float32 spacing of the oracle's value: a float32 d0 plane's 2^-25 on the gain,
    doubled, and the store's rounding -- derived, not measured."""
    worst = 0.0
    for n in cases.edge_sizes(lookahead):
        for release in cases.RELEASES:
            x, want = cases.edge_case(n, lookahead, release)
            got, reduction, d0 = emulated(emu, x, cases.PRE_GAIN, cases.CEILING, lookahead, release)
            ok, ratio = cases.within(got, x, cases.PRE_GAIN, want.out)
            worst = max(worst, ratio)
            assert ok, (n, lookahead, release, ratio)
            assert abs(reduction - want.max_reduction) <= 2.0 ** -24, (n, lookahead, release)
            # the plane is d0 rounded to nearest: half a float32 spacing below 1 (and the envelopes' own 1e-16 apart)
            assert np.abs(d0.astype(np.float64) - oracle.reduction(want.e, cases.CEILING)).max() <= 2.0 ** -25 + 1e-12
    print("look-ahead", lookahead, "largest error / tolerance:", worst)


def test_emulation_carries_the_release_across_many_workgroups(emu):
    x, want = cases.carry_case()
    c = cases.CARRY
    got, reduction, _ = emulated(emu, x, c["pre_gain"], c["ceiling"], c["lookahead"], c["release"])
    ok, ratio = cases.within(got, x, c["pre_gain"], want.out)
    assert ok, ratio
    # the recovery is still a thousand tolerances deep five tiles behind the impulse, and gone by the last
    assert want.s[5 * cases.TILE] > 1e3 * 2.0 ** -24 and want.s[-1] < 2.0 ** -24
    loud = np.abs(x[:, 0]) > 1e-3
    gain = got[loud, 0].astype(np.float64) / (c["pre_gain"] * x[loud, 0].astype(np.float64))
    assert np.abs(gain - (1.0 - want.s[loud])).max() <= 2.0 ** -23          # (a float32 quotient: 2^-24 of its own on top)
    # without the carry (look-back 0) the tiles behind the first come out too loud: the test can see a lost carry
    alone, _, _ = emulated(emu, x, c["pre_gain"], c["ceiling"], c["lookahead"], c["release"], lookback=0)
    assert not cases.within(alone, x, c["pre_gain"], want.out)[0]
    assert np.array_equal(alone[:cases.TILE - 2 * c["lookahead"] - 2], got[:cases.TILE - 2 * c["lookahead"] - 2])


def test_emulation_is_the_identity_below_the_ceiling(emu):
    for n in (1, 513, cases.TILE + 5):
        x = cases.quiet_signal(n)
        got, reduction, d0 = emulated(emu, x, 1.7, 0.5, 66, 2205)
        assert reduction == 0.0 and not d0.any()
        assert got.tobytes() == (x.astype(np.float64) * 1.7).astype(np.float32).tobytes()


# ---- the policy ---------------------------------------------------------------------------------------------------------------

def native_step(target, ceiling, bits, dither, integrated0, true_peak0, pre=(), loud=(), max_passes=4, tolerance_lu=0.1):
    lib = _native.library()
    spec = _native.MgxDelivery(math.nan if target is None else target, math.nan if ceiling is None else ceiling, bits, dither, 0)
    report = _native.MgxLoudnessReport()
    report.integrated, report.true_peak = integrated0, true_peak0
    array = ctypes.c_double * max(len(pre), 1)
    plan = _native.MgxDeliveryLimitPlan()
    rc = lib.mgx_delivery_limit_step(ctypes.byref(spec), ctypes.byref(report), len(pre), array(*pre), array(*loud), max_passes,
                                     tolerance_lu, ctypes.byref(plan))
    return rc, plan, lib.mgx_last_error().decode()


def run_policy(target, ceiling, integrated0, true_peak0, readings, **kwargs):
    """The pre-gains the policy asks for when pass k reads ``readings[k]``; both the library and the oracle."""
    pre, loud = [], []
    while True:
        rc, plan, _ = native_step(target, ceiling, 0, 0, integrated0, true_peak0, pre, loud, **kwargs)
        assert rc == 0
        want = oracle.limit_step(target, ceiling, 0, 0, integrated0, true_peak0, pre, loud, kwargs.get("max_passes", 4),
                                 kwargs.get("tolerance_lu", 0.1))
        assert bool(plan.run) == want.run and plan.ceiling == want.ceiling
        assert abs(plan.pre_gain_db - want.pre_gain_db) <= 1e-12
        if not plan.run:
            return pre
        pre.append(plan.pre_gain_db)
        loud.append(readings[len(loud)])


def test_policy_against_hand_computed_sequences():
    inf = math.inf
    # the ceiling does not bind (-4 dB reaches -14 LUFS with the peak at 0.32): no pass
    assert run_policy(-14.0, -1.0, -10.0, 0.5, []) == []
    # no loudness target: one pass at pre-gain 0
    assert run_policy(None, -1.0, -12.0, 1.2, [-12.4]) == [0.0]
    # a steady tone: 3.9 dB more pre-gain buy 0.01 LU -- slope 0.0026 < 0.1 ends it at pass 2
    pre = run_policy(-9.0, -1.0, -12.0, 1.0, [-12.9, -12.89])
    assert len(pre) == 2 and pre[0] == 3.0 and abs(pre[1] - 6.9) <= 1e-12
    # silence: nothing binds
    assert run_policy(-9.0, -1.0, -inf, 0.0, []) == []
    # a track too short to have a loudness, with a peak over the ceiling: one pass at pre-gain 0, as without a target
    assert run_policy(-9.0, -1.0, -inf, 1.2, [-inf]) == [0.0]
    # ... and one whose limited frames gate out altogether
    assert run_policy(-9.0, -1.0, -14.0, 1.0, [-inf]) == [5.0]
    # the search: p1 = T - I0 = 5; slope 1: p2 = 5 + 1.5; slope 0.6 / 1.5 = 0.4: p3 = 6.5 + 0.9 / 0.4; 0.05 LU short: done
    pre = run_policy(-9.0, -1.0, -14.0, 1.0, [-10.5, -9.9, -9.05])
    assert len(pre) == 3 and pre[0] == 5.0 and pre[1] == 6.5 and abs(pre[2] - 8.75) <= 1e-12
    # max_passes ends it sooner, the tolerance later
    assert run_policy(-9.0, -1.0, -14.0, 1.0, [-10.5, -9.9, -9.05], max_passes=2) == pre[:2]
    assert run_policy(-9.0, -1.0, -14.0, 1.0, [-10.5, -9.9, -9.05], max_passes=1) == pre[:1]
    longer = run_policy(-9.0, -1.0, -14.0, 1.0, [-10.5, -9.9, -9.05, -9.01], tolerance_lu=0.02)
    assert len(longer) == 4 and longer[:3] == pre and abs(longer[3] - (8.75 + 0.05 / (0.85 / 2.25))) <= 1e-12
    # a slope between 0.1 and the stop: 0.12 is used as it is
    pre = run_policy(-9.0, -1.0, -14.0, 1.0, [-10.5, -10.32, -9.0])
    assert len(pre) == 3 and abs(pre[2] - (6.5 + 1.32 / 0.12)) <= 1e-9
    # the first pass reaches the target within the tolerance
    assert run_policy(-9.0, -1.0, -14.0, 1.0, [-9.08]) == [5.0]


def test_policy_ceiling_is_the_gain_rules_numerator():
    for bits, dither in FORMATS:
        rc, plan, _ = native_step(-9.0, -1.0, bits, dither, -14.0, 2.0)
        assert rc == 0 and plan.run == 1
        linear = delivery_oracle.delivery_gain(-9.0, -1.0, bits, dither, -14.0, 2.0)
        assert plan.ceiling == oracle.room(-1.0, bits, dither)
        assert abs(plan.ceiling - linear.gain * 2.0) <= 1e-15              # g_peak true_peak


def test_policy_refusals():
    bad = [native_step(-9.0, None, 16, 0, -14.0, 1.0),                      # a limiter needs a ceiling
           native_step(-9.0, -1.0, 16, 0, -14.0, 1.0, max_passes=0), native_step(-9.0, -1.0, 16, 0, -14.0, 1.0, max_passes=17),
           native_step(-9.0, -1.0, 16, 0, -14.0, 1.0, tolerance_lu=-0.1), native_step(-9.0, -1.0, 16, 0, -14.0, 1.0, tolerance_lu=math.nan),
           native_step(-9.0, -1.0, 16, 0, -14.0, 1.0, pre=(1.0,) * 5, loud=(-10.0,) * 5),      # more passes than max_passes
           native_step(-9.0, -1.0, 16, 0, -14.0, 1.0, pre=(math.nan,), loud=(-10.0,)),
           native_step(-9.0, -1.0, 16, 0, -14.0, 1.0, pre=(1.0,), loud=(math.inf,)),
           native_step(-9.0, -1.0, 20, 0, -14.0, 1.0), native_step(-9.0, 1.0, 16, 0, -14.0, 1.0),   # mgx_delivery_gain's own
           native_step(-9.0, -1.0, 16, 0, math.nan, 1.0)]
    assert [rc for rc, _, _ in bad] == [_native.ERR_ARGUMENT] * len(bad)
    assert "ceiling" in bad[0][2] and "max_passes" in bad[1][2] and "tolerance_lu" in bad[3][2] and "passes" in bad[5][2]
    lib = _native.library()
    assert lib.mgx_delivery_limit_step(None, None, 0, None, None, 4, 0.1, None) == _native.ERR_ARGUMENT


# ---- the pipeline, on the oracle -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def music():
    """1.6 s of the synthetic programme material, loud enough for a true peak near 2."""
    x = (3.0 * synth(1.6, RATE, seed=9)).astype(np.float32)
    return x, loudness_oracle.measure(x, RATE)


def test_pipeline_on_the_oracle_holds_the_ceiling_and_gains_loudness(music):
    x, measured = music
    ceiling = -1.0
    reach = delivery_oracle.delivery_gain(0.0, ceiling, 0, 0, measured.integrated, measured.true_peak).achieved_lufs
    target = reach + 3.0
    for bits, dither in FORMATS:
        done = oracle.pipeline(x, RATE, target, ceiling, bits, dither, 2 ** 40 + 3, 66, 2205.0, 4, 0.1, measured=measured)
        assert done.linear.limited_by == 2 and done.passes >= 1
        read_back = loudness_oracle.measure(delivery_oracle.decoded(done.values, bits), RATE)
        print(bits, dither, "passes", done.passes, "pre-gains", done.pre_gains_db, "shortfall", done.gain.shortfall_lu, "against",
              done.linear.shortfall_lu, "read back", read_back.integrated, read_back.true_peak)
        assert read_back.true_peak <= 10.0 ** (ceiling / 20.0) * (1.0 + 1e-12), (bits, dither)
        assert done.gain.shortfall_lu < done.linear.shortfall_lu, (bits, dither)
        assert abs(read_back.integrated - done.gain.achieved_lufs) <= 0.01


def test_pipeline_without_a_binding_ceiling_is_the_linear_delivery(music):
    x, measured = music
    done = oracle.pipeline(x, RATE, measured.integrated - 12.0, -1.0, 16, 1, 5, 66, 2205.0, 4, 0.1, measured=measured)
    linear = delivery_oracle.delivery_gain(measured.integrated - 12.0, -1.0, 16, 1, measured.integrated, measured.true_peak)
    assert done.passes == 0 and done.gain == linear and np.array_equal(done.limited, x)
    assert np.array_equal(done.values, delivery_oracle.deliver(x, linear.gain, 16, 1, 5))


# ---- the surface ---------------------------------------------------------------------------------------------------------------

def test_limiter_and_delivery_validation():
    assert Delivery() == Delivery(None, None, None, 0) and Delivery().limiter is None
    limiter = TruePeakLimiter()
    assert (limiter.lookahead_ms, limiter.release_ms, limiter.max_passes, limiter.tolerance_lu) == (1.5, 50.0, 4, 0.1)
    assert limiter.frames(44100) == (66, 2205.0) and limiter.frames(48000) == (72, 2400.0)
    assert TruePeakLimiter(lookahead_ms=0.001).frames(44100)[0] == 1 and TruePeakLimiter(release_ms=0).frames(44100)[1] == 0.0
    assert TruePeakLimiter(lookahead_ms=10.0).frames(192000) == (1920, 9600.0)
    for kwargs in ({"lookahead_ms": 0.0}, {"lookahead_ms": -1.0}, {"lookahead_ms": math.nan}, {"release_ms": -1.0},
                   {"release_ms": math.inf}, {"max_passes": 0}, {"max_passes": 17}, {"max_passes": 2.0}, {"max_passes": True},
                   {"tolerance_lu": -0.1}, {"tolerance_lu": "0.1"}):
        with pytest.raises(ValueError, match="TruePeakLimiter"):
            TruePeakLimiter(**kwargs)
    with pytest.raises(ValueError, match="more than 2048"):
        TruePeakLimiter(lookahead_ms=50.0).frames(44100)
    with pytest.raises(ValueError, match="frames"):
        TruePeakLimiter(release_ms=1e6).frames(44100)
    with pytest.raises(ValueError, match="needs a true_peak"):
        Delivery(loudness=-9.0, limiter=limiter)
    with pytest.raises(ValueError, match="TruePeakLimiter or None"):
        Delivery(true_peak=-1.0, limiter=True)
    spec = Delivery(loudness=-9.0, true_peak=-1.0, dither="tpdf_hp", limiter=limiter)
    assert spec.limiter is limiter and spec == Delivery(-9.0, -1.0, "tpdf_hp", 0, TruePeakLimiter())
    mg.pcm16("club.wav", delivery=spec)                                    # a Result takes it as any delivery
    assert mg.TruePeakLimiter is TruePeakLimiter


def test_from_json():
    assert Delivery.from_json({"loudness": -9, "true_peak": -1, "limiter": True}) == Delivery(-9, -1, limiter=TruePeakLimiter())
    assert Delivery.from_json({"true_peak": -1, "limiter": {"lookahead_ms": 3.0, "max_passes": 2}}) == \
        Delivery(true_peak=-1, limiter=TruePeakLimiter(lookahead_ms=3.0, max_passes=2))
    assert Delivery.from_json({"true_peak": -1, "limiter": None}) == Delivery(true_peak=-1)
    assert Delivery.from_json({"true_peak": -1, "limiter": False}) == Delivery(true_peak=-1)
    assert Delivery.from_json({"loudness": -14}) == Delivery(-14)
    for entry in ({"true_peak": -1, "limiter": {"attack": 1}}, {"true_peak": -1, "limiter": "yes"}, {"true_peak": -1, "limiter": 1.5},
                  {"loudness": -9, "limiter": True}, {"true_peak": -1, "limiter": {"max_passes": 0}}):
        with pytest.raises(ValueError):
            Delivery.from_json(entry)


def test_a_batch_job_passes_the_limiter_through(tmp_path):
    import json

    from matchering_amd import batch

    job = {"target": "t.wav", "reference": "r.wav",
           "results": [{"file": "a.wav", "subtype": "PCM_16", "delivery": {"loudness": -9, "true_peak": -1, "limiter": True}},
                       {"file": "b.wav", "subtype": "PCM_24", "delivery": {"true_peak": -1, "limiter": {"release_ms": 80.0}}},
                       {"file": "c.wav", "delivery": {"loudness": -14}}]}
    with open(tmp_path / "jobs.json", "w") as fh:
        json.dump([job], fh)
    results = batch.jobs_from_json(str(tmp_path / "jobs.json"))[0]["results"]
    assert results[0].delivery == Delivery(-9, -1, limiter=TruePeakLimiter())
    assert results[1].delivery.limiter == TruePeakLimiter(release_ms=80.0) and results[2].delivery.limiter is None


def reading(integrated, true_peak):
    return Loudness(integrated, 0.0, integrated, integrated, true_peak, true_peak, RATE, 0, 0, 4410)


def test_delivered_record_and_the_python_policy():
    spec = Delivery(loudness=-9.0, true_peak=-1.0, limiter=TruePeakLimiter())
    first = reading(-14.0, 1.0)
    assert limit_step(Delivery(loudness=-20.0, true_peak=-1.0, limiter=TruePeakLimiter()), 0, first) == (False, 0.0, 10.0 ** -0.05)
    run, pre_gain_db, ceiling = limit_step(spec, 0, first)
    assert run and pre_gain_db == 5.0 and ceiling == 10.0 ** -0.05
    assert limit_step(spec, 0, first, [5.0], [-10.5])[:2] == (True, 6.5)
    assert limit_step(spec, 0, first, [5.0], [-9.05])[:2] == (False, 5.0)
    with pytest.raises(ValueError):
        limit_step(Delivery(true_peak=-1.0), 0, first)
    with pytest.raises(ValueError):
        limit_step(spec, 0, first, [5.0], [])
    plain = delivery_gain(spec, 16, first)
    assert plain.limiter_passes == 0 and plain.limited is None and "limited in" not in str(plain)
    assert Delivered(*[getattr(plain, name) for name in ("gain", "achieved_lufs", "achieved_true_peak", "shortfall_lu",
                                                          "limited_by", "measured", "delivery", "bits")]) == plain
    from dataclasses import replace

    limited = replace(delivery_gain(spec, 16, reading(-9.3, 0.9)), measured=first, limiter_passes=2, pre_gain_db=6.5,
                      max_reduction_db=-4.25, limited=reading(-9.3, 0.9))
    text = str(limited)
    assert "limited in 2 passes: pre-gain +6.50 dB, at most -4.25 dB of reduction" in text
    assert "LU under the -9 LUFS target" in text and limited.shortfall_lu > 0.0
    assert "limited in 1 pass:" in str(replace(limited, limiter_passes=1))


def test_tp_limit_refusals_that_need_no_device():
    lib = _native.library()

    def call(handle=None, x=0x1000, n=64, pre_gain=1.0, ceiling=0.5, lookahead=66, release=2205.0, out=0x2000):
        rc = lib.mgx_tp_limit(handle, P(x), n, pre_gain, ceiling, lookahead, release, P(out), None)
        return rc, lib.mgx_last_error().decode()

    for kwargs, field in (({"n": -1}, "n:"), ({"pre_gain": 0.0}, "pre_gain"), ({"pre_gain": -1.0}, "pre_gain"),
                          ({"pre_gain": math.inf}, "pre_gain"), ({"pre_gain": math.nan}, "pre_gain"), ({"ceiling": 0.0}, "ceiling"),
                          ({"ceiling": math.nan}, "ceiling"), ({"ceiling": math.inf}, "ceiling"), ({"lookahead": 0}, "lookahead"),
                          ({"lookahead": 2049}, "lookahead"), ({"lookahead": -5}, "lookahead"), ({"release": -1.0}, "release"),
                          ({"release": math.nan}, "release"), ({"release": math.inf}, "release"), ({"release": 2.0 ** 22 + 1}, "release"),
                          ({}, "handle")):
        rc, message = call(**kwargs)
        assert rc == _native.ERR_ARGUMENT and field in message, (kwargs, message)
    assert "mgx_tp_limit" in _native.SYMBOLS and "mgx_delivery_limit_step" in _native.SYMBOLS
