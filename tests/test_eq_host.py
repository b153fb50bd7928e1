"""Matching EQ controls without a GPU: ``MatchingEq``, ``mgx_eq_shape_check``, and ``mgx_shape_fir`` -- the library's host
restatement of the shape stage and the minimum-phase chain -- against tests/eq_oracle.py; the properties of the
definition on the oracle alone and then on the host code; the stand-alone program under the sanitizers.
"""

import ctypes
import subprocess

import numpy as np
import pytest

import eq_oracle
import mastering_oracle as mo
from cases import CASES, build_inputs, oracle_params

NAN = float("nan")
c_double_p = ctypes.POINTER(ctypes.c_double)


def native(fft=4096):
    """The default Config's mgx_config at another fft_size (set on the struct: the host entry points take any size)."""
    import matchering_amd as mg

    cfg = mg.Config().to_native()
    cfg.fft_size = fft
    return cfg


def shape_struct(amount=1.0, max_boost_db=None, max_cut_db=None, phase="linear", reserved=0):
    from matchering_amd._native import MgxEqShape

    return MgxEqShape(amount, NAN if max_boost_db is None else max_boost_db, NAN if max_cut_db is None else max_cut_db,
                      {"linear": 0, "minimum": 1}.get(phase, phase), reserved)


def host_shape_fir(smooth, fft, **shape):
    from matchering_amd._native import check, library

    smooth = np.ascontiguousarray(smooth, dtype=np.float64)
    assert smooth.shape == (fft // 2 + 1,)
    taps = np.full(fft, 7.0)
    check(library().mgx_shape_fir(ctypes.byref(native(fft)), ctypes.byref(shape_struct(**shape)),
                                  smooth.ctypes.data_as(c_double_p), taps.ctypes.data_as(c_double_p)))
    return taps


def synthetic_curve(fft, seed=0):
    """A smoothed matching curve's look: a few dB of slow ripple, a steep rise at the top, bin 0 zero."""
    k = np.arange(fft // 2 + 1) / (fft // 2)
    rng = np.random.RandomState(seed)
    db = 9.0 * np.sin(2 * np.pi * (1.3 + seed) * k + rng.rand()) + 7.0 * np.cos(2 * np.pi * 4.1 * k) + 25.0 * k ** 6 - 6.0
    curve = 10.0 ** (db / 20.0)
    curve[0] = 0.0
    return curve


# ---- MatchingEq ---------------------------------------------------------------------------------------------------------
def test_matching_eq_validation():
    import matchering_amd as mg

    eq = mg.MatchingEq()
    assert (eq.amount, eq.max_boost_db, eq.max_cut_db, eq.phase) == (1.0, None, None, "linear") and eq.is_default
    with pytest.raises(Exception):
        eq.amount = 0.5                                             # frozen
    for bad in (dict(amount=-0.1), dict(amount=2.1), dict(amount=NAN), dict(amount="1"), dict(amount=True),
                dict(max_boost_db=-1.0), dict(max_cut_db=-0.5), dict(max_boost_db=float("inf")), dict(max_cut_db="6"),
                dict(phase="zero"), dict(phase=1)):
        with pytest.raises(ValueError):
            mg.MatchingEq(**bad)
    eq = mg.MatchingEq(amount=0.5, max_boost_db=6, max_cut_db=6, phase="minimum")
    assert eq.describe() == "matching EQ: 50 %, +6/−6 dB, minimum phase"
    assert mg.MatchingEq(amount=2).describe() == "matching EQ: 200 %, no caps, linear phase"
    s = eq.to_native()
    assert (s.amount, s.max_boost_db, s.max_cut_db, s.phase, s.reserved) == (0.5, 6.0, 6.0, 1, 0)
    s = mg.MatchingEq().to_native()
    assert np.isnan(s.max_boost_db) and np.isnan(s.max_cut_db) and s.phase == 0


def test_matching_eq_from_json():
    import matchering_amd as mg

    assert mg.MatchingEq.from_json({}) == mg.MatchingEq()
    assert mg.MatchingEq.from_json(None) is None
    eq = mg.MatchingEq.from_json({"amount": 0.5, "max_boost_db": 6, "max_cut_db": 3, "phase": "minimum"})
    assert eq == mg.MatchingEq(0.5, 6, 3, "minimum") and mg.MatchingEq.from_json(eq) is eq
    with pytest.raises(ValueError, match="unknown keys.*strength"):
        mg.MatchingEq.from_json({"strength": 0.5})
    with pytest.raises(ValueError):
        mg.MatchingEq.from_json([0.5])
    with pytest.raises(ValueError):
        mg.MatchingEq.from_json({"amount": 3})


def test_process_refuses_before_any_file_is_read(tmp_path):
    """``process`` validates through mgx_eq_shape_check before it loads audio: the files named here do not exist."""
    import matchering_amd as mg

    results = [mg.pcm16(str(tmp_path / "out.wav"))]
    with pytest.raises(ValueError, match="32768"):
        mg.process(str(tmp_path / "no_target.wav"), str(tmp_path / "no_reference.wav"), results,
                   config=mg.Config(fft_size=32768), eq=mg.MatchingEq(phase="minimum"))
    with pytest.raises(ValueError, match="unknown keys"):
        mg.process(str(tmp_path / "no_target.wav"), str(tmp_path / "no_reference.wav"), results, eq={"amout": 1})
    jobs = [{"target": str(tmp_path / "t.wav"), "reference": str(tmp_path / "r.wav"), "results": results,
             "eq": {"phase": "minimum"}}]
    with pytest.raises(ValueError, match="not 32"):
        mg.process_batch(jobs, config=mg.Config(fft_size=32, max_piece_size=1.0), rank=0, world_size=1)


# ---- mgx_eq_shape_check -------------------------------------------------------------------------------------------------
def test_eq_shape_check_ranges_and_refusals():
    from matchering_amd._native import ERR_ARGUMENT, ERR_UNSUPPORTED, library

    lib = library()

    def rc(fft, **shape):
        return lib.mgx_eq_shape_check(ctypes.byref(native(fft)), ctypes.byref(shape_struct(**shape)))

    assert rc(4096) == 0 and rc(4096, amount=0.0) == 0 and rc(4096, amount=2.0, max_boost_db=0.0, max_cut_db=0.0) == 0
    for bad, field in ((dict(amount=-1e-9), "amount"), (dict(amount=2.0000001), "amount"), (dict(amount=NAN), "amount"),
                       (dict(amount=float("inf")), "amount"), (dict(max_boost_db=-0.1), "max_boost_db"),
                       (dict(max_boost_db=float("inf")), "max_boost_db"), (dict(max_cut_db=-3.0), "max_cut_db"),
                       (dict(phase=2), "phase"), (dict(phase=-1), "phase"), (dict(reserved=1), "reserved")):
        assert rc(4096, **bad) == ERR_ARGUMENT
        assert field in lib.mgx_last_error().decode()
    assert lib.mgx_eq_shape_check(None, ctypes.byref(shape_struct())) == ERR_ARGUMENT
    assert lib.mgx_eq_shape_check(ctypes.byref(native()), None) == ERR_ARGUMENT
    for fft in (64, 512, 4096, 16384):
        assert rc(fft, phase="minimum") == 0
    for fft in (8, 32, 32768, 65536):
        assert rc(fft, phase="linear", amount=0.5) == 0                    # (the shape stage runs at every size)
        assert rc(fft, phase="minimum") == ERR_UNSUPPORTED
        message = lib.mgx_last_error().decode()
        assert f"not {fft}" in message and "minimum-phase" in message


# ---- mgx_shape_fir against the oracle ------------------------------------------------------------------------------------
SHAPES = [dict(amount=0.0), dict(amount=0.5), dict(amount=1.0), dict(amount=2.0),
          dict(amount=1.0, max_boost_db=3.0, max_cut_db=2.0),            # caps that bind
          dict(amount=0.5, max_boost_db=60.0, max_cut_db=80.0)]          # caps that do not


@pytest.fixture(scope="module")
def oracle_fir():
    """(fft, shape, phase, clamped) -> eq_oracle's taps: computed once, shared, never written."""
    cache = {}

    def get(fft, index, phase, clamped=False):
        key = (fft, index, phase, clamped)
        if key not in cache:
            curve = synthetic_curve(fft, index)
            if clamped:
                curve[3::11] = -0.25
                curve[5::13] = 0.0
            taps = eq_oracle.shape_fir(curve, 1e-6, phase=phase, **SHAPES[index])
            taps.setflags(write=False)
            cache[key] = (curve, taps)
        return cache[key]

    return get


@pytest.mark.parametrize("phase", ["linear", "minimum"])
@pytest.mark.parametrize("index", range(len(SHAPES)))
@pytest.mark.parametrize("fft", [64, 512, 4096, 16384])
def test_shape_fir_matches_the_oracle(oracle_fir, fft, index, phase):
    """float64 on both sides: <= 1e-9 of the peak tap.  (The oracle's own rerun through another summation order --
    eq_oracle.minimum_phase(permute=...) -- stays below 3e-14 of the peak on every golden curve and on these, so the
    bound needs no widening; test_oracle_is_stable_under_another_summation_order holds it to 1e-10.)"""
    curve, want = oracle_fir(fft, index, phase)
    got = host_shape_fir(curve, fft, phase=phase, **SHAPES[index])
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


@pytest.mark.parametrize("phase", ["linear", "minimum"])
@pytest.mark.parametrize("fft", [64, 4096])
def test_shape_fir_clamps_non_positive_entries(oracle_fir, fft, phase):
    """Curve entries <= 0 count as min_value (-120 dB at the default): at amount 0.5 they are cut by 60 dB, by the cap where
    one is given -- the deep-floor bins of the minimum-phase logarithm."""
    for index in (1, 4):
        curve, want = oracle_fir(fft, index, phase, clamped=True)
        got = host_shape_fir(curve, fft, phase=phase, **SHAPES[index])
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


def test_oracle_is_stable_under_another_summation_order(oracle_fir):
    for fft in (64, 4096):
        for clamped in (False, True):
            _, lin = oracle_fir(fft, 1, "linear", clamped)
            a, b = eq_oracle.minimum_phase(lin), eq_oracle.minimum_phase(lin, permute=fft // 3 + 1)
            assert np.abs(a - b).max() <= 1e-10 * np.abs(a).max()


# ---- properties of the definition: on the oracle, then on the host code -------------------------------------------------
MAGNITUDE_BOUND_DB = 2 * 0.143


@pytest.fixture(scope="module")
def golden_curves():
    """The smoothed curves of the golden cases (mid and side), sizes up to 16384: the oracle's own analysis and design."""
    out = []
    for name in sorted(CASES):
        case = CASES[name]
        if case["config"].get("fft_size", 4096) > 16384 or case["config"].get("fft_size", 4096) < 64:
            continue
        target, reference = build_inputs(case)
        cfg = oracle_params(case["config"])
        trace = {}
        mo.master(target, reference, cfg, False, True, False, trace=trace)
        out += [(name, ch, cfg, trace[ch].smooth) for ch in ("mid", "side")]
    return out


def test_minimum_phase_magnitude_stays_with_the_linear_one(golden_curves):
    """From bin 2 of the F grid up, |rfft| of the minimum-phase taps within a bound of the linear-phase taps', over the
    golden cases' curves at amount 1 and at amount 0.5 with +-6 dB caps.  Measured on the oracle: 0.143 dB at most
    (robust_second_order, mid, amount 1; the issue's pair gave 0.13); the bound asserted is twice that, 0.286 dB, for the
    oracle and for mgx_shape_fir alike.  Zero before F/2, nothing lost behind it."""
    import matchering_amd as mg

    worst = 0.0
    for name, channel, cfg, smooth in golden_curves:
        fft = cfg.fft_size
        native_cfg = mg.Config(fft_size=fft, max_piece_size=1.0, internal_sample_rate=cfg.internal_sample_rate,
                               lin_log_oversampling=cfg.lin_log_oversampling, lowess_it=cfg.lowess_it).to_native()
        for shape in (dict(), dict(amount=0.5, max_boost_db=6.0, max_cut_db=6.0)):
            lin = eq_oracle.shape_fir(smooth, cfg.min_value, **shape)
            minimum = eq_oracle.shape_fir(smooth, cfg.min_value, phase="minimum", **shape)
            assert not minimum[:fft // 2].any()
            off = np.abs(eq_oracle.magnitude_db(minimum)[2:] - eq_oracle.magnitude_db(lin)[2:]).max()
            worst = max(worst, off)
            assert off <= MAGNITUDE_BOUND_DB, (name, channel, shape, off)
            # ... and the host code
            from matchering_amd._native import check, library

            got = np.zeros(fft)
            check(library().mgx_shape_fir(ctypes.byref(native_cfg), ctypes.byref(shape_struct(phase="minimum", **shape)),
                                          np.ascontiguousarray(smooth).ctypes.data_as(c_double_p), got.ctypes.data_as(c_double_p)))
            assert not got[:fft // 2].any()
            assert np.abs(eq_oracle.magnitude_db(got)[2:] - eq_oracle.magnitude_db(lin)[2:]).max() <= MAGNITUDE_BOUND_DB
            assert np.abs(got - minimum).max() <= 1e-9 * np.abs(minimum).max()
    print(f"largest deviation of the oracle's minimum-phase magnitude: {worst:.4f} dB")
    assert worst > 0.05                                                          # (the measurement the bound came from still stands)


def test_minimum_phase_has_no_pre_ringing_and_keeps_the_energy(golden_curves):
    """What the feature is for: the linear-phase FIR of these curves has 15-30 % of its energy before its main tap, the
    minimum-phase one none, with the same total to within the magnitude bound."""
    for name, channel, cfg, smooth in golden_curves[:6]:
        lin = eq_oracle.shape_fir(smooth, cfg.min_value)
        minimum = eq_oracle.shape_fir(smooth, cfg.min_value, phase="minimum")
        peak = int(np.argmax(np.abs(lin)))
        assert peak == cfg.fft_size // 2
        assert np.sum(lin[:peak] ** 2) > 0.1 * np.sum(lin ** 2)
        assert np.sum(minimum[:peak] ** 2) == 0.0
        assert abs(10.0 * np.log10(np.sum(minimum ** 2) / np.sum(lin ** 2))) <= MAGNITUDE_BOUND_DB


@pytest.mark.parametrize("fft", [8, 64, 4096])
def test_default_shape_is_mgx_design_fir(fft):
    """amount 1 without caps, linear phase: exactly mgx_design_fir's taps, bit for bit -- the stage is skipped, not
    multiplied by one."""
    from matchering_amd._native import check, library

    rng = np.random.RandomState(fft)
    bins = fft // 2 + 1
    avg_t = np.abs(rng.randn(bins)) + 0.05
    avg_r = np.abs(rng.randn(bins)) + 0.05
    cfg = native(fft)
    taps, raw, smooth = np.zeros(fft), np.zeros(bins), np.zeros(bins)
    check(library().mgx_design_fir(ctypes.byref(cfg), avg_t.ctypes.data_as(c_double_p), avg_r.ctypes.data_as(c_double_p),
                                   taps.ctypes.data_as(c_double_p), raw.ctypes.data_as(c_double_p),
                                   smooth.ctypes.data_as(c_double_p)))
    assert np.array_equal(host_shape_fir(smooth, fft), taps)
    assert not np.array_equal(host_shape_fir(smooth, fft, amount=0.999), taps)


def test_shape_fir_refuses():
    from matchering_amd._native import ERR_ARGUMENT, ERR_UNSUPPORTED, library

    lib = library()
    smooth, taps = np.ones(17), np.zeros(32)
    args = (smooth.ctypes.data_as(c_double_p), taps.ctypes.data_as(c_double_p))
    assert lib.mgx_shape_fir(ctypes.byref(native(32)), ctypes.byref(shape_struct(phase="minimum")), *args) == ERR_UNSUPPORTED
    assert "32" in lib.mgx_last_error().decode()
    assert lib.mgx_shape_fir(ctypes.byref(native(32)), ctypes.byref(shape_struct(amount=3.0)), *args) == ERR_ARGUMENT
    assert lib.mgx_shape_fir(ctypes.byref(native(32)), None, *args) == ERR_ARGUMENT
    assert lib.mgx_shape_fir(ctypes.byref(native(32)), ctypes.byref(shape_struct(amount=0.5)), *args) == 0


# ---- the stand-alone program under the sanitizers ------------------------------------------------------------------------
def test_standalone_driver_under_sanitizers(tmp_path):
    """mgx_shape_fir (csrc/mgx_policy.cpp) and the emulated device chain over exactly sized buffers, built with
    AddressSanitizer and UBSan and run as a program of its own: ``ok`` and exit status 0."""
    import emu_build
    import eq_shape_emu

    out = str(tmp_path / "emu_eq_shape_driver")
    emu_build.build_driver(eq_shape_emu.NAME, out, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    done = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip() == "ok", done.stdout + done.stderr
