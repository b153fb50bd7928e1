"""The oracle against the UNMODIFIED reference.

``tests/test_oracle_golden.py`` pins the oracle through the frozen cases of tests/golden/cases.py; this module holds it
against further answers of the reference package's own ``stages.main`` (sergree/matchering; I/O imports stubbed,
oracle/reference_runner.py), frozen by tests/golden/reference_cases.py into tests/golden/reference_cases/ so that
the test needs nothing outside the repository.  Only ``stages.main`` and its helpers are exercised: the hot path.
Outputs and FIRs are held to the reference value for value on both edges and a seeded sample of the middle, and
every 64-value block sum of them to 64 times the same tolerance (reference_cases.assert_matches).
"""

import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import mastering_oracle as mo            # noqa: E402
import reference_cases as rc             # noqa: E402


@pytest.fixture(scope="module")
def frozen():
    return rc.load()


def _inputs(frozen, name):
    target, reference = rc.pair_inputs(name)
    assert rc.digest(target, reference) == str(frozen[name + "/input_sha256"]), "synthetic generator drifted; refreeze"
    return target, reference


def _master(name, target, reference):
    kw = dict(rc.PAIR_CASES[name]["config"])
    kw.update(kw.pop("limiter", {}))
    trace = {}
    return mo.master(target, reference, mo.params(**kw), True, True, True, trace=trace), trace


def _assert_outputs(frozen, name, outs):
    for k, mine in enumerate(outs):
        rc.assert_matches(mine, frozen, f"{name}/out{k}", 1e-11)


def _assert_firs(frozen, name, trace):
    for key in ("fir_mid", "fir_side"):
        rc.assert_matches(trace[key], frozen, f"{name}/{key}", 1e-12 * float(frozen[f"{name}/{key}_max_abs"]))


@pytest.mark.parametrize("name", ["cd_rate", "hot_two_rounds", "quiet_reference_custom_limiter"])
def test_oracle_reproduces_the_reference(name, frozen):
    target, reference = _inputs(frozen, name)
    outs, trace = _master(name, target, reference)
    _assert_outputs(frozen, name, outs)
    assert abs(trace["rms_coefficient"] / frozen[name + "/rms_coefficient"] - 1) <= 1e-12
    assert abs(trace["final_amplitude_coefficient"] / frozen[name + "/final_amplitude_coefficient"] - 1) <= 1e-12
    assert np.abs(np.asarray(trace["correction_coefficients"]) / frozen[name + "/correction_coefficients"] - 1).max() <= 1e-11
    _assert_firs(frozen, name, trace)


# ---- the edges of Config the reference itself supports ------------------------------
@pytest.mark.parametrize("fft_size", [8, 16, 32])
def test_smallest_fft_sizes_the_reference_runs(fft_size, frozen):
    """defaults.py:110-112 asks only for a power of two above 1.  8, 16 and 32 run in the reference, so they run here
    (small_fft_kernels.h); the oracle is pinned to the reference there too."""
    name = f"small_fft_{fft_size}"
    target, reference = _inputs(frozen, name)
    outs, _ = _master(name, target, reference)
    _assert_outputs(frozen, name, outs)


@pytest.mark.parametrize("fft_size", [32768, 65536])
def test_largest_fft_sizes_on_the_inputs_of_the_gpu_test(fft_size, frozen):
    """tests/test_gpu_parity.py::test_master_fft_size_32768_and_65536 compares the device with the oracle on exactly this
    pair and configuration (192 kHz, 2 s): here the oracle is held against the unmodified reference on them -- the three
    outputs and the FIR pair (65536 is the largest fft_size libmgx runs; the reference takes any power of two)."""
    name = f"large_fft_{fft_size}"
    target, reference = _inputs(frozen, name)
    outs, trace = _master(name, target, reference)
    _assert_outputs(frozen, name, outs)
    _assert_firs(frozen, name, trace)


@pytest.mark.parametrize("cfg", [dict(fft_size=2), dict(fft_size=4), dict(limiter=dict(hold=0.25)),
                                 dict(limiter=dict(hold=0.05))])
def test_what_the_reference_itself_cannot_run(cfg, frozen):
    """Values that pass the asserts of defaults.py and then fail INSIDE the reference: fft_size 2 and 4 (the cubic
    interp1d of match_frequencies.py:45-58 has too few points) and limiter hold times below three samples
    (hyrax.py:35-40: the sliding window is empty).  libmgx refuses them with MGX_ERR_ARGUMENT; they are not
    gaps against the reference (tests/test_gpu_parity.py::test_fails_loudly_on_unsupported)."""
    target, reference = rc.failing_inputs()
    assert rc.digest(target, reference) == str(frozen["failing/input_sha256"]), "synthetic generator drifted; refreeze"
    name = next(k for k, v in rc.FAILING.items() if v == cfg)
    assert str(frozen["failing/" + name]) != "", "the reference ran this configuration"


def test_more_than_sixteen_correction_steps(frozen):
    name = "twenty_correction_steps"
    target, reference = _inputs(frozen, name)
    outs, trace = _master(name, target, reference)
    want = frozen[name + "/correction_coefficients"]
    assert len(want) == 20
    assert np.abs(np.asarray(trace["correction_coefficients"]) / want - 1).max() <= 1e-11
    _assert_outputs(frozen, name, outs)
