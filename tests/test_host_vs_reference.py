"""The host-side pieces around the hot path against the UNMODIFIED reference: ``checker.check``
(checker.py:90-142) and ``preview_creator.create_preview`` (preview_creator.py:30-94).  The reference's answers are
frozen by tests/golden/reference_cases.py into tests/golden/reference_cases/, so that the test needs nothing outside
the repository.  Resampling is excluded: the reference delegates it to resampy, which is not installed here
(matchering_amd.checker documents its stand-in)."""

import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import reference_cases as rc             # noqa: E402

import matchering_amd as mg              # noqa: E402


@pytest.fixture(scope="module")
def frozen():
    return rc.load()


@pytest.mark.parametrize("case", rc.CHECK_CASES)
def test_check_matches_the_reference(case, frozen):
    from matchering_amd import checker

    x, name = rc.check_input(case)
    key = f"check/{case}/"
    assert rc.digest(x) == str(frozen[key + "input_sha256"]), "synthetic generator drifted; refreeze"
    got, got_codes, got_err = rc.run_check(checker, mg, x, rc.CHECK_RATE, name, rc.CHECK_CONFIG)
    want_codes, want_err = json.loads(str(frozen[key + "codes"])), json.loads(str(frozen[key + "error"]))
    assert got_err == want_err and got_codes == want_codes
    if key + "rate" in frozen:
        assert got[1] == frozen[key + "rate"]
        assert rc.digest(np.asarray(got[0], np.float64)) == str(frozen[key + "array_sha256"])


@pytest.mark.parametrize("seconds", rc.PREVIEW_SECONDS)
def test_create_preview_matches_the_reference(seconds, monkeypatch, frozen):
    from matchering_amd import preview

    target, result = rc.preview_inputs(seconds)
    key = f"preview/{seconds}/"
    assert rc.digest(target, result) == str(frozen[key + "input_sha256"]), "synthetic generator drifted; refreeze"
    got = rc.run_preview(preview, mg, target, result, rc.PREVIEW_CONFIG, monkeypatch.setattr)
    for name in ("target.wav", "result.wav"):
        rc.assert_matches(got[name], frozen, key + name, 1e-12)
