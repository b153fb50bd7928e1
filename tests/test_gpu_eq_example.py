"""examples/matching_eq.py runs as it is written: one pair of files in, three masters out (GPU)."""

import os
import runpy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_matching_eq_example_runs(tmp_path, monkeypatch):
    import matchering_amd as mg
    from conftest import ROOT
    from matchering_amd import audio_io
    from matchering_amd.synth import make_pair

    target, reference = make_pair(4.0, 44100, pair=61, reference_seconds=3.5)
    audio_io.write_wav(str(tmp_path / "target.wav"), target, 44100, "PCM_16")
    audio_io.write_wav(str(tmp_path / "reference.wav"), reference, 44100, "PCM_16")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr("sys.argv", ["matching_eq.py", "target.wav", "reference.wav"])
    lines = []
    monkeypatch.setattr("builtins.print", lambda *a, **k: lines.append(" ".join(str(v) for v in a)))
    try:
        runpy.run_path(os.path.join(ROOT, "examples", "matching_eq.py"), run_name="__main__")
    finally:
        mg.log()                                    # the example installs handlers: put the defaults back
    read = {name: audio_io.read_wav(str(tmp_path / f"{name}.wav"))[0] for name in ("full", "half_capped", "minimum_phase")}
    for audio in read.values():
        assert audio.shape == target.shape and np.abs(audio).max() > 0
    assert not np.array_equal(read["full"], read["half_capped"]) and not np.array_equal(read["full"], read["minimum_phase"])
    assert any("matching EQ: 50 %, +6/−6 dB, linear phase" in line for line in lines)
    assert any("matching EQ: 100 %, no caps, minimum phase" in line for line in lines)
