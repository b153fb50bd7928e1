"""examples/tone_controls.py runs as it is written: one pair of files in, three toned masters out (GPU)."""

import os
import runpy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_tone_controls_example_runs(tmp_path, monkeypatch):
    import matchering_amd as mg
    from conftest import ROOT
    from matchering_amd import audio_io
    from matchering_amd.synth import make_pair

    target, reference = make_pair(4.0, 44100, pair=62, reference_seconds=3.5)
    audio_io.write_wav(str(tmp_path / "target.wav"), target, 44100, "PCM_16")
    audio_io.write_wav(str(tmp_path / "reference.wav"), reference, 44100, "PCM_16")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr("sys.argv", ["tone_controls.py", "target.wav", "reference.wav"])
    lines = []
    monkeypatch.setattr("builtins.print", lambda *a, **k: lines.append(" ".join(str(v) for v in a)))
    try:
        runpy.run_path(os.path.join(ROOT, "examples", "tone_controls.py"), run_name="__main__")
    finally:
        mg.log()                                    # the example installs handlers: put the defaults back
    names = ("range_image_kept", "mono_bass", "air_and_tilt")
    read = {name: audio_io.read_wav(str(tmp_path / f"{name}.wav"))[0] for name in names}
    for audio in read.values():
        assert audio.shape == target.shape and np.abs(audio).max() > 0
    assert all(not np.array_equal(read[a], read[b]) for a in names for b in names if a < b)
    assert any("matching EQ: 100 %, no caps, linear phase, 60 Hz – 12 kHz, side 0 %" in line for line in lines)
    assert any("linear phase, mono below 120 Hz" in line for line in lines)
    assert any("tilt −0.3 dB/oct, 1 band" in line for line in lines)
    assert sum("side gate" in line for line in lines) == 18
