"""Clip repair without a GPU: what ``mgx_declip_check`` and ``ClipRepair`` refuse, field by field; ``from_json``; that
``stages.main``, ``process`` and a batch refuse a bad ``repair`` before any device or file is touched; and what the
DEFINITION (tests/declip_oracle.py) does to signals whose unclipped form is known.

The readings of ``test_repair_never_hurts_and_often_helps`` (RMS error of the repaired signal over the RMS error of the
clipped one, 1 s at 44.1 kHz, defaults: min_run 2, max_run 32, max_rise 6 dB), level 0.9 / 0.7 / 0.5:
    220 Hz sine     0.016  1.000  1.000     (at 0.7 and 0.5 every run is longer than 32 samples: nothing qualifies)
    1 kHz sine      0.139  0.017  0.079
    five tones      0.173  0.772  0.792
    1/sqrt(f) noise 1.000  0.980  0.788     (at 0.9 one run of three samples, none of them raised)
The highest repaired peak is 1.012 (1 kHz sine at 0.9) against caps of 1.995 times the level: the cap does not bind here.
"""
import ctypes
import math

import numpy as np
import pytest

import declip_oracle as oracle
import matchering_amd as mg
from matchering_amd import _native, stages
from matchering_amd.repair import ClipRepair, Repaired, as_repair

RATE, MAX_RISE = 44100, 10.0 ** (6.0 / 20.0)


def check(level=0.9, max_rise=2.0, min_run=2, max_run=32):
    lib = _native.library()
    rc = lib.mgx_declip_check(ctypes.byref(_native.MgxDeclipParams(level, max_rise, min_run, max_run)))
    return rc, lib.mgx_last_error().decode()


def test_mgx_declip_check_names_the_field():
    lib = _native.library()
    assert check()[0] == 0
    assert check(max_run=512)[0] == 0 and check(min_run=32, max_run=32)[0] == 0 and check(max_rise=1.0)[0] == 0
    assert lib.mgx_declip_check(None) == _native.ERR_ARGUMENT and "params" in lib.mgx_last_error().decode()
    for bad, field in ((dict(level=0.0), "level"), (dict(level=-1.0), "level"), (dict(level=math.nan), "level"),
                       (dict(level=math.inf), "level"), (dict(max_rise=0.99), "max_rise"), (dict(max_rise=math.nan), "max_rise"),
                       (dict(max_rise=math.inf), "max_rise"), (dict(min_run=0), "min_run"), (dict(max_run=513), "max_run"),
                       (dict(min_run=5, max_run=4), "max_run")):
        rc, message = check(**bad)
        assert rc == _native.ERR_ARGUMENT and message.startswith(field), (bad, rc, message)


def test_clip_repair_refuses_in_the_librarys_words():
    assert ClipRepair().check() == ClipRepair()
    assert ClipRepair(level=0.5, max_run=512, max_rise_db=0.0).check()
    for bad, field in ((dict(level=0.0), "level"), (dict(level=math.nan), "level"), (dict(relative_db=0.5), "relative_db"),
                       (dict(relative_db=math.nan), "relative_db"), (dict(min_run=0), "min_run"), (dict(min_run=2.5), "min_run"),
                       (dict(max_run=513), "max_run"), (dict(min_run=40), "max_run"), (dict(max_rise_db=-1.0), "max_rise"),
                       (dict(max_rise_db=math.inf), "max_rise"), (dict(max_rise_db=1e6), "max_rise")):
        with pytest.raises(ValueError, match="^" + field):
            ClipRepair(**bad).check()
    assert ClipRepair(relative_db=0.0).check().level_for(0.5) == 0.5
    assert ClipRepair(level=0.25).level_for(0.9) == 0.25
    assert ClipRepair().level_for(1.0) == 10.0 ** (-0.1 / 20.0)
    # both rails of 16-bit PCM lie at or above the default level of a full-scale file
    assert 32767 / 32768 >= ClipRepair().level_for(1.0)
    native = ClipRepair(max_rise_db=6.0).native(0.8)
    assert native.max_rise == MAX_RISE and (native.min_run, native.max_run) == (2, 32)


def test_from_json_and_the_forms_of_repair():
    assert ClipRepair.from_json(True) == ClipRepair() and ClipRepair.from_json(None) is None
    assert ClipRepair.from_json(False) is None and as_repair(False) == (None, None)
    assert ClipRepair.from_json({"max_run": 16, "level": 0.9}) == ClipRepair(level=0.9, max_run=16)
    with pytest.raises(ValueError, match=r"unknown keys \['maxrun'\]"):
        ClipRepair.from_json({"maxrun": 16})
    with pytest.raises(ValueError, match="true or an object"):
        ClipRepair.from_json([1, 2])
    assert as_repair(None) == (None, None) and as_repair(True) == (None, ClipRepair())
    handler = lambda name, value: None                                      # noqa: E731
    assert as_repair((handler, {"min_run": 3})) == (handler, ClipRepair(min_run=3))
    with pytest.raises(ValueError, match="callable"):
        as_repair((3, ClipRepair()))
    found = Repaired(0.9, 100, runs_repaired=(2, 1), samples_repaired=(9, 4), longest_repaired=(5, 4), peak_before=(0.9, 0.9),
                     peak_after=(1.0, 0.95))
    assert found.as_dict()["runs_repaired"] == [2, 1] and found.as_dict()["level"] == 0.9
    assert "3 runs" in found.describe() and "\n" not in found.describe()
    assert "silent" in Repaired(0.0, 10).describe()
    assert mg.ClipRepair is ClipRepair and mg.Repaired is Repaired and callable(mg.repair_clipping)


class NoDevice:
    """Stands where a device would: touching it is the failure."""

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched ({name}) before the repair was refused")


def test_a_bad_repair_is_refused_before_a_device_or_a_file_is_touched(tmp_path):
    x = np.zeros((64, 2), dtype=np.float32)
    with pytest.raises(ValueError, match="^max_run"):
        stages.main(x, x, mg.Config(), device=NoDevice(), repair=ClipRepair(max_run=600))
    with pytest.raises(ValueError, match="unknown keys"):
        stages.main(x, x, mg.Config(), device=NoDevice(), repair={"run": 3})
    missing = str(tmp_path / "no_such_file.wav")
    with pytest.raises(ValueError, match="^level"):
        mg.process(missing, missing, [mg.pcm16(str(tmp_path / "out.wav"))], repair=ClipRepair(level=-1.0))
    job = {"target": missing, "reference": missing, "results": [mg.pcm16(str(tmp_path / "out.wav"))], "repair": {"min_run": 0}}
    with pytest.raises(ValueError, match="^min_run"):
        mg.process_batch([job], rank=0, world_size=1, master=lambda *a, **k: pytest.fail("mastered"))
    with pytest.raises(ValueError, match="^max_rise"):
        mg.process_batch([dict(job, repair=None)], rank=0, world_size=1, master=lambda *a, **k: pytest.fail("mastered"),
                         repair=ClipRepair(max_rise_db=-3.0))
    with pytest.raises(ValueError, match="^max_run"):
        mg.master_many([(x, x)], master=lambda *a, **k: pytest.fail("mastered"), repair={"max_run": 0})


def test_a_batch_job_file_validates_its_repair(tmp_path):
    import json

    from matchering_amd.batch import jobs_from_json

    item = {"target": "t.wav", "reference": "r.wav", "results": [{"file": "o.wav"}]}
    path = tmp_path / "jobs.json"
    path.write_text(json.dumps([dict(item, repair=True), dict(item, repair={"max_run": 64}), item, dict(item, repair=False)]))
    jobs = jobs_from_json(str(path))
    assert jobs[0]["repair"] == ClipRepair() and jobs[1]["repair"] == ClipRepair(max_run=64) and "repair" not in jobs[2]
    assert jobs[3]["repair"] is False                    # (kept: the job's way out of a batch-wide repair)
    path.write_text(json.dumps([dict(item, repair={"max_run": 1000})]))
    with pytest.raises(ValueError, match="^max_run"):
        jobs_from_json(str(path))
    path.write_text(json.dumps([dict(item, repair={"longest": 3})]))
    with pytest.raises(ValueError, match="unknown keys"):
        jobs_from_json(str(path))


# ---- the definition on signals whose unclipped form is known ------------------------------------------------------------
def signals():
    t = np.arange(RATE) / RATE
    rng = np.random.default_rng(5)
    phases = rng.uniform(0, 6, 5)
    tones = sum(a * np.sin(2 * np.pi * f * t + p)
                for f, a, p in zip((110, 331, 523, 1480, 3100), (1, .6, .4, .3, .2), phases))
    spectrum = np.fft.rfft(rng.standard_normal(RATE))
    hz = np.fft.rfftfreq(RATE, 1.0 / RATE)
    spectrum[1:] /= np.sqrt(hz[1:])
    spectrum[0] = 0.0
    spectrum[hz > 8000.0] = 0.0
    named = {"sine220": np.sin(2 * np.pi * 220 * t), "sine1k": np.sin(2 * np.pi * 1000 * t), "tones": tones,
             "noise": np.fft.irfft(spectrum, RATE)}
    return {name: x / np.max(np.abs(x)) for name, x in named.items()}


@pytest.fixture(scope="module")
def ratios():
    """(signal, level) -> (error of the repaired signal / error of the clipped one, runs repaired, peak after)"""
    out = {}
    for name, clean in signals().items():
        for level in (0.9, 0.7, 0.5):
            lam = np.float32(level)
            clipped = np.clip(clean, -float(lam), float(lam)).astype(np.float32)
            repaired, report = oracle.declip_channel(clipped, float(lam), 2, 32, MAX_RISE)
            rms = lambda y: float(np.sqrt(np.mean((y.astype(np.float64) - clean) ** 2)))       # noqa: E731
            out[name, level] = (rms(repaired) / rms(clipped), report["runs_repaired"], report["peak_after"])
            print(name, level, "ratio %.3f" % out[name, level][0], report)
    return out


def test_repair_never_hurts_and_often_helps(ratios):
    for key, (ratio, runs, peak) in ratios.items():
        assert ratio <= 1.0, (key, ratio)
        assert peak <= float(np.float32(MAX_RISE * float(np.float32(key[1])))), (key, peak)
    assert ratios["sine220", 0.7][1] == 0 and ratios["sine220", 0.7][0] == 1.0          # no run qualifies: a copy
    for key in (("sine1k", 0.7), ("sine1k", 0.5), ("tones", 0.9)):
        assert ratios[key][1] > 0 and ratios[key][0] <= 0.5, (key, ratios[key])
