"""Reference sets without a GPU: ``ReferenceProfile.merge``'s refusals before any device is asked for, how ``analyze``,
``process`` and the batch's job files recognise a set of references, and what ``process_batch(share_references=True)``
analyses and merges (``stages.main``, ``_analyze_reference`` and the merge itself replaced by stand-ins, as in
tests/test_profile_host.py, whose forged profiles these are).
"""

import json
import os

import numpy as np
import pytest

import matchering_amd as mg
from conftest import ROOT
from matchering_amd import audio_io
from test_profile_host import make_profile


@pytest.fixture
def no_device(monkeypatch):
    from matchering_amd import device, profile, stages

    def refuse(*args, **kwargs):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(device, "default_device", refuse)
    monkeypatch.setattr(stages, "default_device", refuse)
    monkeypatch.setattr(profile.ReferenceProfile, "resident", refuse)


class FakeMerge:
    """Stands in for ``ReferenceProfile.merge``: records (sources, weights) and answers with a new forged profile."""

    def __init__(self, config):
        self.calls, self.config = [], config

    def __call__(self, profiles, weights=None, device=None):
        self.calls.append((list(profiles), weights))
        return make_profile(self.config, frames=80000 + len(self.calls), seed=50 + len(self.calls))[0]


def test_merge_refuses_before_any_device_is_asked_for(no_device):
    from matchering_amd.profile import ReferenceProfile

    cfg = mg.Config(fft_size=1024, max_piece_size=2.0)
    a, b, c = (make_profile(cfg, seed=s)[0] for s in (1, 2, 3))
    with pytest.raises(ValueError, match="empty"):
        ReferenceProfile.merge([])
    for bad in (0, -1, 1.0, 2.5, "2", True, 65537, None):
        with pytest.raises(ValueError, match="weight"):
            ReferenceProfile.merge([a, b], weights=[1, bad])
    with pytest.raises(ValueError, match="weights"):
        ReferenceProfile.merge([a, b], weights=[1])
    with pytest.raises(TypeError, match="source 1"):
        ReferenceProfile.merge([a, "b.profile"])
    other = make_profile(mg.Config(fft_size=1024, max_piece_size=2.0, threshold=0.9), seed=4)[0]
    with pytest.raises(ValueError, match=r"source 2 .*threshold|threshold.* source 2") as caught:
        ReferenceProfile.merge([a, b, other])
    assert "threshold" in str(caught.value) and "source 2" in str(caught.value)
    with pytest.raises(ValueError, match="fft_size"):
        ReferenceProfile.merge([a, make_profile(mg.Config(fft_size=2048, max_piece_size=2.0))[0], other])   # (the FIRST that differs)
    with pytest.raises(ValueError, match="loud_count"):
        ReferenceProfile.merge([a] * 20000, weights=[65536] * 20000)          # 2 * 65536 * 20000 > 2^31 - 1
    # with everything in order the device is what is asked next
    with pytest.raises(AssertionError, match="a device was asked for"):
        ReferenceProfile.merge([a, b, c], weights=[1, 2, np.int64(65536)])


def test_what_counts_as_a_set():
    from matchering_amd.profile import is_reference_set

    profile, _ = make_profile(mg.Config())
    frames = np.zeros((10, 2), np.float32)
    assert is_reference_set(["a.wav", b"b.wav", profile, frames])
    assert is_reference_set(("a.wav",)) and is_reference_set([profile, profile])
    assert not is_reference_set("a.wav") and not is_reference_set(profile) and not is_reference_set(frames)
    assert not is_reference_set([[0.0, 0.1], [0.2, 0.3]])              # frames as nested lists: one track, as before
    assert not is_reference_set([frames[0], frames[1]])                # ... and as a list of rows
    assert not is_reference_set(["a.wav", 3])


def test_analyze_makes_a_profile_of_every_element_and_merges(tmp_path, monkeypatch, no_device):
    from matchering_amd.profile import ReferenceProfile

    cfg = mg.Config(fft_size=1024, max_piece_size=2.0)
    a, b = (make_profile(cfg, seed=s)[0] for s in (1, 2))
    saved = str(tmp_path / "b.wav")                                    # (a misleading name: the magic decides)
    b.save(saved)
    fake = FakeMerge(cfg)
    monkeypatch.setattr(ReferenceProfile, "merge", staticmethod(fake))
    got = ReferenceProfile.analyze([a, saved], cfg)
    assert len(fake.calls) == 1 and fake.calls[0][0] == [a, b] and fake.calls[0][0][0] is a
    assert isinstance(got, ReferenceProfile) and got.frames == 80001
    foreign = make_profile(mg.Config(fft_size=2048, max_piece_size=2.0))[0]
    with pytest.raises(ValueError, match="fft_size"):
        ReferenceProfile.analyze([a, foreign], cfg)                    # (matches(config), per element)
    foreign.save(saved)
    with pytest.raises(ValueError, match="fft_size"):
        ReferenceProfile.analyze((a, saved), cfg)
    assert len(fake.calls) == 1
    # audio elements go where a single reference goes: to the device (refused here)
    with pytest.raises(AssertionError, match="a device was asked for"):
        ReferenceProfile.analyze([a, np.zeros((5000, 2), np.float32)], cfg)


def test_process_takes_a_set_in_the_references_place(tmp_path, monkeypatch):
    """Only the target is loaded by ``process`` itself; the set's own files go through ``ReferenceProfile.analyze``
    (per element) and ``merge``; ``main`` receives the merged profile; check_equality cannot run and a debug line says so."""
    from matchering_amd import checker, core, intake
    from matchering_amd.profile import ReferenceProfile
    from matchering_amd.synth import make_pair

    rate = 44100
    t, _ = make_pair(3.0, rate, pair=2)
    tp = str(tmp_path / "t.wav")
    audio_io.write_wav(tp, t, rate, "PCM_16")
    cfg = mg.Config(max_piece_size=1.0)
    a, b = (make_profile(cfg, seed=s)[0] for s in (1, 2))
    saved = str(tmp_path / "b.profile")
    b.save(saved)
    fake = FakeMerge(cfg)
    seen, loaded = {}, []

    def fake_main(target, reference, config, need_default=True, need_no_limiter=False, need_no_limiter_normalized=False,
                  encodings=None):
        seen["reference"] = reference
        return np.zeros((target.shape[0], 2), np.float32), None, None

    real_load = intake.load

    def spy_load(path, role, *args, **kwargs):
        loaded.append(role)
        return real_load(path, role, *args, **kwargs)

    def no_equality(*args, **kwargs):
        raise AssertionError("check_equality ran without a reference track")

    monkeypatch.setattr(ReferenceProfile, "merge", staticmethod(fake))
    monkeypatch.setattr(core, "main", fake_main)
    monkeypatch.setattr(core, "_gpu", lambda: None)
    monkeypatch.setattr(intake, "load", spy_load)
    monkeypatch.setattr(intake, "check_equality", no_equality)
    monkeypatch.setattr(checker, "check_equality", no_equality)
    codes, lines = [], []
    mg.log(info_handler=lambda text: codes.append(int(str(text).split(":")[0])), debug_handler=lines.append, show_codes=True)
    try:
        mg.process(tp, [a, saved], [mg.Result(str(tmp_path / "out.wav"), "FLOAT")], config=cfg)
    finally:
        mg.log()
    assert loaded == ["target"] and len(fake.calls) == 1 and fake.calls[0][0] == [a, b]
    assert isinstance(seen["reference"], ReferenceProfile) and seen["reference"].frames == 80001
    assert codes == [2003, 2008, 2010]
    assert any("cannot be checked" in str(line) for line in lines)
    # a set whose profile was made with another Config: refused by name before the target is read
    loaded.clear()
    with pytest.raises(ValueError, match="fft_size"):
        mg.process(tp, (a, saved), [mg.Result(str(tmp_path / "out2.wav"), "FLOAT")], config=mg.Config(fft_size=2048, max_piece_size=1.0))
    assert loaded == []


def test_job_files_take_references(tmp_path):
    from matchering_amd import batch

    results = [{"file": str(tmp_path / "o.wav")}]
    path = str(tmp_path / "jobs.json")
    json.dump([{"target": "a.wav", "references": ["r.wav", "s.profile"], "results": results},
               {"target": "b.wav", "reference": "r.wav", "results": results}], open(path, "w"))
    jobs = batch.jobs_from_json(path)
    assert jobs[0]["references"] == ["r.wav", "s.profile"] and "reference" not in jobs[0] and "reference_profile" not in jobs[0]
    assert jobs[1]["reference"] == "r.wav" and "references" not in jobs[1]
    for named in (dict(reference="r.wav", references=["s.wav"]), dict(reference_profile="r.profile", references=["s.wav"]),
                  dict(reference="r.wav", reference_profile="r.profile", references=["s.wav"]), dict()):
        json.dump([dict(target="a.wav", results=results, **named)], open(path, "w"))
        with pytest.raises(ValueError, match="reference_profile") as caught:
            batch.jobs_from_json(path)
        assert '"references"' in str(caught.value) and "exactly one" in str(caught.value)
    for bad in ([], "r.wav"):
        json.dump([{"target": "a.wav", "references": bad, "results": results}], open(path, "w"))
        with pytest.raises(ValueError, match="references"):
            batch.jobs_from_json(path)


def test_batch_analyses_every_file_once_and_merges_every_set_once(tmp_path, monkeypatch):
    """Two jobs name the overlapping sets {a, b} and {b, c}, a third names b alone, a fourth {a, b} again: with
    share_references=True a, b and c are analysed once each on the one lane, the sets are merged once each, and ``main``
    receives two different merged objects and b's own profile."""
    from matchering_amd import batch
    from matchering_amd.profile import ReferenceProfile
    from matchering_amd.synth import make_pair

    rate = 44100
    cfg = mg.Config(max_piece_size=1.0)
    paths = {}
    for i, name in enumerate(("t0", "t1", "t2", "t3", "a", "b", "c")):
        paths[name] = str(tmp_path / f"{name}.wav")
        audio_io.write_wav(paths[name], make_pair(2.0 + 0.1 * i, rate, pair=i)[0], rate, "PCM_16")
    link = str(tmp_path / "b_again.wav")
    os.symlink(paths["b"], link)
    out = lambda i: [mg.Result(str(tmp_path / f"o{i}.wav"), "FLOAT")]           # noqa: E731
    jobs = [{"target": paths["t0"], "references": [paths["a"], paths["b"]], "results": out(0)},
            {"target": paths["t1"], "references": [link, paths["c"]], "results": out(1)},
            {"target": paths["t2"], "reference": paths["b"], "results": out(2)},
            {"target": paths["t3"], "references": [paths["a"], link], "results": out(3)}]
    own = {os.path.realpath(paths[name]): make_profile(cfg, seed=10 + i)[0] for i, name in enumerate("abc")}
    analysed, seen = [], {}

    def fake_analyze(path, config, device):
        analysed.append(os.path.realpath(path))
        return own[os.path.realpath(path)]

    def fake_main(target, reference, config, need_default=True, need_no_limiter=False, need_no_limiter_normalized=False):
        seen[target.shape[0]] = reference
        return np.zeros((target.shape[0], 2), np.float32), None, None

    fake = FakeMerge(cfg)
    monkeypatch.setattr(batch, "_analyze_reference", fake_analyze)
    monkeypatch.setattr(ReferenceProfile, "merge", staticmethod(fake))
    frames = [audio_io.read_wav(paths[f"t{i}"])[0].shape[0] for i in range(4)]
    a, b, c = (own[os.path.realpath(paths[name])] for name in "abc")
    assert batch.process_batch(jobs, cfg, rank=0, world_size=1, lanes=1, master=fake_main, share_references=True) == [0, 1, 2, 3]
    assert sorted(analysed) == sorted(own)                              # a, b and c: once each
    assert [[id(p) for p in call[0]] for call in fake.calls] == [[id(a), id(b)], [id(b), id(c)]]    # each distinct set once
    got = [seen[n] for n in frames]
    assert all(isinstance(p, ReferenceProfile) for p in got)
    assert got[0] is got[3] and got[0] is not got[1] and got[0] != got[1]
    assert got[2] is b
    assert not any(p is q for p in (got[0], got[1]) for q in (a, b, c))
    # by default nothing is shared: every set job analyses and merges its own, the lone reference keeps the pair route
    analysed.clear(), fake.calls.clear(), seen.clear()
    assert batch.process_batch(jobs, cfg, rank=0, world_size=1, lanes=1, master=fake_main) == [0, 1, 2, 3]
    assert len(analysed) == 6 and len(fake.calls) == 3
    assert isinstance(seen[frames[2]], np.ndarray) and seen[frames[0]] is not seen[frames[3]]
    with pytest.raises(ValueError, match="reference_profile"):
        batch.process_batch([dict(jobs[0], reference=paths["a"])], cfg, rank=0, world_size=1, lanes=1, master=fake_main)


def test_the_example_uses_the_api_as_it_is(monkeypatch, tmp_path):
    """examples/reference_set.py runs up to its GPU calls with arguments those calls accept: three references in one
    ``analyze``, a saved profile, two targets mastered against it."""
    import inspect
    import runpy

    from matchering_amd import core
    from matchering_amd.profile import ReferenceProfile, is_reference_set

    sets, calls = [], []
    profile, _ = make_profile(mg.Config())

    def fake_analyze(reference, config, device=None):
        assert isinstance(config, mg.Config)
        sets.append(reference)
        return profile

    def fake_process(*args, **kwargs):
        bound = inspect.signature(core.process).bind(*args, **kwargs)
        assert all(isinstance(r, mg.Result) for r in bound.arguments["results"])
        calls.append(bound.arguments["reference"])

    monkeypatch.setattr(ReferenceProfile, "analyze", staticmethod(fake_analyze))
    monkeypatch.setattr(mg, "process", fake_process)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr("sys.argv", ["reference_set.py"])
    runpy.run_path(os.path.join(ROOT, "examples", "reference_set.py"), run_name="__main__")
    mg.log()
    assert len(sets) == 1 and is_reference_set(sets[0]) and len(sets[0]) == 3
    assert len(calls) == 2 and all(isinstance(ref, str) and ReferenceProfile.load(ref) == profile for ref in calls)


def test_the_binding_knows_the_merge():
    import ctypes

    from matchering_amd import _native

    lib = _native.library()
    assert lib.mgx_version() >= 103 and _native.PROFILE_MERGE_MAX == 64
    header = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert "#define MGX_PROFILE_MERGE_MAX 64" in header
    # refusals that need no device: a null handle before anything else
    cfg = _native.MgxConfig()
    assert lib.mgx_config_default(ctypes.byref(cfg)) == 0
    one = (ctypes.c_void_p * 1)(4096)
    assert lib.mgx_profile_merge(None, one, None, 1, ctypes.byref(cfg), ctypes.c_void_p(1 << 20)) == _native.ERR_ARGUMENT
