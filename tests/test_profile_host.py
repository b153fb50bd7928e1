"""Reference profiles without a GPU: the size and layout of the block (include/mgx.h against the ctypes mirror and the
C compiler), the saved file, ``ReferenceProfile.matches``, and the host glue of ``core.process`` and the batch's job
files with a profile in the reference's place (``stages.main`` replaced by a stand-in, as in tests/test_host_api.py).
"""

import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import matchering_amd as mg
from conftest import ROOT
from matchering_amd import _native, audio_io


def make_profile(config, frames=70000, seed=3):
    """A profile as the device would pack it for ``config``, built on the host from made-up analysis results."""
    from matchering_amd.profile import ReferenceProfile

    rng = np.random.RandomState(seed)
    header = _native.MgxProfileHeader(
        magic=_native.PROFILE_MAGIC, version=_native.PROFILE_VERSION, internal_sample_rate=config.internal_sample_rate,
        fft_size=config.fft_size, max_piece_size=float(config.max_piece_size), threshold=float(config.threshold),
        min_value=float(config.min_value), frames=frames, piece=frames // 3, divisions=3, loud_count=2, peak=0.71,
        amplitude_coefficient=0.71 / config.threshold, average_rms=0.11, match_rms=0.13)
    spectra = np.abs(rng.randn(2, config.fft_size // 2 + 1)) * 1e-3
    return ReferenceProfile(bytes(header) + spectra.astype("<f8").tobytes()), spectra


@pytest.mark.parametrize("fft", [8, 4096, 65536])
def test_profile_bytes_needs_no_gpu(fft):
    lib = _native.library()
    cfg = _native.MgxConfig()
    assert lib.mgx_config_default(ctypes.byref(cfg)) == 0
    cfg.fft_size = fft
    n = ctypes.c_size_t()
    assert lib.mgx_profile_bytes(ctypes.byref(cfg), ctypes.byref(n)) == 0
    assert n.value == ctypes.sizeof(_native.MgxProfileHeader) + 2 * (fft // 2 + 1) * 8
    cfg.fft_size = 3000
    assert lib.mgx_profile_bytes(ctypes.byref(cfg), ctypes.byref(n)) == -1 and b"fft_size" in lib.mgx_last_error()
    assert lib.mgx_profile_bytes(None, ctypes.byref(n)) == -1
    assert lib.mgx_version() >= 102


def test_profile_header_layout_matches_the_c_compiler(tmp_path):
    fields = [name for name, _ in _native.MgxProfileHeader._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mgx.h"\n'
                   'int main(void) { printf("%zu %u %u", sizeof(mgx_profile_header), MGX_PROFILE_MAGIC, MGX_PROFILE_VERSION);\n'
                   + "".join(f'  printf(" %zu", offsetof(mgx_profile_header, {name}));\n' for name in fields)
                   + '  printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    c = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert c[0] == ctypes.sizeof(_native.MgxProfileHeader) == 96
    assert (c[1], c[2]) == (_native.PROFILE_MAGIC, _native.PROFILE_VERSION)
    assert c[3:] == [getattr(_native.MgxProfileHeader, name).offset for name in fields]


def test_save_and_load_round_trip_and_refusals(tmp_path):
    from matchering_amd.profile import FILE_MAGIC, ReferenceProfile, is_profile_file

    cfg = mg.Config(fft_size=1024, max_piece_size=2.0)
    profile, spectra = make_profile(cfg)
    path = str(tmp_path / "reference.anything")            # (recognised by its magic, not by its name)
    profile.save(path)
    assert is_profile_file(path) and os.path.getsize(path) == len(FILE_MAGIC) + 96 + 2 * 513 * 8
    back = ReferenceProfile.load(path)
    assert back == profile and back.tobytes() == profile.tobytes()
    assert np.array_equal(back.spectra, spectra) and back.match_rms == 0.13 and back.loud_count == 2
    assert (back.frames, back.divisions, back.piece) == (70000, 3, 70000 // 3)
    with pytest.raises(AttributeError):
        back.match_rms = 1.0                                # read-only
    data = open(path, "rb").read()
    short = str(tmp_path / "short")
    open(short, "wb").write(data[:-40])
    with pytest.raises(ValueError, match="truncated"):
        ReferenceProfile.load(short)
    stub = str(tmp_path / "stub")
    open(stub, "wb").write(data[:30])
    with pytest.raises(ValueError, match="not a reference profile"):
        ReferenceProfile.load(stub)
    wav = str(tmp_path / "audio.wav")
    audio_io.write_wav(wav, np.zeros((100, 2), np.float32), 44100, "PCM_16")
    assert not is_profile_file(wav) and not is_profile_file(str(tmp_path / "missing"))
    with pytest.raises(ValueError, match="not a saved reference profile"):
        ReferenceProfile.load(wav)
    forged = bytearray(profile.tobytes())
    forged[4] = 9                                           # another layout version
    with pytest.raises(ValueError, match="version"):
        ReferenceProfile(bytes(forged))


@pytest.mark.parametrize("field, other", [("fft_size", dict(fft_size=2048)), ("threshold", dict(threshold=0.9)),
                                          ("max_piece_size", dict(max_piece_size=2.5)), ("min_value", dict(min_value=1e-5)),
                                          ("internal_sample_rate", dict(internal_sample_rate=48000))])
def test_matches_names_the_field_that_differs(field, other):
    base = dict(fft_size=1024, max_piece_size=2.0)
    profile, _ = make_profile(mg.Config(**base))
    assert profile.matches(mg.Config(**base))
    assert profile.matches(mg.Config(rms_correction_steps=7, lowess_frac=0.05, **base))      # (not what the analysis reads)
    with pytest.raises(ValueError, match=field):
        profile.matches(mg.Config(**dict(base, **other)))


def test_stages_main_refuses_a_foreign_profile_before_any_launch(monkeypatch):
    from matchering_amd import stages

    profile, _ = make_profile(mg.Config(fft_size=1024, max_piece_size=2.0))

    def no_device(*args, **kwargs):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(stages, "default_device", no_device)
    with pytest.raises(ValueError, match="fft_size"):
        stages.main(np.zeros((50000, 2), np.float32), profile, mg.Config(max_piece_size=2.0), device=object())


@pytest.mark.parametrize("how", ["object", "saved file"])
def test_process_passes_a_profile_through(tmp_path, monkeypatch, how):
    """core.process with a profile in the reference's place: only the target is loaded and checked, check_equality is
    not called (and a debug line says so), the profile reaches ``main`` as it is, the log codes keep their order."""
    from matchering_amd import checker, core, intake
    from matchering_amd.profile import ReferenceProfile
    from matchering_amd.synth import make_pair

    rate = 44100
    t, _ = make_pair(3.0, rate, pair=2)
    tp = str(tmp_path / "t.wav")
    audio_io.write_wav(tp, t, rate, "PCM_16")
    cfg = mg.Config(max_piece_size=1.0)
    profile, _ = make_profile(cfg)
    given = profile
    if how == "saved file":
        given = str(tmp_path / "reference.wav")             # (a misleading name: the magic decides)
        profile.save(given)
    seen = {}

    def fake_main(target, reference, config, need_default=True, need_no_limiter=False, need_no_limiter_normalized=False,
                  encodings=None):
        seen["reference"] = reference
        seen["target_frames"] = target.shape[0]
        return np.zeros((target.shape[0], 2), np.float32), None, None

    loaded = []
    real_load = intake.load

    def spy_load(path, role, *args, **kwargs):
        loaded.append(role)
        return real_load(path, role, *args, **kwargs)

    def no_equality(*args, **kwargs):
        raise AssertionError("check_equality ran without a reference track")

    monkeypatch.setattr(core, "main", fake_main)
    monkeypatch.setattr(core, "_gpu", lambda: None)
    monkeypatch.setattr(intake, "load", spy_load)
    monkeypatch.setattr(intake, "check_equality", no_equality)
    monkeypatch.setattr(checker, "check_equality", no_equality)
    codes, lines = [], []
    mg.log(info_handler=lambda text: codes.append(int(str(text).split(":")[0])), debug_handler=lines.append,
           show_codes=True)
    try:
        mg.process(tp, given, [mg.Result(str(tmp_path / "out.wav"), "FLOAT")], config=cfg)
    finally:
        mg.log()
    assert loaded == ["target"]
    assert isinstance(seen["reference"], ReferenceProfile) and seen["reference"] == profile
    assert seen["target_frames"] == t.shape[0]
    assert codes == [2003, 2008, 2010]                      # (2004-2007 come from stages.main, replaced here)
    assert any("cannot be checked" in str(line) for line in lines)
    # a profile made with another Config: refused by name before the target is even read
    loaded.clear()
    with pytest.raises(ValueError, match="fft_size"):
        mg.process(tp, given, [mg.Result(str(tmp_path / "out2.wav"), "FLOAT")], config=mg.Config(fft_size=2048, max_piece_size=1.0))
    assert loaded == []


def test_job_files_take_a_reference_profile(tmp_path):
    from matchering_amd import batch

    results = [{"file": str(tmp_path / "o.wav")}]
    path = str(tmp_path / "jobs.json")
    json.dump([{"target": "a.wav", "reference": "r.wav", "results": results},
               {"target": "b.wav", "reference_profile": "r.profile", "results": results}], open(path, "w"))
    jobs = batch.jobs_from_json(path)
    assert jobs[0]["reference"] == "r.wav" and "reference_profile" not in jobs[0]
    assert jobs[1]["reference_profile"] == "r.profile" and "reference" not in jobs[1]
    assert all(isinstance(r, mg.Result) for job in jobs for r in job["results"])
    json.dump([{"target": "a.wav", "reference": "r.wav", "reference_profile": "r.profile", "results": results}], open(path, "w"))
    with pytest.raises(ValueError, match="reference_profile"):
        batch.jobs_from_json(path)
    json.dump([{"target": "a.wav", "results": results}], open(path, "w"))
    with pytest.raises(ValueError, match="reference_profile"):
        batch.jobs_from_json(path)


def test_batch_masters_profile_jobs_and_shares_reference_files(tmp_path, monkeypatch):
    """process_batch with a stand-in for the GPU: a job with a "reference_profile" hands the profile to ``main`` without
    loading a reference; with share_references=True the jobs that name one reference file have it analysed once per lane
    and receive that profile, a job with a reference of its own keeps the pair route; by default nothing is shared."""
    from matchering_amd import batch
    from matchering_amd.profile import ReferenceProfile
    from matchering_amd.synth import make_pair

    rate = 44100
    cfg = mg.Config(max_piece_size=1.0)
    profile, _ = make_profile(cfg)
    saved = str(tmp_path / "saved.profile")
    profile.save(saved)
    paths = {}
    for i, name in enumerate(("t0", "t1", "t2", "t3", "shared", "own")):
        paths[name] = str(tmp_path / f"{name}.wav")
        audio_io.write_wav(paths[name], make_pair(2.0 + 0.1 * i, rate, pair=i)[0], rate, "PCM_16")
    link = str(tmp_path / "shared_again.wav")
    os.symlink(paths["shared"], link)                       # (the same file under another name: os.path.samefile)
    jobs = [{"target": paths["t0"], "reference": paths["shared"], "results": [mg.Result(str(tmp_path / "o0.wav"), "FLOAT")]},
            {"target": paths["t1"], "reference": link, "results": [mg.Result(str(tmp_path / "o1.wav"), "FLOAT")]},
            {"target": paths["t2"], "reference": paths["own"], "results": [mg.Result(str(tmp_path / "o2.wav"), "FLOAT")]},
            {"target": paths["t3"], "reference_profile": saved, "results": [mg.Result(str(tmp_path / "o3.wav"), "FLOAT")]}]
    seen = {}

    def fake_main(target, reference, config, need_default=True, need_no_limiter=False, need_no_limiter_normalized=False):
        seen[target.shape[0]] = reference
        return np.zeros((target.shape[0], 2), np.float32), None, None

    analysed = []

    def fake_analyze(path, config, device):
        analysed.append(os.path.realpath(path))
        return profile

    monkeypatch.setattr(batch, "_analyze_reference", fake_analyze)
    frames = [audio_io.read_wav(paths[f"t{i}"])[0].shape[0] for i in range(4)]
    assert batch.process_batch(jobs, cfg, rank=0, world_size=1, lanes=1, master=fake_main) == [0, 1, 2, 3]
    assert analysed == []                                    # the default: every job loads its own reference
    assert all(isinstance(seen[frames[i]], np.ndarray) for i in range(3))
    assert isinstance(seen[frames[3]], ReferenceProfile) and seen[frames[3]] == profile
    seen.clear()
    assert batch.process_batch(jobs, cfg, rank=0, world_size=1, lanes=1, master=fake_main, share_references=True) == [0, 1, 2, 3]
    assert analysed == [os.path.realpath(paths["shared"])]   # once for the two jobs, on the one lane
    assert seen[frames[0]] is profile and seen[frames[1]] is profile
    assert isinstance(seen[frames[2]], np.ndarray)           # a reference nobody shares: the pair route
    assert seen[frames[3]] == profile
    with pytest.raises(ValueError, match="reference_profile"):
        batch.process_batch([dict(jobs[0], reference_profile=saved)], cfg, rank=0, world_size=1, lanes=1, master=fake_main)


def test_the_example_uses_the_api_as_it_is(monkeypatch, tmp_path):
    """examples/reference_profile.py runs up to its GPU calls with arguments those calls accept."""
    import inspect
    import runpy

    from matchering_amd import core
    from matchering_amd.profile import ReferenceProfile

    cfg_seen, calls = [], []
    profile, _ = make_profile(mg.Config())

    def fake_analyze(reference, config, device=None):
        cfg_seen.append(config)
        return profile

    def fake_process(*args, **kwargs):
        bound = inspect.signature(core.process).bind(*args, **kwargs)
        assert all(isinstance(r, mg.Result) for r in bound.arguments["results"])
        calls.append(bound.arguments["reference"])

    monkeypatch.setattr(ReferenceProfile, "analyze", staticmethod(fake_analyze))
    monkeypatch.setattr(mg, "process", fake_process)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr("sys.argv", ["reference_profile.py"])
    runpy.run_path(os.path.join(ROOT, "examples", "reference_profile.py"), run_name="__main__")
    mg.log()
    assert len(cfg_seen) == 1 and len(calls) == 2
    assert all(isinstance(ref, str) and ReferenceProfile.load(ref) == profile for ref in calls)
