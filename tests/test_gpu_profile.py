"""Reference profiles on the GPU (include/mgx.h: mgx_reference_profile / mgx_master_with_profile; profile.py): a
reference analysed once, then targets mastered against the profile without the reference's audio.

Bounds are the project's own: 1e-5 RMS for outputs (RMS_TOL of tests/test_gpu_parity.py), 1e-6 of the peak tap for the
FIR pair and 1e-6 relative for the report's scalars (test_fir_and_stage_scalars_match_reference_golden), 1e-7 / 2e-6 of
the spectrum's peak for the analysis (test_analysis_stage).  The profile route may differ from the pair route only in the
order of the float64 sums on the reference's side.
"""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import mastering_oracle as mo
from cases import CASES, build_inputs, oracle_params
from conftest import ROOT, rms_error

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-5


def make_config(case_cfg):
    import matchering_amd as mg

    kw = dict(case_cfg)
    lim = kw.pop("limiter", None)
    if lim is not None:
        kw["limiter"] = mg.LimiterConfig(**lim)
    return mg.Config(**kw)


@pytest.fixture(scope="module")
def runs():
    """name -> (target, reference, oracle outputs, oracle trace, Config, profile), computed once and left unchanged."""
    from matchering_amd import ReferenceProfile

    cache = {}

    def run(name):
        if name not in cache:
            t, r = build_inputs(CASES[name])
            tr = {}
            outs = mo.master(t, r, oracle_params(CASES[name]["config"]), True, True, True, trace=tr)
            cfg = make_config(CASES[name]["config"])
            cache[name] = (t, r, outs, tr, cfg, ReferenceProfile.analyze(r, cfg))
        return cache[name]

    return run


def master_on_device(t, cfg, reference=None, profile=None, device=None):
    """Device.master through either route: (report, [three outputs], FIR pair)."""
    from matchering_amd._native import check, library
    from matchering_amd.device import default_device

    dev = device or default_device()
    with dev.lock:
        td = dev.upload(t)
        rd = dev.upload(reference) if reference is not None else None
        pd = profile.resident(dev) if profile is not None else None
        outs = [dev.alloc(t.shape[0] * 8) for _ in range(3)]
        try:
            rep = dev.master(td, t.shape[0], rd, 0 if rd is None else reference.shape[0], cfg.to_native(), *outs, profile=pd)
            taps_dev, taps = ctypes.c_void_p(), ctypes.c_int32()
            check(library().mgx_last_fir(dev.handle, ctypes.byref(taps_dev), ctypes.byref(taps)))
            assert taps.value == cfg.fft_size
            fir = np.array(dev.download(int(taps_dev.value), (2, taps.value)))
            res = [np.array(dev.download(o, (t.shape[0], 2))) for o in outs]
        finally:
            for b in (td, rd, *outs):
                if b is not None:
                    b.release()
    return rep, res, fir


# ---- 1. golden parity of the route --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_profile_route_matches_reference_golden(name, golden, runs):
    from matchering_amd import stages

    g = golden(name)
    t, r, outs, tr, cfg, profile = runs(name)
    res, res_nl, res_nln = stages.main(t, profile, cfg, True, True, True)
    assert res.dtype == np.float32 and res.shape == t.shape
    assert rms_error(res, g["result_f32"]) <= RMS_TOL
    assert rms_error(res_nl, g["result_no_limiter_f32"]) <= RMS_TOL
    idx = g["sparse_index"]
    assert rms_error(res_nln[idx], g["result_no_limiter_normalized_sparse"]) <= RMS_TOL
    for mine, want in zip((res, res_nl, res_nln), outs):
        assert rms_error(mine, want) <= RMS_TOL
        assert np.abs(mine - want).max() <= 2e-5 * max(1.0, np.abs(want).max())
    assert np.abs(res).max() <= cfg.threshold * tr["final_amplitude_coefficient"] * (1 + 1e-6)


@pytest.mark.parametrize("name", sorted(CASES))
def test_profile_route_fir_and_scalars_match_reference_golden(name, golden, runs):
    g = golden(name)
    t, r, _, _, cfg, profile = runs(name)
    rep, _, fir = master_on_device(t, cfg, profile=profile)
    for mine, want in ((fir[0], g["fir_mid"]), (fir[1], g["fir_side"])):
        assert np.abs(mine - want).max() <= 1e-6 * np.abs(want).max()
    rel = lambda a, b: abs(a / b - 1.0)                                          # noqa: E731
    assert rel(rep.rms_coefficient, float(g["rms_coefficient"])) <= 1e-6
    assert rel(rep.final_amplitude_coefficient, float(g["final_amplitude_coefficient"])) <= 1e-6
    assert rel(rep.target_match_rms, float(g["target_match_rms"])) <= 1e-6
    assert rel(rep.reference_match_rms, float(g["reference_match_rms"])) <= 1e-6
    steps = cfg.rms_correction_steps
    got = np.array(rep.correction_coefficients[:steps])
    assert got.shape == g["correction_coefficients"].shape
    assert np.abs(got / g["correction_coefficients"] - 1.0).max() <= 1e-6
    assert rel(rep.normalize_coefficient, float(g["normalize_coefficient"])) <= 1e-6
    assert (rep.target_divisions, rep.reference_divisions) == (int(g["target_divisions"]), int(g["reference_divisions"]))
    assert (rep.target_piece, rep.reference_piece) == (int(g["target_piece"]), int(g["reference_piece"]))
    assert (rep.target_loud_count, rep.reference_loud_count) == (int(g["target_loud_count"]), int(g["reference_loud_count"]))
    assert bool(rep.limiter_active) == bool(g["limiter_active"])


# ---- 2. what a profile holds ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_profile_contents(name, runs):
    from matchering_amd import kernels
    from matchering_amd.profile import profile_bytes

    t, r, _, tr, cfg, profile = runs(name)
    assert len(profile.tobytes()) == profile_bytes(cfg)
    assert (profile.internal_sample_rate, profile.fft_size) == (cfg.internal_sample_rate, cfg.fft_size)
    assert (profile.max_piece_size, profile.threshold, profile.min_value) == (cfg.max_piece_size, cfg.threshold, cfg.min_value)
    assert profile.matches(cfg)
    assert profile.frames == r.shape[0]
    assert (profile.divisions, profile.piece) == (tr["reference_divisions"], tr["reference_piece"])
    assert profile.loud_count == len(tr["reference_loud_idx"])
    assert abs(profile.amplitude_coefficient - tr["final_amplitude_coefficient"]) <= 1e-7
    assert abs(profile.match_rms / tr["reference_match_rms"] - 1) <= 1e-7
    spectra = profile.spectra
    for mine, want in ((spectra[0], tr["mid"].avg_reference), (spectra[1], tr["side"].avg_reference)):
        assert np.abs(mine - want).max() <= 2e-6 * want.max()
    # the same kernel chain as mgx_analyze(is_reference = 1): bit for bit
    st = kernels.analyze(r, cfg, is_reference=True)
    assert profile.match_rms == st.match_rms and profile.amplitude_coefficient == st.amplitude_coefficient
    assert profile.peak == st.peak
    assert np.array_equal(spectra[0], st.average_spectrum_mid) and np.array_equal(spectra[1], st.average_spectrum_side)


# ---- 3. against the pair route ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cd_default", "quiet_reference"])
def test_profile_route_against_the_pair_route(name, runs):
    t, r, _, _, cfg, profile = runs(name)
    rep_p, res_p, fir_p = master_on_device(t, cfg, reference=r)
    rep_q, res_q, fir_q = master_on_device(t, cfg, profile=profile)
    tap_diff = np.abs(fir_q - fir_p).max() / np.abs(fir_p).max()
    out_diff = [rms_error(a, b) for a, b in zip(res_q, res_p)]
    print(f"{name}: profile route vs pair route: taps {tap_diff:.3e} of the peak tap, outputs rms {max(out_diff):.3e}, "
          f"max {max(float(np.abs(a - b).max()) for a, b in zip(res_q, res_p)):.3e}")
    assert tap_diff <= 1e-6
    assert max(out_diff) <= RMS_TOL
    # the target's half runs the pair route's arithmetic in the pair route's order
    assert rep_q.target_match_rms == rep_p.target_match_rms
    assert (rep_q.target_divisions, rep_q.target_piece, rep_q.target_loud_count) == \
           (rep_p.target_divisions, rep_p.target_piece, rep_p.target_loud_count)
    assert rep_q.reference_match_rms == rep_p.reference_match_rms
    assert rep_q.final_amplitude_coefficient == rep_p.final_amplitude_coefficient


# ---- 4. edges of the curve kernel ---------------------------------------------------------------------------------------
# 8 kHz, a few seconds.  Bins = fft_size / 2 + 1: 5 (less than a tile), 33, 2049 (in tiles of 32: a last tile of one
# bin) and 8193 (a last tile of one bin in tiles of 32, of nine in tiles of 33, whichever the chip's CU count picks); piece counts of 1 against 5 and 5 against 1; a reference shorter and longer than the target;
# rms_correction_steps 0 and 1 (k_finalize_scalars / the single round that is first and last).
EDGES = {
    "fft8": dict(seconds=2.0, reference_seconds=1.7, config=dict(fft_size=8, max_piece_size=0.5)),
    "fft64": dict(seconds=2.0, reference_seconds=1.7, config=dict(fft_size=64, max_piece_size=0.5)),
    "fft4096": dict(seconds=2.0, reference_seconds=1.7, config=dict(fft_size=4096, max_piece_size=1.0)),
    "fft16384": dict(seconds=4.5, reference_seconds=5.5, config=dict(fft_size=16384, max_piece_size=3.0)),
    "one_piece_against_many": dict(seconds=2.0, reference_seconds=12.0, config=dict(fft_size=512, max_piece_size=2.5)),
    "many_pieces_against_one": dict(seconds=12.0, reference_seconds=2.0, config=dict(fft_size=512, max_piece_size=2.5)),
    "reference_shorter": dict(seconds=2.0, reference_seconds=1.3, config=dict(fft_size=512, max_piece_size=0.5)),
    "reference_longer": dict(seconds=2.0, reference_seconds=3.1, config=dict(fft_size=512, max_piece_size=0.5)),
    "no_correction_rounds": dict(seconds=2.0, reference_seconds=1.7,
                                 config=dict(fft_size=512, max_piece_size=0.5, rms_correction_steps=0)),
    "one_correction_round": dict(seconds=2.0, reference_seconds=1.7,
                                 config=dict(fft_size=512, max_piece_size=0.5, rms_correction_steps=1)),
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_curve_kernel_edges(name):
    import matchering_amd as mg
    from matchering_amd import ReferenceProfile, stages
    from matchering_amd.synth import make_pair

    edge = EDGES[name]
    kw = dict(internal_sample_rate=8000, **edge["config"])
    t, r = make_pair(edge["seconds"], 8000, pair=sorted(EDGES).index(name), reference_seconds=edge["reference_seconds"])
    cfg = mg.Config(**kw)
    tr = {}
    want = mo.master(t, r, mo.params(**kw), True, True, True, trace=tr)
    profile = ReferenceProfile.analyze(r, cfg)
    assert (profile.divisions, profile.loud_count) == (tr["reference_divisions"], len(tr["reference_loud_idx"]))
    got = stages.main(t, profile, cfg, True, True, True)
    errs = [rms_error(a, b) for a, b in zip(got, want)]
    print(name, "rms errors vs oracle", errs)
    assert max(errs) <= RMS_TOL


# ---- 5. piece tables beyond a workgroup's LDS ---------------------------------------------------------------------------
# 8 kHz, fft_size 8, pieces of 9 frames.  "issue": 5001 target pieces -- 188 KB in the PAIR kernel's carve with no
# reference rows, 125 KB in k_profile_curve's own, which therefore still runs it in one launch.  "own_carve": 6201 target
# pieces, 152 KB in k_profile_curve's carve, above the 150 KB a workgroup gets: k_levels + k_average_spectra +
# k_profile_raw (and the most the level-correction tail's own LDS admits, 6378).
FALLBACK_SECONDS = {"issue": 6.25, "own_carve": 7.75}


@pytest.fixture(scope="module")
def many_pieces():
    import matchering_amd as mg

    cache = {}

    def run(which):
        if which not in cache:
            case = dict(CASES["hot_lowrate"], seconds=FALLBACK_SECONDS[which], reference_seconds=4.9)
            kw = dict(internal_sample_rate=8000, fft_size=8, max_piece_size=0.00125)
            t, r = build_inputs(case)
            tr = {}
            want = mo.master(t, r, mo.params(**kw), True, True, True, trace=tr)
            cache[which] = (t, r, want, tr, mg.Config(**kw))
        return cache[which]

    return run


@pytest.mark.parametrize("which", sorted(FALLBACK_SECONDS))
def test_profile_route_with_thousands_of_pieces(which, many_pieces):
    from matchering_amd import ReferenceProfile

    t, r, want, tr, cfg = many_pieces(which)
    assert tr["target_divisions"] == {"issue": 5001, "own_carve": 6201}[which] and tr["reference_divisions"] == 3921
    profile = ReferenceProfile.analyze(r, cfg)
    assert profile.loud_count == len(tr["reference_loud_idx"])
    rep, got, _ = master_on_device(t, cfg, profile=profile)
    assert rep.target_loud_count == len(tr["target_loud_idx"])
    assert rep.reference_loud_count == len(tr["reference_loud_idx"])
    errs = [rms_error(a, b) for a, b in zip(got, want)]
    print(which, "rms errors vs oracle", errs)
    assert max(errs) <= RMS_TOL


@pytest.mark.parametrize("which", sorted(FALLBACK_SECONDS))
def test_pair_route_with_thousands_of_pieces_as_a_control(which, many_pieces):
    """The pair route on the same inputs (k_levels + k_average_spectra + k_fir_raw for both: 235 KB / 259 KB of tables)."""
    t, r, want, tr, cfg = many_pieces(which)
    rep, got, _ = master_on_device(t, cfg, reference=r)
    assert (rep.target_loud_count, rep.reference_loud_count) == (len(tr["target_loud_idx"]), len(tr["reference_loud_idx"]))
    assert max(rms_error(a, b) for a, b in zip(got, want)) <= RMS_TOL


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field, other", [("fft_size", dict(fft_size=2048)), ("threshold", dict(threshold=0.9)),
                                          ("max_piece_size", dict(max_piece_size=0.3))])
def test_a_profile_made_with_another_config_is_refused(field, other, runs):
    import matchering_amd as mg
    from matchering_amd import stages
    from matchering_amd._native import ERR_ARGUMENT, MgxError

    t, r, outs, _, cfg, profile = runs("cd_default")
    wrong = mg.Config(**dict(CASES["cd_default"]["config"], **other))
    # the Python route: before anything is launched
    with pytest.raises(ValueError, match=field):
        stages.main(t, profile, wrong)
    # the C route: the device notices, the next blocking call says which field
    with pytest.raises(MgxError, match=field) as caught:
        master_on_device(t, wrong, profile=profile)
    assert caught.value.code == ERR_ARGUMENT
    # ... and the handle masters a correct pair afterwards
    _, res, _ = master_on_device(t, cfg, reference=r)
    assert rms_error(res[0], outs[0]) <= RMS_TOL


def test_a_corrupted_magic_is_refused(runs):
    from matchering_amd import ReferenceProfile
    from matchering_amd._native import ERR_ARGUMENT, MgxError
    from matchering_amd.device import default_device

    t, r, outs, _, cfg, profile = runs("cd_default")
    blob = bytearray(profile.tobytes())
    blob[0] ^= 0x40
    with pytest.raises(ValueError, match="magic"):
        ReferenceProfile(bytes(blob))

    class Forged:                                   # (what a C host could hand over: the bytes as they are)
        buf = None

        def resident(self, dev):
            self.buf = dev.upload(np.frombuffer(bytes(blob), dtype=np.uint8), dtype=None)
            return self.buf

    forged = Forged()
    try:
        with pytest.raises(MgxError, match="magic") as caught:
            master_on_device(t, cfg, profile=forged)
    finally:
        with default_device().lock:
            forged.buf.release()
    assert caught.value.code == ERR_ARGUMENT
    _, res, _ = master_on_device(t, cfg, profile=profile)
    assert rms_error(res[0], outs[0]) <= RMS_TOL


@pytest.mark.parametrize("value", [np.nan, -np.inf])
def test_a_reference_with_samples_that_are_not_numbers_makes_no_profile(value, runs):
    from matchering_amd import ReferenceProfile, stages
    from matchering_amd._native import ERR_ARGUMENT, MgxError

    t, r, outs, _, cfg, profile = runs("cd_default")
    bad = r.copy()
    bad[30000, 1] = value
    with pytest.raises(MgxError, match="not finite") as caught:
        ReferenceProfile.analyze(bad, cfg)
    assert caught.value.code == ERR_ARGUMENT
    got = stages.main(t, profile, cfg)              # the handle is good for the next call
    assert rms_error(got[0], outs[0]) <= RMS_TOL


def test_a_target_with_a_nan_fails_on_the_profile_route_too(runs):
    from matchering_amd import stages
    from matchering_amd._native import ERR_ARGUMENT, MgxError

    t, r, outs, _, cfg, profile = runs("cd_default")
    bad = t.copy()
    bad[50000, 0] = np.nan
    with pytest.raises(MgxError, match="not finite") as caught:
        stages.main(bad, profile, cfg)
    assert caught.value.code == ERR_ARGUMENT
    assert rms_error(stages.main(t, profile, cfg)[0], outs[0]) <= RMS_TOL


# ---- 7. one launch per correction round (what a handle falls back to, and what its requeue replays) ------------------------
def test_profile_route_one_launch_per_round_equals_the_tail_kernel():
    """MGX_NO_TAIL=1 in a fresh child process against the default mode, both on the profile route: the same
    coefficients.  "Identical" was what was asked for; the assertion is 1e-12 relative, the bound
    tests/test_device_errors.py holds the pair route's two modes to, because the tail kernel and the one-launch rounds
    add a round's partial sums in different orders, on either route.  The requeue itself is not provoked here:
    that MasterCall carries the profile through it is read in queue_master, not run."""
    child = r'''
import sys
sys.path.insert(0, {root!r})
import numpy as np
import matchering_amd as mg
from matchering_amd import ReferenceProfile
from matchering_amd.device import Device
from matchering_amd.synth import make_pair
target, reference = make_pair(6.0, 44100, pair=5)
dev = Device(0)
cfg = mg.Config(rms_correction_steps=6, max_piece_size=1.0)
profile = ReferenceProfile.analyze(reference, cfg, device=dev)
t = dev.upload(target)
out = dev.alloc(target.shape[0] * 8)
rep = dev.master(t, target.shape[0], None, 0, cfg.to_native(), result=out, profile=profile.resident(dev))
print("C", " ".join(repr(c) for c in rep.correction_coefficients[:6]), float(np.abs(dev.download(out, target.shape)).sum()))
'''.format(root=ROOT)
    outs = []
    for flag in ("0", "1"):
        done = subprocess.run([sys.executable, "-c", child], env=dict(os.environ, MGX_NO_TAIL=flag), capture_output=True,
                              text=True, timeout=300)
        assert done.returncode == 0, done.stderr[-2000:]
        outs.append([float(v) for v in done.stdout.split("C", 1)[1].split()])
    a, b = outs
    assert len(a) == 7 and all(abs(x / y - 1.0) <= 1e-12 for x, y in zip(a[:6], b[:6])), (a, b)
    assert abs(a[6] / b[6] - 1.0) <= 1e-6


# ---- 8. album mode ---------------------------------------------------------------------------------------------------------
def test_album_mode_with_a_profile_equals_track_by_track(runs):
    from matchering_amd import batch, stages
    from matchering_amd.synth import make_pair

    _, r, _, _, cfg, profile = runs("cd_default")
    targets = [make_pair(1.5 + 0.4 * i, 44100, pair=20 + i)[0] for i in range(3)]
    album = batch.master_album(targets, profile, cfg, rank=0, world_size=1, device_index=0, need_no_limiter=True)
    dev = batch.lane_device(0, 0)
    fir_ptr, taps = None, None
    first = stages.main(targets[0], profile, cfg, True, True, device=dev)
    with dev.lock:
        fir_ptr, taps = dev.last_fir()
        fir = dev.upload(np.array(dev.download(fir_ptr, (2 * taps,))))
    try:
        for i, t in enumerate(targets):
            alone = first if i == 0 else stages.main(t, profile, cfg, True, True, device=dev, fir=fir)
            for a, b in zip(album[i][:2], alone[:2]):
                assert np.array_equal(a, b), i
    finally:
        fir.release()


def test_master_many_with_a_profile_equals_call_by_call(runs):
    from matchering_amd import batch, stages
    from matchering_amd.synth import make_pair

    _, _, _, _, cfg, profile = runs("cd_default")
    targets = [make_pair(1.5 + 0.3 * i, 44100, pair=30 + i)[0] for i in range(3)]
    many = batch.master_many([(t, profile) for t in targets], cfg, need_no_limiter=True, lanes=2)
    for t, got in zip(targets, many):
        alone = stages.main(t, profile, cfg, True, True)
        assert np.array_equal(got[0], alone[0]) and np.array_equal(got[1], alone[1]) and got[2] is None


def test_process_batch_shares_a_reference_file(tmp_path, monkeypatch):
    """Three jobs naming one reference file, on two real lanes.  share_references=True: the reference is analysed once
    per lane device that masters one of them (counted through a wrapper, nothing is timed) and the files are those of
    job-by-job ``process(target, profile)``; the default writes the files of job-by-job ``process(target, reference)``,
    as it did before there were profiles, and analyses nothing."""
    import matchering_amd as mg
    from matchering_amd import ReferenceProfile, audio_io, batch
    from matchering_amd.synth import make_pair

    sr = 44100
    cfg = mg.Config(max_piece_size=1.0)
    rp = str(tmp_path / "reference.wav")
    audio_io.write_wav(rp, make_pair(3.0, sr, pair=40, reference_seconds=2.6)[1], sr, "PCM_16")
    profile = ReferenceProfile.analyze(rp, cfg)
    jobs, want_profile, want_pair = [], [], []
    for i in range(3):
        tp = str(tmp_path / f"target{i}.wav")
        audio_io.write_wav(tp, make_pair(2.0 + 0.4 * i, sr, pair=41 + i)[0], sr, "PCM_24")
        for route, reference, wanted in (("profile", profile, want_profile), ("pair", rp, want_pair)):
            out = str(tmp_path / f"{route}{i}.wav")
            mg.process(tp, reference, [mg.pcm16(out)], config=cfg)
            wanted.append(open(out, "rb").read())
        jobs.append({"target": tp, "reference": rp, "results": [mg.pcm16(str(tmp_path / f"batch{i}.wav"))]})
    analysed = []
    real = batch._analyze_reference

    def counting(path, config, device):
        analysed.append(device)
        return real(path, config, device)

    monkeypatch.setattr(batch, "_analyze_reference", counting)
    written = lambda: [open(job["results"][0].file, "rb").read() for job in jobs]          # noqa: E731
    assert batch.process_batch(jobs, cfg, rank=0, world_size=1, device_index=0, lanes=2, share_references=True) == [0, 1, 2]
    assert written() == want_profile
    lanes = {batch.lane_device(0, lane) for lane in range(2)}
    assert 1 <= len(analysed) <= 2 and len(set(analysed)) == len(analysed) and set(analysed) <= lanes
    analysed.clear()
    assert batch.process_batch(jobs, cfg, rank=0, world_size=1, device_index=0, lanes=2) == [0, 1, 2]
    assert written() == want_pair and analysed == []


# ---- 9. files end to end ---------------------------------------------------------------------------------------------------
def test_process_with_a_saved_profile(tmp_path):
    import matchering_amd as mg
    from matchering_amd import ReferenceProfile, audio_io
    from matchering_amd.synth import make_pair

    sr = 44100
    t, r = make_pair(3.0, sr, pair=9, reference_seconds=2.3)
    tp, rp, pp = str(tmp_path / "target.wav"), str(tmp_path / "reference.wav"), str(tmp_path / "reference.profile")
    audio_io.write_wav(tp, t, sr, "PCM_24")
    audio_io.write_wav(rp, r, sr, "PCM_16")
    cfg = mg.Config(max_piece_size=1.0)
    profile = ReferenceProfile.analyze(rp, cfg)
    profile.save(pp)
    assert ReferenceProfile.load(pp) == profile
    outs = {k: str(tmp_path / f"{k}.wav") for k in ("pair", "saved", "object")}
    codes = []
    mg.log(lambda m: codes.append(m.split(":")[0]), show_codes=True)
    try:
        mg.process(tp, pp, [mg.pcm16(outs["saved"])], config=cfg)
    finally:
        mg.log()
    assert [c for c in codes if c.startswith("20")] == ["2003", "2004", "2005", "2006", "2007", "2008", "2010"]
    mg.process(tp, profile, [mg.pcm16(outs["object"])], config=cfg)
    mg.process(tp, rp, [mg.pcm16(outs["pair"])], config=cfg)
    saved, obj, pair = (audio_io.read_wav(outs[k])[0] for k in ("saved", "object", "pair"))
    assert np.array_equal(saved, obj)
    assert rms_error(saved, pair) <= RMS_TOL


def test_profile_of_an_off_rate_mono_reference_file(tmp_path):
    """A 22 050 Hz mono reference through ``ReferenceProfile.analyze(path)``: decoded, converted to 44 100 Hz and given
    its second column on the GPU by the route ``process`` takes with such a reference (same log codes, the frame count
    of the conversion), so the two routes see the same frames: the profile route's file against the pair route's, at
    the 1e-5 RMS tests/test_gpu_resample.py holds converted tracks to.  (That the conversion itself is right is
    tests/test_gpu_resample.py's subject, not this test's.)"""
    import matchering_amd as mg
    from matchering_amd import ReferenceProfile, audio_io
    from matchering_amd.synth import make_pair

    sr = 44100
    t, _ = make_pair(3.0, sr, pair=12)
    _, r_low = make_pair(3.0, 22050, pair=13, reference_seconds=2.4)
    tp, rp = str(tmp_path / "target.wav"), str(tmp_path / "reference.wav")
    audio_io.write_wav(tp, t, sr, "PCM_16")
    audio_io.write_wav(rp, r_low[:, :1], 22050, "PCM_16")
    cfg = mg.Config(max_piece_size=1.0)
    codes = []
    mg.log(lambda m: codes.append(m.split(":")[0]), show_codes=True)
    try:
        profile = ReferenceProfile.analyze(rp, cfg)
    finally:
        mg.log()
    assert "2201" in codes and "2202" in codes          # mono, and off-rate: the codes process() logs for such a reference
    assert profile.frames == int(r_low.shape[0] * (44100 / 22050))
    out_q, out_p = str(tmp_path / "profile.wav"), str(tmp_path / "pair.wav")
    mg.process(tp, profile, [mg.Result(out_q, "FLOAT")], config=cfg)
    mg.process(tp, rp, [mg.Result(out_p, "FLOAT")], config=cfg)
    assert rms_error(audio_io.read_wav(out_q)[0], audio_io.read_wav(out_p)[0]) <= RMS_TOL
