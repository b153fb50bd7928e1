"""The clip repair's phase functions (csrc/declip_kernel.h), run segment by segment on the host (tests/declip_emu.py),
against the definition (tests/declip_oracle.py): output bits and every counter equal, at the kernel's geometry on the
border cases and at a scaled-down one on random tracks, where a border comes every 64 frames.  No GPU."""
import subprocess

import numpy as np
import pytest

import declip_emu
import declip_oracle as oracle
import emu_build

SMALL = dict(segment=64, halo=20, stretch=6)         # max_run up to 18


def same(x, level, geometry=None, **params):
    want, want_report = oracle.declip(x, level, **params)
    got, got_report = declip_emu.declip(x, level, **params, **(geometry or {}))
    assert got.tobytes() == want.tobytes()
    assert got_report == want_report
    return want_report


def test_constants_are_the_issues():
    k = declip_emu.constants()
    assert k["segment"] == 4096 and k["max_run"] == 512 and k["halo"] == 514 and k["window"] == 5124
    assert k["window"] * 8 == 40992 and k["threads"] * k["stretch"] >= k["window"] and k["stretch"] % 2 == 0


@pytest.mark.parametrize("max_run", [32, 512])
def test_border_cases_at_the_kernels_geometry(max_run):
    seen = {}
    for name, (n, runs) in oracle.border_cases(4096, max_run).items():
        seen[name] = same(oracle.track_with(n, runs), 0.8, max_run=max_run)
    assert seen["max_run_across"]["runs_repaired"] == (2, 2) and seen["max_run_across"]["longest_repaired"] == (max_run, max_run)
    assert seen["max_run_plus_one_across"]["runs_long"] == (1, 1)
    assert seen["min_run_less_one"]["runs_short"] == (2, 2) and seen["min_run"]["runs_repaired"] == (2, 2)
    assert seen["track_ends"]["runs_edge"] == (2, 2) and seen["track_ends"]["runs_repaired"] == (0, 0)
    assert seen["second_frame_and_last_but_one"]["runs_repaired"] == (2, 2)
    assert seen["starts_at_border"]["first_repaired"] == (4096, 4093)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 517, 4 * 4096 + 1])
def test_lengths_at_the_kernels_geometry(n):
    same(oracle.random_track(n, 100 + n % 97, nonfinite=2 if n > 8 else 0), 0.8)


@pytest.mark.parametrize("max_run", [6, 18])
def test_border_cases_at_a_small_geometry(max_run):
    for name, (n, runs) in oracle.border_cases(64, max_run).items():
        same(oracle.track_with(n, runs), 0.8, SMALL, max_run=max_run)


def test_random_tracks_at_a_small_geometry():
    rng = np.random.default_rng(11)
    raised = 0
    for seed in range(120):
        n = int(rng.integers(0, 700))
        x = oracle.random_track(n, seed, longest=22, density=0.08, nonfinite=seed % 3)
        report = same(x, 0.8, SMALL, min_run=1 + seed % 3, max_run=int(rng.integers(3, 19)), max_rise=1.0 + (seed % 4) * 0.5)
        raised += sum(report["samples_raised"])
    assert raised > 100                            # (the tracks do exercise the evaluation)


def test_nonfinite_anchors_and_samples_inside_a_run():
    n = 64 * 3 + 5
    for bad in (np.nan, np.inf, -np.inf):
        for at in (58, 59, 66, 67, 62):             # the four anchors of the run [60, 66), and a sample inside it
            x = oracle.track_with(n, [(0, 60, 6, 1), (1, 60, 6, -1)])
            x[at, :] = bad
            report = same(x, 0.8, SMALL, max_run=18)
            # (inside, it ends the run and is an anchor of both halves)
            assert report["runs_edge"] == ((2, 2) if at == 62 else (1, 1)) and report["runs_repaired"] == (0, 0)


def test_clean_all_at_rail_and_a_binding_cap():
    x = oracle.quiet(4 * 64 + 3, 3)
    report = same(x, 0.8, SMALL, max_run=18)
    assert sum(report["runs_repaired"] + report["runs_short"] + report["runs_long"] + report["runs_edge"]) == 0
    rail = np.full((4 * 64 + 3, 2), 0.8, dtype=np.float32)
    rail[:, 1] = -0.8
    assert same(rail, 0.8, SMALL, max_run=18)["runs_long"] == (1, 1)
    assert same(np.full((3 * 4096 + 9, 2), 1.0, dtype=np.float32), 1.0, max_run=512)["runs_long"] == (1, 1)
    # steep anchors: the segment overshoots and max_rise 1.05 holds it
    x = oracle.quiet(200, 5, 0.01)
    x[98:110, 0] = [-0.5, 0.75, 0.8, 0.8, 0.8, 0.8, 0.8, 0.8, 0.8, 0.8, 0.75, -0.5]
    x[98:110, 1] = -x[98:110, 0]
    capped, loose = same(x, 0.8, SMALL, max_run=18, max_rise=1.05), same(x, 0.8, SMALL, max_run=18, max_rise=4.0)
    assert capped["peak_after"] == (float(np.float32(1.05 * 0.8)),) * 2 and loose["peak_after"][0] > capped["peak_after"][0]


def test_standalone_emulation_under_sanitizers(tmp_path):
    """Built with AddressSanitizer and UBSan, run once (nothing loaded into Python runs under a sanitizer): ``ok`` and
    exit status 0."""
    out = str(tmp_path / "emu_declip_driver")
    emu_build.build_driver(declip_emu.NAME, out, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    done = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip() == "ok", done.stdout + done.stderr
