"""Level correction with the running gain outside [BAND_G_LO, BAND_G_HI] = [0.7, 1.5] (csrc/correction_kernels.h), where a
round streams the mid plane again instead of reading round 0's band lists.

The hard material of tests/test_gpu_hard_inputs.py leaves the band downwards from round 1 on, by accident and on the tail
kernel's pair route alone.  The stimuli here (tests/boundary_cases.py, BAND_EXITS) are made for it, and every test first
asserts from the oracle's trace that the gain each round starts from is where the stimulus says -- inside the band for
the rounds meant to read the lists, outside it by 1 % at least for the rounds meant to stream -- so that a change of the
generators or of the constants cannot silently take the cover away:

  up_midway      an ordinary pair against a hard-clipped reference: 1.2656, 1.4337, 1.5521, 1.6387 -- rounds 1 and 2 on the
                 lists, round 3 streams: the band is left upwards, in the middle of the tail kernel
  up_midway_12   the same with twelve rounds, on to 1.88: nine rounds stream in one tail launch
  down_at_once   sixteen bins of every 256 against broadband noise: 0.5245, then 0.5241 -- every later round streams
  far_up         a click every 997 frames against the same noise: 4.77, 18.97, 31.5, 34.0, 35.0, 35.3

Routes: the tail kernel (the default) and one launch per round (MGX_NO_TAIL=1, also what a handle falls back to after a
tail error), each on the pair and on the profile route.  No loud-piece decision of these stimuli sits on a tie in the
oracle (the coefficients would miss their bound by far more than rounding; tests/test_gpu_hard_inputs.py shows how to
tell); should a change of the generators put one there, the stimulus's seed is what changes, not a bound.

Measured on an MI355X (largest over the stimuli and routes):

  renderings against the oracle, RMS (bound 1e-5): result 6.9e-7, no_limiter 2.5e-6 (up_midway_12), normalized 4.0e-7;
  correction coefficients, relative (bound 1e-6): 5.6e-7 (up_midway), 4.0e-7 (far_up), 1.6e-7 (down_at_once);
  rms_coefficient and normalize_coefficient (bound 1e-6): 6.9e-7 (up_midway_12's normalize_coefficient).
  The four routes of a stimulus give the same figures to the digits shown; launch per round against the tail kernel
  holds its 1e-12.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import boundary_cases as bc
import mastering_oracle as mo
from conftest import ROOT, rms_error

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-5                  # the project's bar, float32 renderings against the float64 oracle
COEFFICIENT_TOL = 1e-6          # test_fir_and_stage_scalars_match_reference_golden's, relative
RENDERINGS = ("result", "no_limiter", "no_limiter_normalized")


@pytest.fixture(scope="module")
def oracle():
    """name -> (target, reference, the oracle's three renderings, its trace), once per module."""
    cache = {}

    def get(name):
        if name not in cache:
            target, reference = bc.band_exit_pair(name)
            trace = {}
            outs = mo.master(target, reference, mo.params(**bc.band_exit_config(name)), True, True, True, trace=trace)
            cache[name] = (target, reference, outs, trace)
        return cache[name]

    return get


@pytest.fixture(scope="module")
def dev():
    """A handle of this module's own: whatever route earlier tests left the default device on, this one starts on the
    tail kernel."""
    from matchering_amd.device import Device

    assert os.environ.get("MGX_NO_TAIL", "0") in ("", "0")
    device = Device(0)
    yield device
    device.close()


def master(dev, name, route):
    """One mgx_master (or mgx_master_with_profile) call: (the three renderings, the report's scalars as a dict)."""
    import matchering_amd as mg

    target, reference = bc.band_exit_pair(name)
    cfg = mg.Config(**bc.band_exit_config(name))
    n = target.shape[0]
    profile = mg.ReferenceProfile.analyze(reference, cfg, device=dev) if route == "profile" else None
    with dev.lock:
        td = dev.upload(target)
        rd = dev.upload(reference) if profile is None else None
        outs = [dev.alloc(n * 8) for _ in range(3)]
        try:
            extra = {} if profile is None else {"profile": profile.resident(dev)}
            rep = dev.master(td, n, rd, 0 if rd is None else reference.shape[0], cfg.to_native(), *outs, **extra)
            got = [np.array(dev.download(b, (n, 2))) for b in outs]
        finally:
            for b in (td, rd, *outs):
                if b is not None:
                    b.release()
    steps = cfg.rms_correction_steps
    return got, dict(correction_coefficients=[float(c) for c in rep.correction_coefficients[:steps]],
                     rms_coefficient=float(rep.rms_coefficient), normalize_coefficient=float(rep.normalize_coefficient))


def check_against_oracle(name, route, got, scalars, oracle_run):
    _, _, want, trace = oracle_run
    errs = [rms_error(a, b) for a, b in zip(got, want)]
    coeffs = np.array(scalars["correction_coefficients"])
    rel = float(np.abs(coeffs / trace["correction_coefficients"] - 1.0).max())
    others = max(abs(scalars["rms_coefficient"] / trace["rms_coefficient"] - 1.0),
                 abs(scalars["normalize_coefficient"] / trace["normalize_coefficient"] - 1.0))
    print(f"BOUNDARY band_exit {name} {route} rms=" + "/".join(f"{e:.2e}" for e in errs)
          + f" coefficients={rel:.2e} rms_and_normalize_coefficient={others:.2e}")
    for rendering, mine, err in zip(RENDERINGS, got, errs):
        assert np.all(np.isfinite(mine)), (name, route, rendering)
        assert err <= RMS_TOL, (name, route, rendering, err)
    assert coeffs.shape == trace["correction_coefficients"].shape and rel <= COEFFICIENT_TOL, (name, route, rel)
    assert others <= COEFFICIENT_TOL, (name, route, others)


@pytest.mark.parametrize("route", ["pair", "profile"])
@pytest.mark.parametrize("name", sorted(bc.BAND_EXITS))
def test_tail_kernel_with_the_gain_outside_the_band(dev, oracle, name, route):
    """The three renderings against the oracle at 1e-5 RMS, the correction coefficients, rms_coefficient and
    normalize_coefficient at 1e-6 relative, on the tail kernel."""
    run = oracle(name)
    bc.check_band_routes(name, run[3]["correction_coefficients"])            # the stimulus does what it is meant to
    got, scalars = master(dev, name, route)
    check_against_oracle(name, route, got, scalars, run)
    # the gain the device arrived at takes the same routes
    bc.check_band_routes(name, scalars["correction_coefficients"])


CHILD = r"""
import json, sys
sys.path[:0] = [{root!r}, {root!r} + "/oracle", {root!r} + "/tests", {root!r} + "/tests/golden"]
import numpy as np
import boundary_cases as bc
import test_gpu_band_exits as here
from matchering_amd.device import Device

dev = Device(0)
report = {{}}
for name in sorted(bc.BAND_EXITS):
    for route in ("pair", "profile"):
        got, scalars = here.master(dev, name, route)
        np.save({folder!r} + "/" + name + "_" + route + ".npy", np.stack(got))
        report[name + " " + route] = scalars
print("REPORT " + json.dumps(report))
"""


def test_one_launch_per_round_with_the_gain_outside_the_band(dev, oracle, tmp_path):
    """MGX_NO_TAIL=1 on a fresh handle in a child process, every stimulus on both routes: against the oracle as above, and
    against the tail kernel at the bound test_profile_route_one_launch_per_round_equals_the_tail_kernel holds the two
    modes to -- coefficients 1e-12 relative (the two add a round's partial sums in different orders), the result's sum of
    magnitudes 1e-6."""
    child = CHILD.format(root=ROOT, folder=str(tmp_path))
    done = subprocess.run([sys.executable, "-c", child], env=dict(os.environ, MGX_NO_TAIL="1"), capture_output=True,
                          text=True, timeout=300)
    assert done.returncode == 0 and "REPORT " in done.stdout, done.stderr[-2000:]
    report = json.loads(done.stdout.split("REPORT ", 1)[1])
    for name in sorted(bc.BAND_EXITS):
        run = oracle(name)
        bc.check_band_routes(name, run[3]["correction_coefficients"])
        for route in ("pair", "profile"):
            scalars = report[f"{name} {route}"]
            got = list(np.load(os.path.join(str(tmp_path), f"{name}_{route}.npy")))
            check_against_oracle(name, route + "/launch-per-round", got, scalars, run)
            tail_got, tail_scalars = master(dev, name, route)
            a, b = np.array(scalars["correction_coefficients"]), np.array(tail_scalars["correction_coefficients"])
            assert np.abs(a / b - 1.0).max() <= 1e-12, (name, route, a, b)
            assert abs(float(np.abs(got[0]).sum()) / float(np.abs(tail_got[0]).sum()) - 1.0) <= 1e-6, (name, route)
