"""Pipelined master calls with different matching EQ tones: the tone is a field of the call next to the
shape, copied when the call is queued, so the front half of call k + 1 -- which designs its FIR under the back half of
call k -- tones it with its own.  A handle pipelines only while it is its device's only live handle, and a pytest process
keeps others alive, so the scenario runs in a child process of its own: this file, run as a script.
"""

import os
import subprocess
import sys

import numpy as np
import pytest


def child():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import matchering_amd as mg
    from matchering_amd.device import Device
    from matchering_amd.synth import make_pair

    target, reference = make_pair(3.0, 44100, pair=72, reference_seconds=2.6)
    n, nr = target.shape[0], reference.shape[0]
    cfg = mg.Config(max_piece_size=0.8).to_native()
    eqs = [mg.MatchingEq(amount=0.5, match_range=(60.0, 12000.0), side_amount=0.0),
           mg.MatchingEq(phase="minimum", mono_below_hz=120.0, tilt_db_per_octave=-0.5),
           mg.MatchingEq(amount=0.5),                                                   # a neutral tone: k_eq_shape's route
           mg.MatchingEq(bands=(mg.ToneBand("high_shelf", 10000.0, 1.5), mg.ToneBand("bell", 250.0, -3.0, channels="side")))]
    dev = Device(0)
    td, rd = dev.upload(target), dev.upload(reference)
    # each tone alone, waited for: what every queued call below has to give
    alone = []
    for eq in eqs:
        out = dev.alloc(n * 8)
        dev.master(td, n, rd, nr, cfg, result=out, want_report=False, eq=eq)
        dev.synchronize()
        alone.append(dev.download(out, (n, 2)))
    assert all(not np.array_equal(alone[i], alone[j]) for i in range(4) for j in range(i))
    # eight calls queued without a wait; the tone objects' native structs die right after each call returns
    outs, firs = [dev.alloc(n * 8) for _ in range(8)], []
    for k, out in enumerate(outs):
        dev.master(td, n, rd, nr, cfg, result=out, want_report=False, eq=eqs[k % 4])
        firs.append(dev.last_fir()[0])
    dev.synchronize()
    # (consecutive pipelined calls design their FIRs into the handle's two contexts in turn)
    assert firs[0] != firs[1] and firs[0] == firs[2], "the handle did not pipeline: the comparison would show nothing"
    for k, out in enumerate(outs):
        assert np.array_equal(dev.download(out, (n, 2)), alone[k % 4]), f"call {k} did not get its own tone"
    dev.close()
    print("ok")


@pytest.mark.gpu
def test_pipelined_calls_keep_their_own_tones():
    done = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and done.stdout.strip().endswith("ok"), done.stdout + done.stderr


if __name__ == "__main__":
    child()
