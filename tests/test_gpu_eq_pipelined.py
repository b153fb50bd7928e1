"""Pipelined master calls with different matching EQ shapes: the shape is a field of the call, copied when
the call is queued, so the front half of call k + 1 -- which designs its FIR under the back half of call k -- shapes it
with its own.  A handle pipelines only while it is its device's only live handle, and a pytest process keeps others
alive, so the scenario runs in a child process of its own: this file, run as a script.
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

    target, reference = make_pair(3.0, 44100, pair=71, reference_seconds=2.6)
    n, nr = target.shape[0], reference.shape[0]
    cfg = mg.Config(max_piece_size=0.8).to_native()
    shapes = [mg.MatchingEq(amount=0.5, max_boost_db=6.0, max_cut_db=6.0), mg.MatchingEq(phase="minimum"), None]
    dev = Device(0)
    td, rd = dev.upload(target), dev.upload(reference)
    # each shape alone, waited for: what every queued call below has to give
    alone = []
    for eq in shapes:
        out = dev.alloc(n * 8)
        dev.master(td, n, rd, nr, cfg, result=out, want_report=False, eq=eq)
        dev.synchronize()
        alone.append(dev.download(out, (n, 2)))
    assert not np.array_equal(alone[0], alone[1]) and not np.array_equal(alone[0], alone[2])
    # six calls queued without a wait; the shape objects' native structs die right after each call returns
    outs, firs = [dev.alloc(n * 8) for _ in range(6)], []
    for k, out in enumerate(outs):
        dev.master(td, n, rd, nr, cfg, result=out, want_report=False, eq=shapes[k % 3])
        firs.append(dev.last_fir()[0])
    dev.synchronize()
    # (consecutive pipelined calls design their FIRs into the handle's two contexts in turn)
    assert firs[0] != firs[1] and firs[0] == firs[2], "the handle did not pipeline: the comparison would show nothing"
    for k, out in enumerate(outs):
        assert np.array_equal(dev.download(out, (n, 2)), alone[k % 3]), f"call {k} did not get its own shape"
    dev.close()
    print("ok")


@pytest.mark.gpu
def test_pipelined_calls_keep_their_own_shapes():
    done = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and done.stdout.strip().endswith("ok"), done.stdout + done.stderr


if __name__ == "__main__":
    child()
