"""k_conv_wide at the edges of its blocks and of the memory it is given (conv_wide_kernel.h; written for a 16-byte
access path that blocks inside the track would have taken on 16-byte aligned memory -- it lost its A/B, DESIGN.md
section 3.4, and the cases stay: the block peak that is written a barrier late and the last-block branch of the
end-of-track mask meet the same edges).  4096 taps, the default fft_size: blocks of 12288 frames whose
windows start 2048 frames early.  Track lengths: one to three frames; around the first window's negative start; around
one block; a last block of one frame behind two whole ones; three blocks less a frame, whose middle block is the only
one inside the track.  Each length again with the target one frame into its buffer -- a pointer that is 8- but not
16-byte aligned -- which must give the same bits.

mgx_master refuses tracks of fft_size frames or fewer (core.py:69-74): the lengths below 4097 are the convolution's alone.
"""

import ctypes
import types

import numpy as np
import pytest

import mastering_oracle as mo
from conftest import rms_error

pytestmark = pytest.mark.gpu

TAPS = 4096
HOP = 3 * TAPS
LENGTHS = [1, 2, 3, 2047, 2048, 2049, HOP - 1, HOP, HOP + 1, 2 * HOP + 1, 3 * HOP - 1]
MASTER_LENGTHS = [n for n in LENGTHS if n > TAPS]
RMS_TOL = 1e-5                                                 # test_gpu_parity.py, the master against the oracle


def _convolve(x_padded, offset, hm, hs, gain):
    """mgx_convolve on frames [offset, ...) of an uploaded buffer: (y, mid plane, peak)."""
    from matchering_amd._native import c_double_p, check, library
    from matchering_amd.device import default_device

    dev = default_device()
    n = x_padded.shape[0] - offset
    with dev.lock:
        xb, yb, mb = dev.upload(x_padded), dev.alloc(n * 8), dev.alloc(n * 4)
        peak = ctypes.c_double()
        try:
            check(library().mgx_convolve(dev.handle, ctypes.c_void_p(xb.ptr + 8 * offset), n, hm.ctypes.data_as(c_double_p),
                                         hs.ctypes.data_as(c_double_p), TAPS, float(gain), ctypes.c_void_p(yb.ptr),
                                         ctypes.c_void_p(mb.ptr), ctypes.byref(peak)))
            return np.array(dev.download(yb, (n, 2))), np.array(dev.download(mb, (n,))), peak.value
        finally:
            for b in (xb, yb, mb):
                b.release()


def _filters(seed):
    rng = np.random.RandomState(seed)
    return rng.randn(TAPS) / np.sqrt(TAPS), rng.randn(TAPS) / np.sqrt(TAPS)


@pytest.mark.parametrize("n", LENGTHS)
def test_convolution_aligned_and_one_frame_off(n):
    """The bounds of test_default_filter_on_wide_blocks, against the oracle's convolution and scipy's fftconvolve."""
    from scipy import signal

    rng = np.random.RandomState(n % 100000)
    padded = np.ascontiguousarray((0.3 * rng.randn(n + 1, 2)).astype(np.float32))
    x = np.ascontiguousarray(padded[1:])
    hm, hs = _filters(n)
    y, ymid, peak = _convolve(x, 0, hm, hs, 1.1)
    mid, side = mo.mid_side(x.astype(np.float64))
    want, want_mid = mo.convolve_same(mid * 1.1, hm, side * 1.1, hs)
    assert rms_error(y, want) <= 1e-6
    assert rms_error(ymid, want_mid) <= 1e-6
    assert abs(peak - np.abs(y).max()) <= 1e-6
    sm, ss = signal.fftconvolve(mid * 1.1, hm, "same"), signal.fftconvolve(side * 1.1, hs, "same")
    assert rms_error(y, np.stack([sm + ss, sm - ss], axis=1)) <= 1e-6
    assert rms_error(ymid, sm) <= 1e-6
    y2, ymid2, peak2 = _convolve(padded, 1, hm, hs, 1.1)
    assert np.array_equal(y, y2) and np.array_equal(ymid, ymid2) and peak == peak2
    if n == 3 * HOP - 1:
        assert np.abs(ymid - 0.5 * (y[:, 0] + y[:, 1])).max() <= 1e-6      # dsp.py:57-68 round trip (test_gpu_full_size.py)


@pytest.mark.parametrize("n", [HOP + 1, 2 * HOP + 1, 3 * HOP - 1])
def test_every_blocks_peak_is_the_maximum_over_that_block(n):
    """The library consumes the block peaks through their maximum alone, so each block takes its turn at holding it: an
    impulse on the block's last frame under a filter whose centre tap dominates, over noise a thousand times quieter.
    The returned peak must then BE max |y| over that block -- the kernel's maximum is over the very float32 values it
    stores, so equality is exact.  The impulses shrink from run to run: a block's entry left over from the run before
    (a peak that was never written, or written to another block's slot) would be too large for its block or too small
    for the new one."""
    rng = np.random.RandomState(n)
    hm, hs = 0.05 * rng.randn(TAPS) / np.sqrt(TAPS), 0.05 * rng.randn(TAPS) / np.sqrt(TAPS)
    hm[TAPS // 2 - 1], hs[TAPS // 2 - 1] = 1.0, 0.6          # fftconvolve "same": this tap maps frame f to frame f
    blocks = (n + HOP - 1) // HOP
    for b in range(blocks):
        x = (1e-3 * rng.randn(n, 2)).astype(np.float32)
        f = min((b + 1) * HOP, n) - 1
        x[f] = (0.9 - 0.1 * b, 0.3)
        y, _, peak = _convolve(np.ascontiguousarray(x), 0, hm, hs, 1.0)
        mags = np.abs(y).max(axis=1)
        assert mags.argmax() == f
        assert peak == float(mags[b * HOP:(b + 1) * HOP].max()) == float(mags.max())


@pytest.fixture(scope="module")
def master_pair():
    from matchering_amd.synth import make_pair

    return make_pair(1.0, 44100, pair=5, reference_seconds=0.9)


def _master(target_padded, offset, reference):
    import matchering_amd as mg
    from matchering_amd.device import default_device

    dev = default_device()
    n = target_padded.shape[0] - offset
    with dev.lock:
        td, rd = dev.upload(target_padded), dev.upload(reference)
        outs = [dev.alloc(n * 8) for _ in range(3)]
        try:
            dev.master(types.SimpleNamespace(ptr=td.ptr + 8 * offset), n, rd, reference.shape[0], mg.Config().to_native(), *outs)
            return [np.array(dev.download(o, (n, 2))) for o in outs]
        finally:
            for b in (td, rd, *outs):
                b.release()


@pytest.mark.parametrize("n", MASTER_LENGTHS)
def test_master_aligned_and_one_frame_off(n, master_pair):
    """mgx_master at the default fft_size (its convolution reads the target where the caller put it) against the oracle,
    at the bounds of test_gpu_parity.py's master tests."""
    target, reference = master_pair
    padded = np.ascontiguousarray(target[:n + 1])
    t = np.ascontiguousarray(padded[1:])
    got = _master(t, 0, reference)
    want = mo.master(t, reference, mo.params(), True, True, True)
    for mine, ref in zip(got, want):
        assert rms_error(mine, ref) <= RMS_TOL
        assert np.abs(mine - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max())
    again = _master(padded, 1, reference)
    for a, b in zip(got, again):
        assert np.array_equal(a, b)
