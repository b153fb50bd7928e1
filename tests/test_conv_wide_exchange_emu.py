"""The wide-block convolution's newer phase forms against the ones they replaced, on the CPU and bit for bit
(tests/emu/emu_conv_wide_forms.cpp over conv_wide_kernel.h): the block peak as one maximum per wave that thread 0 combines, and the end-of-track
mask behind a last-block branch.  Neither changes the arithmetic or its order, so every output must be the same bits --
on the 2048- to 16384-point plans, whose pass-0 butterflies per thread, strides and row lengths all differ.  (The form
this file is named after, 16-byte global accesses with an exchange between lanes 2p and 2p + 1, was emulated here as a
permutation between paired threads and passed, and so did filter tables that hold P and Q; both lost their A/B on the
GPU and left the kernel)  A target that starts one frame into its buffer must give the same
bits too.
"""

import ctypes

import numpy as np
import pytest

import emu_build

c_float_p = ctypes.POINTER(ctypes.c_float)
c_double_p = ctypes.POINTER(ctypes.c_double)
KEEP, PEAK, END = 1, 2, 4                                      # emu_conv_wide_forms.cpp, WIDE_*
ALL = KEEP | PEAK | END

# the emulation unit with a choice of forms (tests/emu/emu_conv_wide_forms.cpp), registered with tests/emu/build.py at
# run time under the flags of the "kernels" unit
NAME = "conv_wide_forms"
if NAME not in emu_build.UNITS:
    _kernels = emu_build.UNITS["kernels"]
    emu_build.UNITS[NAME] = type(_kernels)(("emu_conv_wide_forms.cpp",), _kernels.headers, _kernels.flags, None)


@pytest.fixture(scope="module")
def emu():
    return emu_build.load(NAME)


def _run(emu, x, hm, hs, forms, offset=0):
    """x: (n + offset, 2) float32; the track starts `offset` frames into it (8 bytes a frame: an odd offset is a pointer
    that is 8- but not 16-byte aligned)."""
    n = x.shape[0] - offset
    taps = len(hm)
    y = np.zeros((n, 2), dtype=np.float32)
    ymid = np.zeros(n, dtype=np.float32)
    peaks = np.zeros((n + 3 * taps - 1) // (3 * taps), dtype=np.float32)
    rc = emu.emu_convolve_wide_forms(x[offset:].ctypes.data_as(c_float_p), ctypes.c_longlong(n),
                                     hm.ctypes.data_as(c_double_p), hs.ctypes.data_as(c_double_p), ctypes.c_int(taps),
                                     ctypes.c_double(1.3), y.ctypes.data_as(c_float_p), ymid.ctypes.data_as(c_float_p),
                                     peaks.ctypes.data_as(c_float_p), ctypes.c_int(forms))
    assert rc == 0
    return y, ymid, peaks


def _inputs(taps, n, offset=0):
    rng = np.random.RandomState(taps + n)
    x = np.ascontiguousarray((0.3 * rng.randn(n + offset, 2)).astype(np.float32))
    assert x.ctypes.data % 16 == 0
    return x, rng.randn(taps) / np.sqrt(taps), rng.randn(taps) / np.sqrt(taps)


# hop = 3 taps.  Per plan: a track shorter than a block, one that ends a frame into a block (a last block of one frame),
# one that ends a frame short of a block's end, and several blocks of which the middle ones lie inside the track
@pytest.mark.parametrize("taps,n", [(512, 1), (512, 3), (512, 1535), (512, 1537), (512, 5 * 1536 + 1),
                                    (1024, 3 * 3072 - 1), (1024, 4 * 3072 + 2), (2048, 3 * 6144 + 1),
                                    (4096, 12289), (4096, 3 * 12288 - 1), (4096, 4 * 12288 + 4321)])
def test_new_phase_forms_equal_the_old_ones_bit_for_bit(emu, taps, n):
    x, hm, hs = _inputs(taps, n)
    want = _run(emu, x, hm, hs, KEEP)
    assert np.abs(want[0]).max() > 0 and want[2].min() > 0
    for forms in (ALL, KEEP | PEAK, KEEP | END, PEAK | END, 0):
        got = _run(emu, x, hm, hs, forms)
        for g, w, what in zip(got, want, ("y", "mid plane", "block peaks")):
            assert np.array_equal(g, w), (forms, what)


@pytest.mark.parametrize("taps,n", [(512, 5 * 1536 + 1), (4096, 3 * 12288 - 1)])
def test_a_target_one_frame_into_its_buffer_gives_the_same_bits(emu, taps, n):
    x, hm, hs = _inputs(taps, n, offset=1)
    want = _run(emu, np.ascontiguousarray(x[1:]), hm, hs, KEEP)
    got = _run(emu, x, hm, hs, ALL, offset=1)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_the_last_block_branch_is_what_masks_the_peak(emu):
    """The frames a last block computes past the end of the track are not zero (the filter's tail over the last real
    frames): a block peak that ignored the end of the track would exceed the maximum over the frames that exist.  Guards
    the comparisons above against a track whose tail happens not to matter."""
    taps, n = 512, 1537                                        # the last block holds one frame
    x, hm, hs = _inputs(taps, n)
    x[:-1] *= 1e-3                                             # everything the last block computes comes from the last frames
    y, _, peaks = _run(emu, x, hm, hs, ALL)
    assert peaks[1] == np.abs(y[1536:]).max()
    full = _run(emu, np.concatenate([x, np.zeros((1536, 2), np.float32)]), hm, hs, ALL)
    assert np.abs(full[0][1537:]).max() > peaks[1]             # what lies past the end is larger than the frame that exists
