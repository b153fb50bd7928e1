"""The device sample-rate converter without a GPU: the host plan of csrc/resample_plan.cpp against the rows read off
``resample._prototype``, its output length against Python's, the kernel's phase functions (resample_kernel.h) driven
on the CPU by tests/emu/libmgx_emu_resample.so against ``resample.resample``, and what ``mgx_resample`` decides
before it touches a handle, through the real libmgx.so.
"""

import ctypes

import numpy as np
import pytest

import emu_build
from matchering_amd import _native
from matchering_amd import resample as host

# the rate pairs of the converter's design table (every file rate the loaders commonly meet, both directions)
PAIRS = [(48000, 44100), (44100, 48000), (96000, 44100), (192000, 44100), (8000, 44100), (32000, 44100),
         (22050, 44100), (88200, 44100)]
SHAPE = {(48000, 44100): (147, 160, 140), (44100, 48000): (160, 147, 130), (96000, 44100): (147, 320, 280),
         (192000, 44100): (147, 640, 562), (8000, 44100): (441, 80, 130), (32000, 44100): (441, 320, 130),
         (22050, 44100): (2, 1, 130), (88200, 44100): (1, 2, 258)}


@pytest.fixture(scope="module")
def emu():
    lib = emu_build.load("resample")
    lib.emu_resample_length.restype = ctypes.c_longlong
    lib.emu_resample_length.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    lib.emu_resample_launch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p]
    lib.emu_resample.restype = ctypes.c_longlong
    lib.emu_resample.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_void_p, ctypes.c_void_p]
    return lib


def prototype_rows(sr, new):
    """rows[p][k], the weight of x[n - (k - taps)] at phase p, read off ``resample._prototype``: the left wing's
    weight of x[n - i] sits at tap centre + p + i L of the prototype, the right wing's at negative i."""
    plan = host._Plan(sr, new)
    g = int(np.gcd(sr, new))
    phases, hop = new // g, sr // g
    proto, centre = host._prototype(plan, phases, hop)
    i = np.arange(2 * plan.taps) - plan.taps
    return proto[centre + np.arange(phases)[:, None] + i[None, :] * phases], phases, hop, plan.taps


def plan_rows(emu, sr, new):
    geometry = (ctypes.c_int * 6)()
    assert emu.emu_resample_geometry(sr, new, geometry) == 0
    phases, hop, taps, width = list(geometry)[:4]
    rows = np.zeros((phases, width))
    row_sum = ctypes.c_double()
    assert emu.emu_resample_rows(sr, new, rows.ctypes.data_as(ctypes.c_void_p), ctypes.byref(row_sum)) == 0
    return rows, (phases, hop, taps, width), row_sum.value


@pytest.mark.parametrize("sr,new", PAIRS)
def test_plan_rows_are_the_prototypes(emu, sr, new):
    """A row entry is a convex interpolation of two entries of the Kaiser table plus one rounding; two implementations
    of that table agree to 1e-15 (tests/test_resample.py), so the rows agree to 2e-15."""
    want, phases, hop, taps = prototype_rows(sr, new)
    got, shape, row_sum = plan_rows(emu, sr, new)
    assert shape == (phases, hop, taps, 2 * taps)
    assert (phases, hop, 2 * taps) == SHAPE[(sr, new)]
    worst = float(np.abs(got - want).max())
    print(f"{sr} -> {new}: L {phases} M {hop} W {2 * taps}, max row difference {worst:.2e}")
    assert worst <= 2e-15
    assert row_sum == pytest.approx(float(np.abs(want).sum(axis=1).max()), rel=1e-12)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("sr,new", PAIRS)
def test_the_launch_is_the_geometrys(emu, sr, new, channels):
    """What ``resample_launch`` gives ``mgx_resample`` and the emulation alike: LDS for the geometry's span, within what
    a launch may ask for (RESAMPLE_SPAN_MAX stereo frames), and a workgroup per 256 outputs."""
    geometry = (ctypes.c_int * 6)()
    assert emu.emu_resample_geometry(sr, new, geometry) == 0
    span, tile = geometry[5], 256
    launch = (ctypes.c_longlong * 2)()
    for n_out in (1, tile - 1, tile, tile + 1):
        assert emu.emu_resample_launch(sr, new, channels, n_out, launch) == 0
        grid, lds = launch
        assert lds == span * channels * 4
        assert lds <= 7680 * 8
        assert grid == -(-n_out // tile), (n_out, grid)
    assert emu.emu_resample_launch(44100, 44101, channels, 1, launch) == -1


def test_output_length_is_pythons(emu):
    """trunc((double) n * ((double) new / (double) sr)) is ``int(n * plan.ratio)``, the same IEEE operations, for
    lengths up to and around an hour of audio."""
    rng = np.random.RandomState(11)
    rates = [8000, 11025, 16000, 22050, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 44101, 47999]
    checked = 0
    for sr in rates:
        for new in rates:
            if sr == new:
                continue
            hour = 3600 * sr
            lengths = np.concatenate([np.arange(0, 12), rng.randint(0, 10 * sr, 12), hour + rng.randint(-sr, sr, 12),
                                      [hour - 1, hour, hour + 1, 2 * hour + 7]])
            for n in lengths:
                assert emu.emu_resample_length(int(n), sr, new) == int(int(n) * host._Plan(sr, new).ratio), (n, sr, new)
                checked += 1
    assert checked >= 4000


def emulated(emu, x, sr, new):
    """(float64 sums before the store's rounding, float32 frames as stored) of the kernel's phases on the CPU."""
    n, channels = x.shape
    n_out = int(n * (float(new) / sr))
    sums, out = np.zeros((n_out, 2)), np.full((n_out, 2), np.nan, dtype=np.float32)
    rc = emu.emu_resample(x.ctypes.data_as(ctypes.c_void_p), n, channels, sr, new, sums.ctypes.data_as(ctypes.c_void_p),
                          out.ctypes.data_as(ctypes.c_void_p))
    assert rc == n_out, rc
    return sums, out


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("n", [5, 300, 700, 3000])
@pytest.mark.parametrize("sr,new", PAIRS)
def test_emulated_kernel_is_the_host_resampler(emu, sr, new, n, channels):
    """The kernel's sum in float64, before its one rounding to float32, against ``resample.resample`` of the same
    float32-valued input, array ends included.  Bound: max|x| (sum|w| W 2^-53 + W 2e-15) -- the rounding of W float64
    accumulations of terms bounded by the largest row sum, plus the plan tolerance carried through the sum -- computed
    from the plan.  A mono track comes out as two equal columns (dsp.py:45-46)."""
    rng = np.random.RandomState(sr % 997 + n + channels)
    x = (0.3 * rng.randn(n, channels)).astype(np.float32)
    _, (_, _, _, width), row_sum = plan_rows(emu, sr, new)
    sums, out = emulated(emu, x, sr, new)
    want = host.resample(np.repeat(x, 2, axis=1).astype(np.float64) if channels == 1 else x.astype(np.float64), sr, new)
    assert sums.shape == want.shape
    if want.size == 0:
        return
    bound = float(np.abs(x).max()) * (row_sum * width * 2.0 ** -53 + width * 2e-15)
    worst = float(np.abs(sums - want).max())
    print(f"{sr} -> {new}, {n} frames x {channels}: {worst:.2e} (bound {bound:.2e})")
    assert worst <= bound
    assert np.array_equal(out, sums.astype(np.float32))            # the store rounds once, and writes every frame
    if channels == 1:
        assert np.array_equal(out[:, 0], out[:, 1])


def test_emulated_kernel_far_into_a_file(emu):
    """Twenty-one seconds of 48 kHz: the last workgroups' phases come from the 64-bit t M / L, compared on a window at
    the end."""
    x = (0.3 * np.random.RandomState(5).randn(48000 * 21, 2)).astype(np.float32)
    sums, _ = emulated(emu, x, 48000, 44100)
    want = host.resample(x.astype(np.float64), 48000, 44100)
    _, (_, _, _, width), row_sum = plan_rows(emu, 48000, 44100)
    bound = float(np.abs(x).max()) * (row_sum * width * 2.0 ** -53 + width * 2e-15)
    assert float(np.abs(sums[-5000:] - want[-5000:]).max()) <= bound


def test_the_plan_refuses_what_the_host_path_does_literally(emu):
    geometry = (ctypes.c_int * 6)()
    assert emu.emu_resample_geometry(44100, 44101, geometry) == -1           # 44101 phases > 4096
    assert emu.emu_resample_geometry(44100, 48000, geometry) == 0
    assert emu.emu_resample_geometry(192000, 8000, geometry) == -1           # 256 outputs would reach 6000 + 6146 frames
    assert emu.emu_resample_geometry(1000000, 1000, geometry) == -1          # table stride int(scale * 512) = 0


def test_mgx_resample_decides_before_it_touches_the_handle():
    """Argument checks, the refusal of more than 4096 phases and the output length need no device: asserted through
    the real library with a null handle."""
    lib = _native.library()
    n_out = ctypes.c_int64(-7)

    def call(n, channels, rate_in, rate_out, out=None, capacity=0):
        return lib.mgx_resample(None, None, n, channels, rate_in, rate_out, out, capacity, ctypes.byref(n_out))

    assert lib.mgx_version() >= 101
    assert call(1000, 3, 48000, 44100) == -1 and b"channels" in lib.mgx_last_error()          # MGX_ERR_ARGUMENT
    assert call(1000, 0, 48000, 44100) == -1
    assert call(1000, 2, 0, 44100) == -1 and call(1000, 2, 48000, -5) == -1
    assert call(1000, 2, 44100, 44100) == -1
    assert call(1000, 2, 44100, 44101) == _native.ERR_UNSUPPORTED and b"4096" in lib.mgx_last_error()
    assert n_out.value == -7                                                                    # nothing reported so far
    assert call(48000 * 480, 2, 48000, 44100) == 0 and n_out.value == 44100 * 480               # the length only
    assert call(3, 1, 48000, 44100) == 0 and n_out.value == 2
    assert call(1, 1, 48000, 44100) == 0 and n_out.value == 0
    # with somewhere to write, a handle is needed
    somewhere = ctypes.c_void_p(4096)
    assert call(1000, 2, 48000, 44100, somewhere, 918) == -1
    assert lib.mgx_resample(None, None, 1000, 2, 48000, 44100, None, 0, None) == -1
    handle = ctypes.c_void_p()
    ptr, phases, width, designed = ctypes.c_void_p(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    assert lib.mgx_resample_plan(handle, 48000, 44100, ctypes.byref(ptr), ctypes.byref(phases), ctypes.byref(width),
                                 ctypes.byref(designed)) == -1


def test_checker_leaves_the_conversion_to_the_device_when_told():
    """``check(on_device=True)`` emits what the host path emits for the same file, in the same order, raises the same
    codes, and does not read or change the samples."""
    import matchering_amd as mg
    from matchering_amd import checker
    from matchering_amd.config import Config
    from matchering_amd.log import Code, ModuleError

    config = Config()
    mono = np.zeros((48000 * 3, 1), dtype=np.int16)
    mono[100, 0] = 20000

    def run(**kw):
        seen = []
        mg.log(info_handler=seen.append, warning_handler=seen.append, show_codes=True)
        try:
            out = checker.check(mono, 48000, config, "target", **kw)
        finally:
            mg.log()
        return seen, out

    host_codes, (converted, rate) = run()
    peaks = checker.count_max_peaks(converted)
    device_codes, (same, device_rate) = run(peaks=peaks, on_device=True)
    assert device_codes == host_codes and len(host_codes) == 2
    assert same is mono and rate == device_rate == config.internal_sample_rate
    with pytest.raises(ValueError):
        checker.check(mono, 48000, config, "target", on_device=True)            # no statistics: nothing to warn from
    with pytest.raises(ModuleError) as short:
        checker.check(mono[:4000], 48000, config, "target", peaks=checker.LATER, on_device=True)
    assert short.value.code == Code.ERROR_TARGET_LENGTH_IS_TOO_SMALL
    wide = np.zeros((48000 * 3, 3), dtype=np.int16)
    with pytest.raises(ModuleError) as many:
        checker.check(wide, 48000, config, "reference", on_device=True)
    assert many.value.code == Code.ERROR_REFERENCE_NUM_OF_CHANNELS_IS_EXCEEDED
