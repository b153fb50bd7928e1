"""Every analysis, convolution, limiter and scale route of libmgx on the GPU, at its block edges, against a float64
reference of the same operation (tests/stage_sweeps.py holds the cases, inputs, references and yardsticks;
tests/test_emu_stage_sweeps.py runs the same cases through the CPU emulation).

Kernels reached: k_analyze_small<3..5>, k_analyze<6..14>, k_analyze_double<14>, k_analyze_quad<14>; k_conv_direct,
k_conv<7..12> and <14> (one partition, and four and eight), k_conv_wide<14>, k_conv_delay<14>; k_limit<256,4,...> in its three
specialised and its general instantiation, k_limit<1024,1>, k_limit_general<2> and <3>; k_scale_outputs in its three
paths.

Measured on an MI355X (largest error over the cases of a size; `yardstick` = scipy in float32 on the same input):

  analysis, largest error of a bin of the average spectra, of the peak bin (bound 2e-6):

    fft_size  kernel              kernel   yardstick
           8  k_analyze_small     1.1e-07  1.1e-07
          16  k_analyze_small     1.3e-07  8.3e-08
          32  k_analyze_small     1.0e-07  1.8e-07
          64  k_analyze           1.2e-07  1.1e-07
         128  k_analyze           1.0e-07  1.3e-07
         256  k_analyze           1.6e-07  1.2e-07
         512  k_analyze           1.5e-07  1.7e-07
        1024  k_analyze           1.7e-07  1.7e-07
        2048  k_analyze           2.1e-07  1.5e-07
        4096  k_analyze           2.1e-07  1.4e-07
        8192  k_analyze           2.3e-07  1.5e-07
       16384  k_analyze           2.0e-07  1.6e-07
       32768  k_analyze_double    2.0e-07  1.9e-07
       65536  k_analyze_quad      1.9e-07  1.9e-07

  convolution, largest error of a frame (bound: 8 x the yardstick on the same input, at most 5e-6); `ratio` is the
  largest kernel / yardstick of a single case:

    taps   route        kernel   yardstick  ratio
        2  direct       3.6e-07  8.8e-07    0.6
        4  direct       2.3e-07  5.0e-07    0.8
        8  direct       5.4e-07  8.8e-07    1.1
       16  direct       3.3e-07  6.2e-07    1.4
       32  direct       4.6e-07  6.5e-07    1.2
       64  queue        5.6e-07  5.5e-07    2.4
      128  queue        6.2e-07  4.7e-07    2.2
      256  queue        6.9e-07  5.4e-07    2.7
      512  queue        6.8e-07  4.8e-07    2.6
     1024  queue        6.8e-07  5.3e-07    2.5
     2048  queue        4.8e-07  2.6e-07    2.1
     4096  wide         4.9e-07  3.3e-07    2.1
     8192  queue        5.4e-07  3.6e-07    2.3
    16384  delay        5.6e-07  4.0e-07    2.7
    32768  partitioned  5.2e-07  3.5e-07    2.1
    65536  partitioned  5.2e-07  3.8e-07    2.1

  limiter, largest error of a frame over the eleven lengths (bounds 5e-6, and 1e-5 for the filters of order 2 and 3):
  6.5e-7 .. 1.1e-6 on the noise (3.3e-7 with 0.1 ms windows), 7.9e-8 .. 9.4e-8 on the spikes; RMS at most 7.3e-8; first and
  last 64 frames (bound 1e-6) at most 6.4e-7.
  mgx_scale: exact.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import stage_sweeps as sw
from conftest import ROOT

pytestmark = pytest.mark.gpu


# ---- A. analysis ----------------------------------------------------------------------------------------------------
ANALYSIS_CASES = [(f, name) for f in sw.FFT_SIZES for name in sw.analysis_cases(f)]


@pytest.mark.parametrize("kind", ["comb", "noise"])
@pytest.mark.parametrize("fft,name", ANALYSIS_CASES)
def test_analysis_every_size_per_bin(fft, name, kind):
    from matchering_amd import kernels

    case = sw.analysis_cases(fft)[name]
    cfg, ocfg = sw.analysis_configs(fft, case)
    x = sw.analysis_input(fft, case, kind)
    for is_reference in (False, True):
        ref = sw.analysis_reference(x, ocfg, is_reference, case, fft)
        if kind == "comb":
            for closed, measured in zip(sw.comb_closed_form(fft, case, ref), (ref.avg_mid, ref.avg_side)):
                assert np.abs(closed - measured).max() <= 1e-6 * measured.max()
        st = kernels.analyze(x, cfg, is_reference=is_reference)
        key = f"fft={fft} {name} {kind} ref={int(is_reference)}"
        yard = sw.analysis_yardstick(x, ref, fft)
        worst = sw.check_analysis(st, x, ref, is_reference, key)
        sw.record("analyze", key, worst, yard)


@pytest.mark.parametrize("kind", ["mono", "panned"])
@pytest.mark.parametrize("fft", [16, 4096, 65536])
def test_analysis_of_mono_and_hard_panned_tracks(fft, kind):
    from matchering_amd import kernels

    case = sw.analysis_cases(fft)["leftover_peak"]
    cfg, ocfg = sw.analysis_configs(fft, case)
    x = sw.analysis_input(fft, case, kind)
    for is_reference in (False, True):
        ref = sw.analysis_reference(x, ocfg, is_reference, case, fft)
        st = kernels.analyze(x, cfg, is_reference=is_reference)
        sw.check_analysis(st, x, ref, is_reference, f"fft={fft} {kind} ref={int(is_reference)}", mono_side=kind == "mono")


# ---- B. convolution -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", sw.TAP_COUNTS)
def test_convolution_every_route_on_noise(taps):
    from matchering_amd import kernels

    hm, hs = sw.conv_taps(taps, "random", taps)
    for n in sw.conv_lengths(taps):
        x = sw.conv_noise(n, taps + n)
        y, ymid, peak = kernels.convolve(x, hm, hs, gain=1.3)
        sw.check_convolution(y, ymid, peak, x, hm, hs, 1.3, taps, f"noise n={n}")


@pytest.mark.parametrize("taps", sw.TAP_COUNTS)
def test_convolution_of_impulses_on_the_edges(taps):
    from matchering_amd import kernels

    hm, hs = sw.conv_taps(taps, "range60", taps + 1)
    for n in sw.conv_lengths(taps, with_grid_overflow=False):
        x = sw.conv_edge_impulses(n, taps)
        y, ymid, peak = kernels.convolve(x, hm, hs, gain=1.0)
        sw.check_convolution(y, ymid, peak, x, hm, hs, 1.0, taps, f"impulses n={n}")


@pytest.mark.parametrize("where", ["first", "last", "centre"])
@pytest.mark.parametrize("taps", [32, 2048, 4096, 16384, 65536])
def test_convolution_with_delta_filters(taps, where):
    from matchering_amd import kernels

    h, at = sw.conv_delta(taps, where)
    hop = sw.conv_route(taps)[1]
    n = max((3 * hop + 777) | 1, taps // 2 + 3)             # (so that a delta on tap 0 still leaves frames to see)
    x = sw.conv_noise(n, taps + at)
    y, ymid, peak = kernels.convolve(x, h, h, gain=1.0)
    sw.check_convolution(y, ymid, peak, x, h, h, 1.0, taps, f"delta@{where} n={n}")
    # the output is the input shifted by (taps - 1) // 2 - at frames, zero-filled
    shift = (taps - 1) // 2 - at
    want = np.zeros_like(x)
    if shift >= 0:
        want[: n - shift] = x[shift:]
    else:
        want[-shift:] = x[: n + shift]
    assert np.abs(y - want).max() <= 2e-6                   # (test_convolution_identity_and_linearity's bound)


# ---- C. limiter -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def geometry():
    """Chunk geometry of a configuration from the library's own rule (host_params.h limiter_params), through the
    emulation's export."""
    emu = sw.load_emulation()
    return lambda cfg: sw.limiter_geometry(emu, cfg)


def limiter_sweep(geometry, name, kind):
    """Every length of the sweep, each a launch of its own: yields (n, frames, output, active)."""
    from matchering_amd import kernels

    cfg, ocfg = sw.limiter_configs(name)
    geo = geometry(cfg)
    for n in sw.limiter_lengths(geo.chunk):
        x = sw.limiter_noise(n) if kind == "noise" else sw.limiter_spikes(n, geo.chunk, ocfg.threshold)[0]
        out, active = kernels.limit(x, cfg)
        yield n, x, out, active


@pytest.mark.parametrize("kind", ["noise", "spikes"])
@pytest.mark.parametrize("name", sorted(sw.LIMITER_CONFIGS))
def test_limiter_lengths_around_chunk_seams(geometry, name, kind):
    cfg, ocfg = sw.limiter_configs(name)
    general = geometry(cfg).general != 0
    for n, x, out, active in limiter_sweep(geometry, name, kind):
        sw.check_limiter(out, active, x, ocfg, general, f"{name} {kind} n={n}")


FIRST_ORDER = sorted(k for k, v in sw.LIMITER_CONFIGS.items() if "hold_filter_order" not in v)


@pytest.mark.parametrize("kind", ["noise", "spikes"])
@pytest.mark.parametrize("name", FIRST_ORDER)
def test_limiter_first_and_last_64_frames(geometry, name, kind):
    """The first and last 64 frames of every length to 1e-6, the bound test_limiter_stage holds on its tracks.

    Worst over the lengths on an MI355X: 9.4e-8 on the spikes, 2.1e-7 .. 6.4e-7 on the noise (tests/test_emu_stage_sweeps.py
    tells why the noise is the harder input)."""
    cfg, ocfg = sw.limiter_configs(name)
    worst = 0.0
    for n, x, out, active in limiter_sweep(geometry, name, kind):
        worst = max(worst, sw.check_limiter(out, active, x, ocfg, False, f"{name} {kind} n={n}")[1])
    assert worst <= sw.LIMITER_EDGE_BOUND, (name, kind, worst)


def test_limiter_refuses_seven_frames():
    """limiter_args (run_limiter.h) takes eight frames at least: the lower edge of the sweep is the library's own."""
    import matchering_amd as mg
    from matchering_amd import kernels
    from matchering_amd._native import MgxError

    with pytest.raises(MgxError) as failure:
        kernels.limit(sw.limiter_noise(7), mg.Config())
    assert failure.value.code == -1                              # MGX_ERR_ARGUMENT
    out, active = kernels.limit(sw.limiter_noise(8), mg.Config())
    assert out.shape == (8, 2) and active


# the specialised instantiations of k_limit<256, 4, HW, HB, GR> against the general one, bit for bit: a test
# build whose launch_limiter_256 always takes its last branch, in a child process (a process loads one libmgx)
BUILD_DIR = os.path.join(ROOT, "tests", "_build")
GENERAL_VARIANT = os.path.join(BUILD_DIR, "libmgx_limitgeneral.so")
GENERAL_FLAGS = ("-DMGX_TEST_LIMIT_GENERAL",)

LIMIT_CHILD = r"""
import sys
sys.path[:0] = [{root!r}, {root!r} + "/oracle", {root!r} + "/tests", {root!r} + "/tests/golden"]
import numpy as np
import stage_sweeps as sw
from matchering_amd import kernels

for name, chunk in {jobs!r}:
    cfg, _ = sw.limiter_configs(name)
    out, active = kernels.limit(sw.limiter_noise(5 * chunk + 7), cfg)
    np.save({folder!r} + "/" + name + ".npy", out)
print("done")
"""


def test_specialised_limiter_instantiations_equal_the_general_one_bit_for_bit(geometry, tmp_path):
    sys.path.insert(0, ROOT)
    from matchering_amd import build as native_build
    from matchering_amd import kernels

    assert not any(f.startswith("-DMGX_TEST") for f in native_build.FLAGS)
    os.makedirs(BUILD_DIR, exist_ok=True)
    lib = native_build.build(out=GENERAL_VARIANT, extra_flags=GENERAL_FLAGS)
    jobs = [(name, geometry(sw.limiter_configs(name)[0]).chunk) for name in sw.SPECIALISED]
    child = LIMIT_CHILD.format(root=ROOT, jobs=jobs, folder=str(tmp_path))
    done = subprocess.run([sys.executable, "-c", child], env=dict(os.environ, MGX_LIB=lib), capture_output=True, text=True,
                          timeout=600)
    assert done.returncode == 0 and "done" in done.stdout, done.stderr[-2000:]
    for name, chunk in jobs:
        cfg, _ = sw.limiter_configs(name)
        out, active = kernels.limit(sw.limiter_noise(5 * chunk + 7), cfg)
        general = np.load(os.path.join(str(tmp_path), name + ".npy"))
        assert active and np.abs(out).max() > 0.5
        assert out.dtype == general.dtype and np.array_equal(out.view(np.uint32), general.view(np.uint32)), name


# ---- D. scale -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sw.SCALE_LENGTHS)
def test_scale_rounds_once(n):
    from matchering_amd import kernels

    x = sw.scale_input(n)
    for gain in sw.SCALE_GAINS:
        got = kernels.scale(x, gain)
        assert got.dtype == np.float32 and np.array_equal(got, sw.scale_reference(x, gain)), (n, gain)


def _raw_scale(x, gain, lead):
    """mgx_scale with source and destination `lead` frames into their allocations and one frame of room behind:
    returns the whole destination, sentinel frames included."""
    from matchering_amd._native import check, library
    from matchering_amd.device import default_device

    n = x.shape[0]
    dev = default_device()
    src = np.full((lead + n + 1, 2), sw.SENTINEL, dtype=np.float32)
    src[lead:lead + n] = x
    with dev.lock:
        xb, ob = dev.upload(src), dev.upload(np.full((lead + n + 1, 2), sw.SENTINEL, dtype=np.float32))
        try:
            assert xb.ptr % 16 == 0 and ob.ptr % 16 == 0
            check(library().mgx_scale(dev.handle, ctypes.c_void_p(xb.ptr + 8 * lead), n, float(gain),
                                      ctypes.c_void_p(ob.ptr + 8 * lead)))
            dev.synchronize()
            return np.array(dev.download(ob, (lead + n + 1, 2)))
        finally:
            xb.release()
            ob.release()


@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "eight_bytes_in"])
@pytest.mark.parametrize("n", sw.SCALE_LENGTHS)
def test_scale_writes_its_frames_and_no_others(n, lead):
    """lead = 1: both buffers 8 bytes into their allocations, the kernel's path for buffers that are not 16-byte
    aligned.  lead = 0: the 16-byte path and, at odd n, the last frame alone.  Frames before and after stay as they were."""
    x = sw.scale_input(n)
    for gain in sw.SCALE_GAINS:
        whole = _raw_scale(x, gain, lead)
        assert np.array_equal(whole[lead:lead + n], sw.scale_reference(x, gain)), (n, gain)
        assert np.all(whole[:lead] == sw.SENTINEL) and np.all(whole[lead + n:] == sw.SENTINEL), (n, gain)


def test_scale_of_no_frames_succeeds_and_launches_nothing():
    """mgx_scale with n == 0 answers success without a launch (as mgx_resample does for an empty conversion); a negative
    count is an argument error."""
    from matchering_amd._native import library

    whole = _raw_scale(np.zeros((0, 2), dtype=np.float32), 2.0, 1)
    assert whole.shape == (2, 2) and np.all(whole == sw.SENTINEL)
    from matchering_amd.device import default_device

    dev = default_device()
    with dev.lock:
        buf = dev.alloc(64)
        try:
            rc = library().mgx_scale(dev.handle, ctypes.c_void_p(buf.ptr), -1, 1.0, ctypes.c_void_p(buf.ptr))
        finally:
            buf.release()
    assert rc == -1                                              # MGX_ERR_ARGUMENT
