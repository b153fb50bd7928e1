"""The stage sweeps of tests/stage_sweeps.py through the CPU emulation (tests/emu): the kernels' own phase functions,
driven thread by thread, against the float64 references -- the cases tests/test_gpu_stage_sweeps.py runs on the GPU, here
where they can be run and debugged without one.

Left out, because the emulation has no twin of the kernel or of the decision:
  * analysis at fft_size 8, 16 and 32 (k_analyze_small is a kernel of its own, not a set of phase functions), the
    grid-filling cases (`grid_full`, `second_trip`: the emulation deals segments by its own rule, five per chunk);
  * convolution at 2 .. 32 taps (k_conv_direct, likewise) and the lengths with more blocks than a grid holds (the
    emulation has no grid);
  * the limiter's n = 7 refusal (limiter_args is host code of the library) and the bit-for-bit comparison of its
    instantiations (one template on the CPU).
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import stage_sweeps as sw

c_float_p = ctypes.POINTER(ctypes.c_float)
c_double_p = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def emu():
    return sw.load_emulation()


def _fp(a):
    return a.ctypes.data_as(c_float_p)


def _dp(a):
    return a.ctypes.data_as(c_double_p)


# ---- A. analysis ----------------------------------------------------------------------------------------------------
def emu_analyze(emu, x32, cfg, is_reference):
    n = x32.shape[0]
    native = cfg.to_native()
    max_div = int(n / cfg.max_piece_size) + 1
    half = cfg.fft_size // 2
    peak, amp, match = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    div, piece = ctypes.c_int(), ctypes.c_longlong()
    rms = np.zeros(max_div)
    loud = np.zeros(max_div, dtype=np.int32)
    avg_mid, avg_side = np.zeros(half + 1), np.zeros(half + 1)
    rc = emu.emu_analyze(_fp(x32), ctypes.c_longlong(n), ctypes.byref(native), int(is_reference), ctypes.byref(peak),
                         ctypes.byref(amp), ctypes.byref(match), ctypes.byref(div), ctypes.byref(piece), _dp(rms),
                         loud.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _dp(avg_mid), _dp(avg_side))
    assert rc == 0
    d = div.value
    return SimpleNamespace(peak=peak.value, amplitude_coefficient=amp.value, match_rms=match.value, divisions=d,
                           piece_size=piece.value, rmses=rms[:d].copy(), loud=loud[:d].astype(bool),
                           average_spectrum_mid=avg_mid, average_spectrum_side=avg_side)


EMU_FFT_SIZES = [f for f in sw.FFT_SIZES if f >= 64]
ANALYSIS_CASES = [(f, name) for f in EMU_FFT_SIZES for name, case in sw.analysis_cases(f).items() if case["emu"]]


@pytest.mark.parametrize("kind", ["comb", "noise"])
@pytest.mark.parametrize("fft,name", ANALYSIS_CASES)
def test_analysis_every_size_per_bin(emu, fft, name, kind):
    case = sw.analysis_cases(fft)[name]
    cfg, ocfg = sw.analysis_configs(fft, case)
    x = sw.analysis_input(fft, case, kind)
    for is_reference in (False, True):
        ref = sw.analysis_reference(x, ocfg, is_reference, case, fft)
        if kind == "comb":
            for closed, measured in zip(sw.comb_closed_form(fft, case, ref), (ref.avg_mid, ref.avg_side)):
                assert np.abs(closed - measured).max() <= 1e-6 * measured.max()
        st = emu_analyze(emu, x, cfg, is_reference)
        key = f"fft={fft} {name} {kind} ref={int(is_reference)}"
        worst = sw.check_analysis(st, x, ref, is_reference, key)
        sw.record("analyze", key, worst, sw.analysis_yardstick(x, ref, fft))


@pytest.mark.parametrize("kind", ["mono", "panned"])
@pytest.mark.parametrize("fft", [4096, 65536])
def test_analysis_of_mono_and_hard_panned_tracks(emu, fft, kind):
    case = sw.analysis_cases(fft)["leftover_peak"]
    cfg, ocfg = sw.analysis_configs(fft, case)
    x = sw.analysis_input(fft, case, kind)
    for is_reference in (False, True):
        ref = sw.analysis_reference(x, ocfg, is_reference, case, fft)
        st = emu_analyze(emu, x, cfg, is_reference)
        sw.check_analysis(st, x, ref, is_reference, f"fft={fft} {kind} ref={int(is_reference)}", mono_side=kind == "mono")


# ---- B. convolution -------------------------------------------------------------------------------------------------
def emu_convolve(emu, x, hm, hs, gain, taps):
    """The form run_conv (run_conv.h) takes for this tap count."""
    n = x.shape[0]
    x = np.ascontiguousarray(x, dtype=np.float32)
    y, ymid = np.zeros((n, 2), dtype=np.float32), np.zeros(n, dtype=np.float32)
    hm, hs = np.ascontiguousarray(hm, dtype=np.float64), np.ascontiguousarray(hs, dtype=np.float64)
    route, hop, _ = sw.conv_route(taps)
    head = (_fp(x), ctypes.c_longlong(n), _dp(hm), _dp(hs), ctypes.c_int(taps), ctypes.c_double(gain), _fp(y), _fp(ymid))
    if route in ("wide", "delay"):
        peaks = np.zeros((n + hop - 1) // hop, dtype=np.float32)
        if route == "wide":
            rc = emu.emu_convolve_wide(*head, _fp(peaks))
        else:
            rc = emu.emu_convolve_delay(*head, _fp(peaks), ctypes.c_int(3))
        peak = float(peaks.max())
    else:
        pk = ctypes.c_double()
        rc = emu.emu_convolve_blocked(*head, ctypes.byref(pk), ctypes.c_int(14 if route == "partitioned" else 0))
        peak = pk.value
    assert rc == 0
    return y, ymid, peak


EMU_TAP_COUNTS = [t for t in sw.TAP_COUNTS if t >= 64]


def emu_lengths(taps):
    return sw.conv_lengths(taps, with_grid_overflow=False)


@pytest.mark.parametrize("taps", EMU_TAP_COUNTS)
def test_convolution_every_route_on_noise(emu, taps):
    hm, hs = sw.conv_taps(taps, "random", taps)
    for n in emu_lengths(taps):
        x = sw.conv_noise(n, taps + n)
        y, ymid, peak = emu_convolve(emu, x, hm, hs, 1.3, taps)
        sw.check_convolution(y, ymid, peak, x, hm, hs, 1.3, taps, f"noise n={n}")


@pytest.mark.parametrize("taps", EMU_TAP_COUNTS)
def test_convolution_of_impulses_on_the_edges(emu, taps):
    hm, hs = sw.conv_taps(taps, "range60", taps + 1)
    for n in emu_lengths(taps):
        x = sw.conv_edge_impulses(n, taps)
        y, ymid, peak = emu_convolve(emu, x, hm, hs, 1.0, taps)
        sw.check_convolution(y, ymid, peak, x, hm, hs, 1.0, taps, f"impulses n={n}")


@pytest.mark.parametrize("where", ["first", "last", "centre"])
@pytest.mark.parametrize("taps", [2048, 4096, 16384, 65536])
def test_convolution_with_delta_filters(emu, taps, where):
    h, at = sw.conv_delta(taps, where)
    hop = sw.conv_route(taps)[1]
    n = (3 * hop + 777) | 1
    n = max(n, taps // 2 + 3)                                # (so that a delta on tap 0 still leaves frames to see)
    x = sw.conv_noise(n, taps + at)
    y, ymid, peak = emu_convolve(emu, x, h, h, 1.0, taps)
    sw.check_convolution(y, ymid, peak, x, h, h, 1.0, taps, f"delta@{where} n={n}")
    # the output is the input shifted by (taps - 1) // 2 - at frames, zero-filled
    shift = (taps - 1) // 2 - at
    want = np.zeros_like(x)
    if shift >= 0:
        want[: n - shift] = x[shift:]
    else:
        want[-shift:] = x[: n + shift]
    assert np.abs(y - want).max() <= 2e-6                   # (test_convolution_identity's bound)


# ---- C. limiter -----------------------------------------------------------------------------------------------------
limiter_geometry = sw.limiter_geometry


def emu_limit(emu, x, cfg):
    out = np.zeros_like(x)
    native = cfg.to_native()
    rc = emu.emu_limit(_fp(x), ctypes.c_longlong(x.shape[0]), ctypes.byref(native), ctypes.c_double(1.0),
                       ctypes.c_double(1.0), _fp(out), None, None)
    assert rc == 0
    return out


def test_limiter_geometry_export_matches_what_the_kernels_are_built_for(emu):
    """The geometries launch_limiter_256 (run_limiter.h) has instantiations for, from the library's own rule."""
    import matchering_amd as mg

    g = limiter_geometry(emu, mg.Config())
    assert (g.threads, g.gl, g.gr, g.general) == (256, 6, 26, 0) and g.chunk == 16 * g.core_blocks == 16 * (256 - 32)
    g = limiter_geometry(emu, sw.limiter_configs("96000")[0])
    assert (g.threads, g.gl, g.gr) == (256, 12, 55) and g.chunk == 16 * (256 - 67)
    g = limiter_geometry(emu, sw.limiter_configs("long_attack")[0])
    assert g.threads == 1024 and g.chunk == 16 * (1024 - g.gl - g.gr)
    assert limiter_geometry(emu, sw.limiter_configs("orders_2_2")[0]).general == 2
    assert limiter_geometry(emu, sw.limiter_configs("orders_3_1")[0]).general == 3
    refused = mg.Config(limiter=mg.LimiterConfig(release_filter_order=3)).to_native()
    assert emu.emu_limiter_geometry(ctypes.byref(refused), None, None, None, None, None, None) == -1


def limiter_sweep(emu, name, kind):
    """Every length of the sweep: yields (n, frames, output)."""
    cfg, ocfg = sw.limiter_configs(name)
    geo = limiter_geometry(emu, cfg)
    for n in sw.limiter_lengths(geo.chunk):
        if kind == "noise":
            x = sw.limiter_noise(n)
        else:
            x, places = sw.limiter_spikes(n, geo.chunk, ocfg.threshold)
            assert len(places) == (4 if n > geo.chunk + 1 else 3 if n > geo.chunk else 2)
        yield n, x, emu_limit(emu, x, cfg)


@pytest.mark.parametrize("kind", ["noise", "spikes"])
@pytest.mark.parametrize("name", sorted(sw.LIMITER_CONFIGS))
def test_limiter_lengths_around_chunk_seams(emu, name, kind):
    cfg, ocfg = sw.limiter_configs(name)
    general = limiter_geometry(emu, cfg).general != 0
    for n, x, out in limiter_sweep(emu, name, kind):
        sw.check_limiter(out, None, x, ocfg, general, f"{name} {kind} n={n}")


FIRST_ORDER = sorted(k for k, v in sw.LIMITER_CONFIGS.items() if "hold_filter_order" not in v)


@pytest.mark.parametrize("kind", ["noise", "spikes"])
@pytest.mark.parametrize("name", FIRST_ORDER)
def test_limiter_first_and_last_64_frames(emu, name, kind):
    """The first and last 64 frames of every length to 1e-6, the bound tests/test_gpu_parity.py::test_limiter_stage
    holds on its tracks.

    Worst over the lengths: 7.5e-8 on the spikes, 2.1e-7 .. 5.0e-7 on the noise.  0.9 randn reaches 3.5 times full scale,
    so an error of the gain counts 3.5-fold there: with the filters' poles rounded to float32 (iir1_step in
    limiter_kernel.h tells what replaced them) these frames were off by 8.2e-7 .. 1.2e-6, in the middle of a track as at
    its ends."""
    cfg, ocfg = sw.limiter_configs(name)
    worst = 0.0
    for n, x, out in limiter_sweep(emu, name, kind):
        worst = max(worst, sw.check_limiter(out, None, x, ocfg, False, f"{name} {kind} n={n}")[1])
    assert worst <= sw.LIMITER_EDGE_BOUND, (name, kind, worst)
