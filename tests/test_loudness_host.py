"""The loudness meter without a GPU: the host plan of csrc/loudness_plan.cpp against the published tables and the oracle,
the kernel's phase functions (loudness_kernel.h) driven on the CPU by tests/emu/libmgx_emu_loudness.so against
tests/loudness_oracle.py at the bounds the GPU suite asserts, ``mgx_loudness_gate`` through the real libmgx.so, the EBU
Tech 3341 / 3342 known answers, and what ``mgx_loudness`` decides before it touches a handle.
"""

import ctypes
import importlib.util
import math
import os
import subprocess

import numpy as np
import pytest

import emu_build
import loudness_cases as cases
import loudness_oracle as oracle
from conftest import ROOT
from matchering_amd import _native

P = ctypes.c_void_p


@pytest.fixture(scope="module")
def emu():
    lib = emu_build.load("loudness")
    lib.emu_loudness.restype = ctypes.c_longlong
    lib.emu_loudness.argtypes = [P, ctypes.c_longlong, ctypes.c_int, P, P, P]
    lib.emu_loudness_geometry.argtypes = [ctypes.c_int, ctypes.c_longlong, P]
    lib.emu_loudness_gate.argtypes = [P, ctypes.c_longlong, ctypes.c_int, P]
    return lib


def plan(emu, rate):
    c, a, b, table, misc = np.zeros(10), np.zeros(16), np.zeros(4), np.zeros(36 + 8 * 16), np.zeros(3)
    assert emu.emu_loudness_plan(rate, *[v.ctypes.data_as(P) for v in (c, a, b, table, misc)]) == table.size
    return c, a.reshape(4, 4), b, table, misc[0], int(misc[1]), int(misc[2])


def emu_geometry(emu, rate, n):
    out = (ctypes.c_longlong * 5)()
    emu.emu_loudness_geometry(rate, n, out)
    return tuple(out)


def gate_report(energy, rate):
    """mgx_loudness_gate of the real library on sub-block energies."""
    lib = _native.library()
    energy = np.ascontiguousarray(energy, dtype=np.float64).reshape(-1, 2)
    report = _native.MgxLoudnessReport()
    report.true_peak = report.sample_peak = -7.0
    rc = lib.mgx_loudness_gate(energy.ctypes.data_as(_native.c_double_p), energy.shape[0], rate, ctypes.byref(report))
    assert rc == 0, lib.mgx_last_error()
    assert report.sub_blocks == energy.shape[0] and report.sub_block_frames == oracle.sub_block_frames(rate)
    assert report.true_peak == report.sample_peak == -7.0                # the peaks are not this call's
    return report.integrated, report.range, report.momentary_max, report.short_term_max


def emulated(emu, x, rate):
    """(sub-block energies, the four gated fields, true peak, sample peak, input word) of the kernel's phases on the CPU
    followed by the library's own gating."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.shape[0]
    _, nsub, _, _, workgroups = emu_geometry(emu, rate, n)
    energy, peaks, word = np.full((nsub, 2), np.nan), np.full((workgroups, 2), np.nan), ctypes.c_int(0)
    assert emu.emu_loudness(x.ctypes.data_as(P), n, rate, energy.ctypes.data_as(P), peaks.ctypes.data_as(P),
                            ctypes.byref(word)) == workgroups
    assert not np.isnan(peaks).any()                                     # every workgroup wrote its two maxima
    return energy, gate_report(energy, rate), float(peaks[:, 0].max()), float(peaks[:, 1].max()), word.value


def check(emu, x, rate, label):
    energy, fields, true_peak, sample_peak, word = emulated(emu, x, rate)
    assert word == 0
    return cases.assert_measured(x, rate, energy, fields, true_peak, sample_peak, label)


# ---- the plan ------------------------------------------------------------------------------------------------------

def test_coefficients_are_the_published_tables_at_48_khz(emu):
    c, *_ = plan(emu, 48000)
    table = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
             1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]
    assert np.abs(c - table).max() < 5e-14
    for rate in cases.RATES:
        shelf, high = oracle.k_weighting(rate)
        got = plan(emu, rate)[0]
        assert np.abs(got - np.concatenate([shelf[0], shelf[1][1:], high[0], high[1][1:]])).max() < 1e-15


def test_warmup_and_geometry(emu):
    """ceil(ln 1e-12 / ln rho) is 5089 frames at 44.1 kHz and 22156 at 192 kHz, but the high-pass's near-double pole
    leaves ||A^k|| far above rho^k there (> 1e-11): the warm-up is the first k from there on at which the norm of A^k
    itself (largest row sum) is down to 1e-12, a third longer."""
    assert plan(emu, 44100)[6] == 5089 and plan(emu, 192000)[6] == 22156
    for rate in cases.RATES + (76050,):
        _, a, _, _, rho, warmup, poles = plan(emu, rate)
        assert poles == cases.warmup_poles(rate) and rho ** poles <= 1e-12 < rho ** (poles - 1)
        assert warmup == cases.warmup(rate) and poles < warmup < 1.5 * poles
        assert np.abs(a - cases.state_matrix(rate).astype(np.float64)).max() < 1e-15
        wide = a.astype(np.longdouble)
        norm = lambda k: float(np.abs(np.linalg.matrix_power(wide, k)).sum(axis=1).max())       # noqa: E731
        assert norm(warmup) <= 1e-12 < norm(warmup - 1) and norm(poles) > 1e-11
        size = oracle.sub_block_frames(rate)
        for n in cases.lengths(rate) + [0, 401 * size, 4801 * size + 5, 12 * 400 * size]:
            assert emu_geometry(emu, rate, n) == cases.geometry(rate, n), (rate, n)
    assert emu_geometry(emu, 44100, 44100 * 480)[3:] == (12, 400)        # the 8-minute track: 400 workgroups of 12
    assert oracle.sub_block_frames(11025) == 1103                        # 100 ms is not a whole number of frames


def test_state_matrices_are_the_recursion(emu):
    """z' = A z + B x reproduces lfilter's cascade frame by frame, and the table holds A^16, A^32, ... A^2048."""
    for rate in (8000, 44100, 192000):
        c, a, b, table, *_ = plan(emu, rate)
        shelf, high = oracle.k_weighting(rate)
        x = np.random.RandomState(rate).randn(40)
        from scipy.signal import lfilter, lfiltic                       # noqa: F401
        y = lfilter(high[0], high[1], lfilter(shelf[0], shelf[1], x))
        z, out = np.zeros(4), []
        for v in x:
            out.append(high[0][0] * (shelf[0][0] * v + z[0]) + z[2])      # y2 = c0 (b0 x + s1) + t1
            z = a @ z + b * v
        assert np.abs(np.array(out) - y).max() < 1e-13
        power = np.linalg.matrix_power(a.astype(np.longdouble), 16)
        for k in range(8):
            got = table[36 + 16 * k:36 + 16 * (k + 1)].reshape(4, 4)
            assert np.abs(got - power.astype(np.float64)).max() <= 1e-13 * max(1.0, float(np.abs(power).max())), (rate, k)
            power = power @ power


def test_true_peak_taps(emu):
    taps = np.zeros(49)
    emu.emu_loudness_taps(taps.ctypes.data_as(P))
    assert np.abs(taps - oracle.true_peak_taps()).max() < 1e-15
    table = plan(emu, 48000)[3]
    want = oracle.true_peak_taps()
    for phase in (1, 2, 3):
        for i in range(12):
            assert table[(phase - 1) * 12 + i] == taps[24 + phase + 4 * (i - 6)]
    assert abs(want[24] - 1.0) < 1e-15 and np.abs(want[24 + 4::4]).max() < 1e-15      # phase 0 is the track itself


# ---- the kernel's phases against the oracle -------------------------------------------------------------------------

@pytest.mark.parametrize("rate", cases.RATES)
def test_emulated_kernel_at_every_rate_and_length(emu, rate):
    for n in cases.lengths(rate):
        check(emu, cases.noise(n, rate % 1000 + n % 97, dc=0.05), rate, f"{rate} Hz, {n} frames")


@pytest.mark.parametrize("rate,subs", [(44100, 1), (44100, 2), (44100, 3), (44100, 50), (8000, 401), (8000, 801),
                                        (8000, 4801), (8000, 4813)])
def test_emulated_kernel_workgroup_counts(emu, rate, subs):
    """One workgroup, two, two and one sub-block more, about fifty; then tracks long enough for two, three and twelve
    sub-blocks per workgroup (12 x 400 + 1 sub-blocks: the last workgroup owns one; + 13: two workgroups more)."""
    size = oracle.sub_block_frames(rate)
    n = subs * size + 7
    _, _, _, own, workgroups = cases.geometry(rate, n)
    assert (own, workgroups) == {1: (1, 1), 2: (1, 2), 3: (1, 3), 50: (1, 50), 401: (2, 201), 801: (3, 267),
                                 4801: (12, 401), 4813: (12, 402)}[subs]
    check(emu, cases.noise(n, subs, dc=-0.1), rate, f"{rate} Hz, {subs} sub-blocks in {workgroups} workgroups of {own}")


def test_second_workgroup_with_a_clipped_warmup(emu):
    """Two sub-blocks at 192 kHz: the second workgroup's warm-up (22156 frames) is longer than the sub-block before it."""
    assert cases.warmup(192000) > 19200 and cases.geometry(192000, 2 * 19200 + 1)[3:] == (1, 2)
    assert cases.workgroup_start(192000, 2 * 19200 + 1, 1) == 0
    check(emu, cases.noise(2 * 19200 + 1, 5, dc=0.2), 192000, "clipped warm-up")


@pytest.mark.parametrize("rate", [44100, 192000])
def test_emulated_noise_dc_and_a_60_db_step(emu, rate):
    """The step on an ownership boundary, and on a tile boundary of the workgroup that owns what follows."""
    size = oracle.sub_block_frames(rate)
    n = 40 * size + 11
    on_ownership = 17 * size
    check(emu, cases.noise_dc_step(rate, n, on_ownership), rate, f"{rate} Hz, step on an ownership boundary")
    on_tile = cases.workgroup_start(rate, n, 20) + 2 * cases.TILE
    assert (on_tile - cases.workgroup_start(rate, n, 20)) % cases.TILE == 0 and on_tile < 21 * size
    check(emu, cases.noise_dc_step(rate, n, on_tile), rate, f"{rate} Hz, step on a tile boundary")


@pytest.mark.parametrize("rate", [44100, 48000, 76050, 192000])
def test_emulated_step_ahead_of_a_warmup_with_nothing_to_spare(emu, rate):
    """A track length at which the last workgroup's tiles begin exactly H frames ahead of its sub-blocks (at 76050 Hz
    every workgroup's do), and the 60 dB step at 0.1 to 0.4 sub-blocks ahead of them -- the
    transient of the step has died down, the state the workgroup never saw is 60 dB above what it measures: here H
    alone has to hold the bound."""
    n, begin = cases.zero_slack_length(rate, 40)
    size = oracle.sub_block_frames(rate)
    for back in (size * k // 20 for k in (2, 3, 4, 5, 6, 8)):
        check(emu, cases.noise_dc_step(rate, n, begin - back), rate, f"{rate} Hz, {n} frames, step {back} frames ahead of {begin}")


def test_emulated_impulses(emu):
    """Full-scale impulses at frame 0, at the last frame, and either side of an ownership boundary: the true peak's
    apron across every edge, with zeros beyond the track."""
    rate, size = 44100, 4410
    n = 6 * size + 100
    for at in ([0], [n - 1], [3 * size - 1], [3 * size], [0, n - 1, 3 * size - 1, 3 * size]):
        want = check(emu, cases.impulses(n, at), rate, f"impulses at {at}")
        assert want.true_peak == 1.0 == want.sample_peak
    # an impulse between two samples of the oversampled grid: two half-scale neighbours peak above both
    x = np.zeros((n, 2), dtype=np.float32)
    x[3 * size - 1, 0] = x[3 * size, 0] = 0.5
    want = check(emu, x, rate, "a pair across the boundary")
    assert want.true_peak > 0.6 and want.sample_peak == 0.5


def test_emulated_silence_and_non_finite_input(emu):
    energy, fields, true_peak, sample_peak, word = emulated(emu, np.zeros((5 * 4410, 2), dtype=np.float32), 44100)
    assert word == 0 and not energy.any() and true_peak == 0.0 == sample_peak
    assert fields[0] == fields[2] == fields[3] == -math.inf and fields[1] == 0.0
    x = cases.noise(5 * 4410 + 300, 1)
    for at, value in ((0, np.nan), (5 * 4410 + 299, np.inf), (2 * 4410 + 17, -np.inf)):
        bad = x.copy()
        bad[at, 1] = value
        assert emulated(emu, bad, 44100)[4] == 1, at


def test_emulated_kernel_is_reproducible(emu):
    x = cases.noise(9 * 4410 + 3, 8)
    first, second = emulated(emu, x, 44100), emulated(emu, x, 44100)
    assert np.array_equal(first[0], second[0]) and first[1:] == second[1:]


# ---- the gating through the real library ----------------------------------------------------------------------------

def test_gate_equals_the_oracle():
    rng = np.random.RandomState(21)
    for rate, subs in ((44100, 0), (44100, 3), (44100, 4), (44100, 29), (44100, 30), (48000, 217), (11025, 640)):
        levels = 10.0 ** (rng.uniform(-9.0, -1.0, size=(subs, 1)) + rng.uniform(-0.2, 0.2, size=(subs, 2)))
        energy = levels * oracle.sub_block_frames(rate)
        assert oracle.gate_margin(energy, rate) > 1e-6
        got, want = gate_report(energy, rate), oracle.gate(energy, rate)
        for g, w in zip(got, want):
            assert (g == w) if math.isinf(w) else abs(g - w) <= 1e-12, (rate, subs, got, want)
    # NaN energies never give NaN loudness
    assert gate_report(np.full((40, 2), np.nan), 44100) == (-math.inf, 0.0, -math.inf, -math.inf)


# ---- known answers, independent of the oracle ------------------------------------------------------------------------

@pytest.mark.parametrize("rate", [44100, 48000])
@pytest.mark.parametrize("name,parts,field,required,below,above", cases.KNOWN, ids=[k[0] for k in cases.KNOWN])
def test_ebu_known_answers(emu, rate, name, parts, field, required, below, above):
    """EBU Tech 3341 (integrated, +-0.1 LU) and Tech 3342 (range, +-1 LU) on 1 kHz stereo sines: the kernel's phases and
    the library's gating, and the oracle on its own."""
    x = cases.segments(rate, parts)
    energy, fields, _, _, word = emulated(emu, x, rate)
    got = dict(zip(("integrated", "range", "momentary_max", "short_term_max"), fields))[field]
    oracle_says = dict(zip(("integrated", "range"), oracle.gate(oracle.sub_energies(x, rate), rate)[:2]))[field]
    print(f"{name} at {rate} Hz: {field} {got:.3f} (oracle {oracle_says:.3f}), required {required} -{below} +{above}")
    assert word == 0
    assert required - below <= got <= required + above
    assert required - below <= oracle_says <= required + above


@pytest.mark.parametrize("fraction,degrees,amplitude,required,below,above", cases.TRUE_PEAKS)
def test_true_peak_known_answers(emu, fraction, degrees, amplitude, required, below, above):
    rate = 48000
    x = cases.faded_sine(rate, fraction * rate, degrees, amplitude)
    _, _, true_peak, sample_peak, _ = emulated(emu, x, rate)
    got, want = 20.0 * math.log10(true_peak), 20.0 * math.log10(oracle.peaks(x)[0])
    print(f"fs x {fraction:.3f} at {degrees} degrees, amplitude {amplitude}: {got:.3f} dBTP (oracle {want:.3f}), "
          f"sample peak {20.0 * math.log10(sample_peak):.2f} dB")
    assert required - below <= got <= required + above
    assert required - below <= want <= required + above
    if (fraction, degrees, amplitude) == (1 / 4, 45.0, 0.5):
        assert abs(20.0 * math.log10(sample_peak) + 9.03) < 0.01          # what a sample-peak meter reads: 3 dB short


def test_oracle_stays_on_nominal_up_to_192_khz():
    for rate in (96000, 192000):
        x = cases.segments(rate, [(20, -23)])
        assert abs(oracle.gate(oracle.sub_energies(x, rate), rate)[0] + 23.0) <= 0.05


# ---- the C ABI without a device ---------------------------------------------------------------------------------------

def test_mgx_loudness_decides_before_it_touches_the_handle():
    lib = _native.library()
    assert lib.mgx_version() >= 104
    report, count = _native.MgxLoudnessReport(), ctypes.c_int64(-7)
    somewhere = ctypes.c_void_p(4096)

    def call(n, rate, rep=report, energy=None, capacity=0, handle=None):
        return lib.mgx_loudness(handle, somewhere, n, rate, ctypes.byref(rep) if rep is not None else None, energy,
                                capacity, ctypes.byref(count))

    assert call(1000, 7999) == _native.ERR_ARGUMENT and b"8000" in lib.mgx_last_error()
    assert call(1000, 0) == _native.ERR_ARGUMENT and call(1000, -44100) == _native.ERR_ARGUMENT
    assert call(1000, 44100, rep=None) == _native.ERR_ARGUMENT
    assert call(-1, 44100) == _native.ERR_ARGUMENT
    assert count.value == -7                                              # nothing reported so far
    energy = (ctypes.c_double * 8)()
    assert call(5 * 4410, 44100, energy=energy, capacity=4) == _native.ERR_ARGUMENT and count.value == 5
    assert b"fewer" in lib.mgx_last_error()
    assert call(5 * 4410, 44100) == _native.ERR_ARGUMENT                  # a null handle
    assert lib.mgx_loudness_gate(None, 3, 44100, ctypes.byref(report)) == _native.ERR_ARGUMENT
    assert lib.mgx_loudness_gate(energy, 4, 44100, None) == _native.ERR_ARGUMENT
    assert lib.mgx_loudness_gate(energy, 4, 4000, ctypes.byref(report)) == _native.ERR_ARGUMENT
    assert lib.mgx_loudness_gate(None, 0, 44100, ctypes.byref(report)) == 0 and report.integrated == -math.inf


def test_report_layout_matches_the_c_compiler(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mgx.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(mgx_loudness_report),\n'
                   '  offsetof(mgx_loudness_report, true_peak), offsetof(mgx_loudness_report, sub_blocks),\n'
                   '  offsetof(mgx_loudness_report, sub_block_frames)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    c = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    r = _native.MgxLoudnessReport
    assert c == [ctypes.sizeof(r), r.true_peak.offset, r.sub_blocks.offset, r.sub_block_frames.offset]


def test_the_kernel_uses_no_scratch():
    spec = importlib.util.spec_from_file_location("code_object", os.path.join(ROOT, "tools", "code_object.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    _native.library()
    hits = [v for k, v in mod.kernels(_native.LIB_PATH).items() if "k_loudness" in k]
    assert len(hits) == 1 and hits[0]["scratch"] == 0


def test_the_python_surface():
    import inspect

    import matchering_amd as mg
    from matchering_amd import stages

    assert "loudness" in inspect.signature(mg.process).parameters and "loudness" in inspect.signature(stages.main).parameters
    value = mg.Loudness(-14.0, 5.0, -10.0, -12.0, 0.5, 0.25, 44100, 441000, 100, 4410)
    assert abs(value.true_peak_db + 6.0206) < 1e-3 and abs(value.sample_peak_db + 12.0412) < 1e-3
    assert "-14.00 LUFS" in str(value) and mg.Loudness(-math.inf, 0, -math.inf, -math.inf, 0, 0, 44100, 0, 0, 4410).true_peak_db == -math.inf
