"""Matching EQ controls on the GPU (include/mgx.h, mgx_eq_shape; csrc/eq_shape_kernels.h) against tests/eq_oracle.py.

Pairs of 2-3 s from matchering_amd.synth.make_pair, the generator of the golden cases.  The oracle of a size runs once
per module.  Sizes: 64 (the smallest the minimum-phase chain takes), 1024 (the largest at which a channel's transform is
one workgroup), 2048 (the smallest that is split), 4096 (the default; the cosine-sum tap synthesis) and 16384 (BASELINE
config #5; the transform tap synthesis, the factored curve route).  The minimum-phase chain also runs at 128 and 512,
whose transforms of 4 x 128 = 2^9 and 2^11 points have an odd log2 -- the single radix-2 stage in front of the radix-4
passes (minphase_sub_first), which no size with an even log2 reaches -- and at 8192, eight workgroups per transform.

Measured on an MI355X, minimum-phase taps against the oracle in parts of the peak tap (bound 2e-7), mid / side:
  64: 4.6e-8 / 4.2e-8, 128: 1.3e-8 / 1.2e-8, 512: 2.0e-8 / 2.6e-8, 1024: 3.3e-8 / 3.7e-9, 2048: 1.1e-8 / 8.6e-9,
  4096: 5.3e-9 / 2.2e-8, 8192: 4.1e-8 / 3.7e-9, 16384: 5.0e-9 / 2.6e-9.
"""

import ctypes

import numpy as np
import pytest

import eq_oracle
import mastering_oracle as mo
from conftest import rms_error

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-5                  # the project's bar, float32 against the float64 oracle
SECONDS = {64: 2.0, 128: 2.0, 512: 2.0, 1024: 2.0, 2048: 2.0, 4096: 2.5, 8192: 2.5, 16384: 3.0}
PAIR = {64: 40, 1024: 41, 2048: 42, 4096: 43, 16384: 44, 128: 45, 512: 46, 8192: 47}      # make_pair's seed of a size
HALF = dict(amount=0.5, max_boost_db=6.0, max_cut_db=6.0)


def config_of(fft):
    import matchering_amd as mg

    return mg.Config(fft_size=fft, max_piece_size=0.8)


def oracle_config(fft):
    return mo.params(fft_size=fft, max_piece_size=0.8)


@pytest.fixture(scope="module")
def pairs():
    from matchering_amd.synth import make_pair

    cache = {}

    def get(fft):
        if fft not in cache:
            cache[fft] = make_pair(SECONDS[fft], 44100, PAIR[fft], reference_seconds=SECONDS[fft] - 0.4)
        return cache[fft]

    return get


@pytest.fixture(scope="module")
def curves(pairs):
    """fft -> the oracle's trace of the pair (its smoothed curves are what every shape starts from)."""
    cache = {}

    def get(fft):
        if fft not in cache:
            trace = {}
            target, reference = pairs(fft)
            mo.master(target, reference, oracle_config(fft), False, True, False, trace=trace)
            cache[fft] = trace
        return cache[fft]

    return get


def eq_of(shape):
    import matchering_amd as mg

    return None if shape is None else mg.MatchingEq(**shape)


def run(dev, pair, fft, eq, outputs=(True, False, False), profile=None, report=False):
    """One master call: (the three renderings or None, the handle's taps [2][fft])."""
    target, reference = pair
    n = target.shape[0]
    with dev.lock:
        td = dev.upload(target)
        rd = None if profile is not None else dev.upload(reference)
        outs = [dev.alloc(n * 8) if want else None for want in outputs]
        try:
            route = {} if profile is None else {"profile": profile.resident(dev)}
            dev.master(td, n, rd, 0 if rd is None else reference.shape[0], config_of(fft).to_native(), *outs,
                       want_report=report, eq=eq, **route)
            ptr, taps = dev.last_fir()
            assert taps == fft
            fir = dev.download(ptr, (2, fft))
            got = [None if b is None else dev.download(b, (n, 2)) for b in outs]
        finally:
            for b in (td, rd, *outs):
                if b is not None:
                    b.release()
    return got, fir


@pytest.fixture(scope="module")
def dev():
    from matchering_amd.device import default_device

    return default_device()


# ---- (a) shaped linear-phase taps ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fft", [64, 4096, 16384])
def test_shaped_linear_taps(dev, pairs, curves, fft):
    """k_eq_shape in front of every tap synthesis: the handle's taps against the oracle's, <= 1e-6 of the peak tap
    (tests/test_gpu_parity.py's tolerance for taps)."""
    _, fir = run(dev, pairs(fft), fft, eq_of(HALF))
    trace = curves(fft)
    for mine, channel in zip(fir, ("mid", "side")):
        want = eq_oracle.shape_fir(trace[channel].smooth, 1e-6, **HALF)
        err = np.abs(mine - want).max() / np.abs(want).max()
        print(f"fft {fft} {channel}: shaped linear taps off by {err:.3g} of the peak")
        assert err <= 1e-6
        plain = eq_oracle.shape_fir(trace[channel].smooth, 1e-6)
        assert np.abs(want - plain).max() > 1e-3 * np.abs(plain).max()          # (the shape is not a no-op on this pair)


# ---- (b) the transform chain in isolation ------------------------------------------------------------------------------
@pytest.mark.parametrize("fft", [64, 128, 512, 1024, 2048, 4096, 8192, 16384])
def test_minimum_phase_chain(dev, pairs, fft):
    """The minimum-phase taps against eq_oracle's minimum phase of the SAME run's float32 linear taps: <= 2e-7 of the
    peak -- one float32 rounding, 6e-8, with margin for the float64 transforms."""
    pair = pairs(fft)
    _, lin = run(dev, pair, fft, eq_of(HALF))
    _, got = run(dev, pair, fft, eq_of(dict(HALF, phase="minimum")))
    for mine, linear, channel in zip(got, lin, ("mid", "side")):
        want = eq_oracle.minimum_phase(linear)
        err = np.abs(mine - want).max() / np.abs(want).max()
        print(f"fft {fft} {channel}: minimum-phase taps off by {err:.3g} of the peak")
        assert err <= 2e-7
        assert not mine[:fft // 2].any() and mine[fft // 2] != 0.0


# ---- (c) end to end ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def end_to_end_oracle(pairs, curves):
    cache = {}

    def get(name, shape):
        if name not in cache:
            target, reference = pairs(4096)
            trace = curves(4096)
            fir = tuple(eq_oracle.shape_fir(trace[ch].smooth, 1e-6, **shape) for ch in ("mid", "side"))
            cache[name] = mo.master(target, reference, oracle_config(4096), True, True, True, fir=fir)
        return cache[name]

    return get


SHAPES = {"half_capped": HALF, "minimum": dict(phase="minimum"), "half_capped_minimum": dict(HALF, phase="minimum")}


@pytest.mark.parametrize("route", ["pair", "profile"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_master_shaped_end_to_end(dev, pairs, end_to_end_oracle, name, route):
    """mgx_master_shaped's three renderings against oracle.master(fir = eq_oracle's taps): <= 1e-5 RMS, pair and profile route."""
    import matchering_amd as mg

    pair = pairs(4096)
    profile = mg.ReferenceProfile.analyze(pair[1], config_of(4096), device=dev) if route == "profile" else None
    got, _ = run(dev, pair, 4096, eq_of(SHAPES[name]), outputs=(True, True, True), profile=profile, report=True)
    for mine, want, rendering in zip(got, end_to_end_oracle(name, SHAPES[name]), ("result", "no_limiter", "normalized")):
        err = rms_error(mine, want)
        print(f"{name} {route} {rendering}: rms error {err:.3g}")
        assert err <= RMS_TOL
    plain, _ = run(dev, pair, 4096, None)
    assert rms_error(got[0], plain[0]) > 1e-3                                    # (the shape is heard)


# ---- (d) the null shape ------------------------------------------------------------------------------------------------
def test_null_shape_is_mgx_master(dev, pairs):
    """shape == NULL and MatchingEq() give mgx_master's bytes on the same handle, renderings and taps."""
    from matchering_amd._native import check, library

    pair = pairs(4096)
    plain, plain_fir = run(dev, pair, 4096, None, outputs=(True, True, True))
    default, default_fir = run(dev, pair, 4096, eq_of({}), outputs=(True, True, True))
    for a, b in zip(plain + [plain_fir], default + [default_fir]):
        assert np.array_equal(a, b)
    target, reference = pair
    n = target.shape[0]
    with dev.lock:
        td, rd, out = dev.upload(target), dev.upload(reference), dev.alloc(n * 8)
        try:
            check(library().mgx_master_shaped(dev.handle, ctypes.c_void_p(td.ptr), n, ctypes.c_void_p(rd.ptr), reference.shape[0],
                                              None, ctypes.byref(config_of(4096).to_native()), None, ctypes.c_void_p(out.ptr),
                                              None, None, None))
            assert np.array_equal(dev.download(out, (n, 2)), plain[0])
        finally:
            for b in (td, rd, out):
                b.release()


# ---- (e) pipelined calls -----------------------------------------------------------------------------------------------
def test_queued_calls_keep_their_own_shapes(dev, pairs):
    """Four calls queued without a wait, shapes A, B, A, none: each result is the one its shape gives alone."""
    pair = pairs(4096)
    target, reference = pair
    n = target.shape[0]
    shapes = [eq_of(HALF), eq_of(dict(phase="minimum")), eq_of(HALF), None]
    alone = [run(dev, pair, 4096, eq)[0][0] for eq in shapes[1:]]                # (B, A, none)
    with dev.lock:
        td, rd = dev.upload(target), dev.upload(reference)
        outs = [dev.alloc(n * 8) for _ in shapes]
        try:
            cfg = config_of(4096).to_native()
            for eq, out in zip(shapes, outs):
                dev.master(td, n, rd, reference.shape[0], cfg, result=out, want_report=False, eq=eq)
            dev.synchronize()
            got = [dev.download(b, (n, 2)) for b in outs]
        finally:
            for b in (td, rd, *outs):
                b.release()
    assert np.array_equal(got[0], alone[1]) and np.array_equal(got[1], alone[0])
    assert np.array_equal(got[2], alone[1]) and np.array_equal(got[3], alone[2])
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[0], got[3])


# ---- (f) refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fft", [32, 32768])
def test_refused_sizes_launch_nothing(dev, pairs, fft):
    """A minimum-phase EQ at a size outside [64, 16384]: MGX_ERR_UNSUPPORTED with the size named, before anything is
    queued -- the output buffer keeps its bytes and the handle's last FIR stays the previous call's."""
    import matchering_amd as mg
    from matchering_amd._native import ERR_UNSUPPORTED, MgxError

    target, reference = pairs(4096)
    n = target.shape[0]
    run(dev, (target, reference), 4096, None)
    cfg = mg.Config(fft_size=fft, max_piece_size=0.8)
    with dev.lock:
        marker = np.full((n, 2), 0.25, dtype=np.float32)
        td, rd, out = dev.upload(target), dev.upload(reference), dev.upload(marker)
        try:
            with pytest.raises(MgxError) as refusal:
                dev.master(td, n, rd, reference.shape[0], cfg.to_native(), result=out, want_report=False,
                           eq=mg.MatchingEq(phase="minimum"))
            assert refusal.value.code == ERR_UNSUPPORTED and str(fft) in str(refusal.value)
            dev.synchronize()
            assert np.array_equal(dev.download(out, (n, 2)), marker)
            assert dev.last_fir()[1] == 4096
        finally:
            for b in (td, rd, out):
                b.release()
