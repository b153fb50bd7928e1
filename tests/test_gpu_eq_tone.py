"""Matching EQ tone controls on the GPU (include/mgx.h, mgx_eq_tone; csrc/eq_tone_kernels.h) against
tests/eq_tone_oracle.py.

Pairs of 2-3 s from matchering_amd.synth.make_pair, as in tests/test_gpu_eq.py.  The oracle of a size runs once per
module.  Sizes: 64 taps (one partial workgroup of k_eq_tone per channel), 4096 at 44.1 kHz (the dense curve route, the
cosine-sum tap synthesis), 16384 at 96 kHz (the factored curve route, the transform tap synthesis) and, taps only, 32768
(the chain on the curve itself).

Measured on an MI355X, in parts of the peak tap: toned linear taps against the oracle (bound 1e-6) 3e-9 - 2.8e-8 at 64
taps, 1.4e-8 - 8.3e-8 at 4096, 9e-9 - 1.3e-7 at 16384, 3.6e-8 at 32768; minimum-phase toned taps against the oracle's
minimum phase of the same run's linear taps (bound 2e-7) 3e-9 - 2.9e-8; the renderings 7.7e-8 - 1.6e-7 RMS (bound 1e-5);
the 50 Hz side component under mono bass: the oracle drops it by 50.29 dB, the device by 50.29 dB.
"""

import ctypes

import numpy as np
import pytest

import eq_oracle
import eq_tone_oracle as tone_oracle
import mastering_oracle as mo
from conftest import rms_error
from eq_tone_emu import shape_struct, tone_struct

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-5                  # the project's bar, float32 against the float64 oracle
RATE = {64: 44100, 4096: 44100, 16384: 96000, 32768: 44100}
SECONDS = {64: 2.0, 4096: 2.5, 16384: 3.0, 32768: 3.0}
PAIR = {64: 50, 4096: 51, 16384: 52, 32768: 53}             # make_pair's seed of a size
PIECE = {64: 0.8, 4096: 0.8, 16384: 0.8, 32768: 1.0}        # max_piece_size, seconds: no piece shorter than fft_size
SHAPE = dict(amount=0.8, max_boost_db=9.0, max_cut_db=7.0)


def config_of(fft):
    import matchering_amd as mg

    return mg.Config(fft_size=fft, max_piece_size=PIECE[fft], internal_sample_rate=RATE[fft])


def oracle_config(fft):
    return mo.params(fft_size=fft, max_piece_size=PIECE[fft], internal_sample_rate=RATE[fft])


def bands_of(fs):
    import matchering_amd as mg

    r = fs / 44100.0
    return (mg.ToneBand("high_shelf", 9000.0 * r, 1.0), mg.ToneBand("bell", 300.0 * r, -2.5, q=1.4, channels="mid"),
            mg.ToneBand("low_shelf", 180.0 * r, 3.0, q=0.5, channels="side"))


def tones(fs):
    """name -> the MatchingEq keywords of a tone: each control alone and all together, valid at every rate used here."""
    r = fs / 44100.0
    return {
        "range": dict(match_range=(60.0 * r, 12000.0 * r)),
        "side_amount": dict(side_amount=0.0),
        "mono": dict(mono_below_hz=120.0 * r),
        "tilt": dict(tilt_db_per_octave=-0.5),
        "bands": dict(bands=bands_of(fs)),
        "all": dict(match_range=(60.0 * r, 12000.0 * r), range_octaves=0.5, side_amount=0.3, mono_below_hz=120.0 * r,
                    mono_octaves=1.5, tilt_db_per_octave=0.75, tilt_pivot_hz=700.0 * r, bands=bands_of(fs)),
    }


def oracle_tone(eq):
    """The oracle's dict of a MatchingEq's tone."""
    from matchering_amd.eq import BAND_CHANNELS, BAND_KINDS

    low, high = eq.match_range or (None, None)
    return tone_oracle.tone_of(low_hz=low, high_hz=high, range_octaves=eq.range_octaves, side_amount=eq.side_amount,
                               mono_below_hz=eq.mono_below_hz, mono_octaves=eq.mono_octaves,
                               tilt_db_per_octave=eq.tilt_db_per_octave, tilt_pivot_hz=eq.tilt_pivot_hz,
                               bands=tuple((BAND_KINDS[b.kind], BAND_CHANNELS[b.channels], b.hz, b.gain_db, b.q) for b in eq.bands))


def oracle_taps(trace, fft, eq, float32_linear=False):
    """(mid, side) taps of the oracle under ``eq`` from the pair's smoothed curves."""
    shape = dict(amount=eq.amount, max_boost_db=eq.max_boost_db, max_cut_db=eq.max_cut_db, phase=eq.phase)
    return tuple(tone_oracle.tone_fir(trace[ch].smooth, 1e-6, RATE[fft], c, oracle_tone(eq), float32_linear=float32_linear, **shape)
                 for c, ch in enumerate(("mid", "side")))


@pytest.fixture(scope="module")
def pairs():
    from matchering_amd.synth import make_pair

    cache = {}

    def get(fft):
        if fft not in cache:
            pair = make_pair(SECONDS[fft], RATE[fft], PAIR[fft], reference_seconds=SECONDS[fft] - 0.4)
            for track in pair:
                track.setflags(write=False)
            cache[fft] = pair
        return cache[fft]

    return get


@pytest.fixture(scope="module")
def curves(pairs):
    """fft -> the oracle's trace of the pair (its smoothed curves are what every tone starts from)."""
    cache = {}

    def get(fft):
        if fft not in cache:
            trace = {}
            target, reference = pairs(fft)
            mo.master(target, reference, oracle_config(fft), False, True, False, trace=trace)
            cache[fft] = trace
        return cache[fft]

    return get


@pytest.fixture(scope="module")
def dev():
    from matchering_amd.device import default_device

    return default_device()


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


def profile_of(dev, pair, fft, route):
    import matchering_amd as mg

    return mg.ReferenceProfile.analyze(pair[1], config_of(fft), device=dev) if route == "profile" else None


# ---- (a) toned linear-phase taps ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["pair", "profile"])
@pytest.mark.parametrize("fft", [64, 4096, 16384])
def test_toned_linear_taps(dev, pairs, curves, fft, route):
    """k_eq_tone in front of every tap synthesis, behind the dense and the factored curve route, from a pair and from a
    profile: the handle's taps against the oracle's, <= 1e-6 of the peak tap, each control alone and all together."""
    import matchering_amd as mg

    pair, trace = pairs(fft), curves(fft)
    profile = profile_of(dev, pair, fft, route)
    plain = oracle_taps(trace, fft, mg.MatchingEq(**SHAPE))
    for name, tone in tones(RATE[fft]).items():
        eq = mg.MatchingEq(**SHAPE, **tone)
        _, fir = run(dev, pair, fft, eq, profile=profile)
        for mine, want, base, channel in zip(fir, oracle_taps(trace, fft, eq), plain, ("mid", "side")):
            err = np.abs(mine - want).max() / np.abs(want).max()
            print(f"fft {fft} {route} {name} {channel}: toned linear taps off by {err:.3g} of the peak")
            assert err <= 1e-6
        # (the tone is not a no-op on this pair -- but for mono bass at 64 taps, whose first bin lies at 689 Hz)
        if (fft, name) != (64, "mono"):
            assert any(np.abs(w - b).max() > 1e-3 * np.abs(b).max() for w, b in zip(oracle_taps(trace, fft, eq), plain))


def test_toned_linear_taps_at_32768(dev, pairs, curves):
    """32768 taps, where the curve chain runs on the curve itself: linear phase, taps only."""
    import matchering_amd as mg

    eq = mg.MatchingEq(**SHAPE, **tones(RATE[32768])["all"])
    _, fir = run(dev, pairs(32768), 32768, eq)
    for mine, want, channel in zip(fir, oracle_taps(curves(32768), 32768, eq), ("mid", "side")):
        err = np.abs(mine - want).max() / np.abs(want).max()
        print(f"fft 32768 all {channel}: toned linear taps off by {err:.3g} of the peak")
        assert err <= 1e-6


# ---- (b) minimum phase with a tone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fft", [64, 4096, 16384])
def test_minimum_phase_with_a_tone(dev, pairs, fft):
    """The minimum-phase chain on toned taps -- with mono bass a side response with zeros -- against eq_oracle's minimum
    phase of the SAME run's float32 linear taps: <= 2e-7 of the peak."""
    import matchering_amd as mg

    pair = pairs(fft)
    for name in ("mono", "all"):
        tone = tones(RATE[fft])[name]
        _, lin = run(dev, pair, fft, mg.MatchingEq(**SHAPE, **tone))
        _, got = run(dev, pair, fft, mg.MatchingEq(**SHAPE, phase="minimum", **tone))
        for mine, linear, channel in zip(got, lin, ("mid", "side")):
            want = eq_oracle.minimum_phase(linear)
            err = np.abs(mine - want).max() / np.abs(want).max()
            print(f"fft {fft} {name} {channel}: minimum-phase toned taps off by {err:.3g} of the peak")
            assert err <= 2e-7
            assert not mine[:fft // 2].any() and mine[fft // 2] != 0.0


# ---- (c) the three renderings end to end --------------------------------------------------------------------------------
def renderings():
    import matchering_amd as mg

    return {"range_image_kept": mg.MatchingEq(match_range=(60.0, 12000.0), side_amount=0.0),
            "mono_bass": mg.MatchingEq(mono_below_hz=120.0),
            "air_and_tilt": mg.MatchingEq(tilt_db_per_octave=-0.3, bands=(mg.ToneBand("high_shelf", 10000.0, 1.0),))}


@pytest.fixture(scope="module")
def end_to_end_oracle(pairs, curves):
    cache = {}

    def get(name):
        if name not in cache:
            target, reference = pairs(4096)
            fir = oracle_taps(curves(4096), 4096, renderings()[name])
            cache[name] = mo.master(target, reference, oracle_config(4096), True, True, True, fir=fir)
        return cache[name]

    return get


@pytest.mark.parametrize("route", ["pair", "profile"])
@pytest.mark.parametrize("name", ["range_image_kept", "mono_bass", "air_and_tilt"])
def test_master_eq_end_to_end(dev, pairs, end_to_end_oracle, name, route):
    """mgx_master_eq's three renderings against oracle.master(fir = the oracle's toned taps): <= 1e-5 RMS, both routes."""
    pair = pairs(4096)
    got, fir = run(dev, pair, 4096, renderings()[name], outputs=(True, True, True), profile=profile_of(dev, pair, 4096, route),
                   report=True)
    for mine, want, rendering in zip(got, end_to_end_oracle(name), ("result", "no_limiter", "normalized")):
        err = rms_error(mine, want)
        print(f"{name} {route} {rendering}: rms error {err:.3g}")
        assert err <= RMS_TOL
    _, plain_fir = run(dev, pair, 4096, None)
    assert np.abs(fir - plain_fir).max() > 1e-3 * np.abs(plain_fir).max()        # (the tone is in the taps)


# ---- (d) identities ------------------------------------------------------------------------------------------------------
def call_library(dev, entry, pair, fft, *eq_args):
    """mgx_master / mgx_master_shaped / mgx_master_eq by name with the structs given: (three renderings, taps)."""
    from matchering_amd._native import check, library

    target, reference = pair
    n = target.shape[0]
    with dev.lock:
        td, rd = dev.upload(target), dev.upload(reference)
        outs = [dev.alloc(n * 8) for _ in range(3)]
        try:
            head = (dev.handle, ctypes.c_void_p(td.ptr), n, ctypes.c_void_p(rd.ptr), reference.shape[0])
            route = () if entry == "mgx_master" else (None,)
            tail = tuple(ctypes.c_void_p(b.ptr) for b in outs) + (None,)
            check(getattr(library(), entry)(*head, *route, ctypes.byref(config_of(fft).to_native()),
                                            *(None if a is None else ctypes.byref(a) for a in eq_args), *tail))
            ptr, taps = dev.last_fir()
            return [dev.download(b, (n, 2)) for b in outs] + [dev.download(ptr, (2, taps))]
        finally:
            for b in (td, rd, *outs):
                b.release()


def test_neutral_and_null_tone_are_mgx_master_shaped(dev, pairs):
    """A neutral tone and a null tone are byte for byte mgx_master_shaped on the same handle, renderings and taps; a null
    shape with a neutral tone is byte for byte mgx_master."""
    pair = pairs(4096)
    neutral = tone_struct(tone_oracle.tone_of(range_octaves=2.5, mono_octaves=0.0, tilt_pivot_hz=300.0))
    for shape in (shape_struct(**SHAPE), shape_struct(phase="minimum"), shape_struct()):
        want = call_library(dev, "mgx_master_shaped", pair, 4096, shape)
        for tone in (None, neutral):
            for a, b in zip(call_library(dev, "mgx_master_eq", pair, 4096, shape, tone), want):
                assert np.array_equal(a, b)
    plain = call_library(dev, "mgx_master", pair, 4096)
    for tone in (None, neutral):
        for a, b in zip(call_library(dev, "mgx_master_eq", pair, 4096, None, tone), plain):
            assert np.array_equal(a, b)
    # ... and a null shape with a tone is amount 1, no caps, linear phase
    tilt = tone_struct(tone_oracle.tone_of(tilt_db_per_octave=1.0))
    for a, b in zip(call_library(dev, "mgx_master_eq", pair, 4096, None, tilt),
                    call_library(dev, "mgx_master_eq", pair, 4096, shape_struct(), tilt)):
        assert np.array_equal(a, b)
    assert not np.array_equal(call_library(dev, "mgx_master_eq", pair, 4096, None, tilt)[3], plain[3])


# ---- (e) mono bass seen in the audio -------------------------------------------------------------------------------------
def test_mono_bass_in_the_audio(dev, pairs, curves):
    """The target carries a 50 Hz sine in the left channel only; mono_below_hz = 120 at F = 4096 takes it out of the
    result's side channel (L - R) / 2.  The drop of the 50 Hz component against the same master without the control is the
    oracle's to within 3 dB (float32 frames, the level rounds)."""
    import matchering_amd as mg

    target, reference = pairs(4096)
    t = np.arange(target.shape[0]) / 44100.0
    target = np.array(target)
    target[:, 0] = np.clip(target[:, 0] + 0.1 * np.sin(2 * np.pi * 50.0 * t), -1.0, 1.0).astype(np.float32)
    probe = np.hanning(t.shape[0]) * np.exp(-2j * np.pi * 50.0 * t)

    def side_50(audio):
        audio = np.asarray(audio, dtype=np.float64)
        return abs(np.dot(probe, 0.5 * (audio[:, 0] - audio[:, 1])))

    eq = mg.MatchingEq(mono_below_hz=120.0)
    trace = {}
    ocfg = oracle_config(4096)
    without = mo.master(target, reference, ocfg, True, False, False, trace=trace)[0]
    fir = tuple(tone_oracle.tone_fir(trace[ch].smooth, 1e-6, 44100, c, oracle_tone(eq)) for c, ch in enumerate(("mid", "side")))
    with_control = mo.master(target, reference, ocfg, True, False, False, fir=fir)[0]
    expected = 20.0 * np.log10(side_50(without) / side_50(with_control))
    got_without, _ = run(dev, (target, reference), 4096, None)
    got_with, _ = run(dev, (target, reference), 4096, eq)
    drop = 20.0 * np.log10(side_50(got_without[0]) / side_50(got_with[0]))
    print(f"50 Hz in the side channel: the oracle drops it by {expected:.2f} dB, the device by {drop:.2f} dB")
    assert expected > 40.0                                                         # (there is something to see)
    assert abs(drop - expected) <= 3.0


# ---- (f) queued calls ----------------------------------------------------------------------------------------------------
def test_queued_calls_keep_their_own_tones(dev, pairs):
    """Four calls queued without a wait, tones A, B, neutral, C: each result is the one its tone gives alone."""
    import matchering_amd as mg

    pair = pairs(4096)
    target, reference = pair
    n = target.shape[0]
    all_tones = tones(44100)
    eqs = [mg.MatchingEq(**SHAPE, **all_tones["range"]), mg.MatchingEq(phase="minimum", **all_tones["mono"]),
           mg.MatchingEq(**SHAPE), mg.MatchingEq(**SHAPE, **all_tones["all"])]
    alone = [run(dev, pair, 4096, eq)[0][0] for eq in eqs]
    with dev.lock:
        td, rd = dev.upload(target), dev.upload(reference)
        outs = [dev.alloc(n * 8) for _ in eqs]
        try:
            cfg = config_of(4096).to_native()
            for eq, out in zip(eqs, outs):
                dev.master(td, n, rd, reference.shape[0], cfg, result=out, want_report=False, eq=eq)
            dev.synchronize()
            got = [dev.download(b, (n, 2)) for b in outs]
        finally:
            for b in (td, rd, *outs):
                b.release()
    for k, (mine, want) in enumerate(zip(got, alone)):
        assert np.array_equal(mine, want), f"call {k} did not get its own tone"
    assert all(not np.array_equal(got[i], got[j]) for i in range(4) for j in range(i))


# ---- (g) refusals --------------------------------------------------------------------------------------------------------
def test_refused_calls_launch_nothing(dev, pairs):
    """A field out of range, or minimum phase with a tone at 32768 taps: refused by name before anything is queued -- the
    output buffer keeps its bytes and the handle's last FIR stays the previous call's."""
    import matchering_amd as mg
    from matchering_amd._native import ERR_ARGUMENT, ERR_UNSUPPORTED, MgxError

    target, reference = pairs(4096)
    n = target.shape[0]
    _, before = run(dev, (target, reference), 4096, None)
    tilt = mg.MatchingEq(phase="minimum", tilt_db_per_octave=1.0)
    cases = [(config_of(4096), mg.MatchingEq(mono_below_hz=30000.0), ERR_ARGUMENT, "mono_below_hz"),
             (config_of(4096), mg.MatchingEq(bands=(mg.ToneBand("bell", 100.0, 1.0), mg.ToneBand("bell", 23000.0, 1.0))),
              ERR_ARGUMENT, "bands[1].hz"),
             (config_of(32768), tilt, ERR_UNSUPPORTED, "32768")]
    with dev.lock:
        marker = np.full((n, 2), 0.25, dtype=np.float32)
        td, rd, out = dev.upload(target), dev.upload(reference), dev.upload(marker)
        try:
            for cfg, eq, code, word in cases:
                with pytest.raises(MgxError) as refusal:
                    dev.master(td, n, rd, reference.shape[0], cfg.to_native(), result=out, want_report=False, eq=eq)
                assert refusal.value.code == code and word in str(refusal.value)
                dev.synchronize()
                assert np.array_equal(dev.download(out, (n, 2)), marker)
                ptr, taps = dev.last_fir()
                assert taps == 4096 and np.array_equal(dev.download(ptr, (2, 4096)), before)
        finally:
            for b in (td, rd, out):
                b.release()


# ---- (h) album mode -------------------------------------------------------------------------------------------------------
def test_album_mode_tones_the_one_fir_once(pairs):
    """master_album(eq = toned) on one rank: track 0 designs the toned FIR; track 1 is given it -- its taps are the first's,
    toned once, not toned again and not its own."""
    import matchering_amd as mg
    from matchering_amd import batch, stages
    from matchering_amd.synth import make_pair

    target, reference = pairs(4096)
    second, _ = make_pair(2.5, 44100, 58, reference_seconds=2.1)
    cfg = config_of(4096)
    eq = mg.MatchingEq(**SHAPE, **tones(44100)["all"])
    dev = batch.lane_device(0, 0)                                # the handle master_album works on: its last FIR is track 1's
    _, first_taps = run(dev, (target, reference), 4096, eq)
    album = batch.master_album([target, second], reference, cfg, rank=0, world_size=1, device_index=0, eq=eq)
    ptr, taps = dev.last_fir()
    assert taps == 4096 and np.array_equal(dev.download(ptr, (2, 4096)), first_taps)
    solo = stages.main(target, reference, cfg, device=dev, eq=eq)
    assert np.array_equal(album[0][0], solo[0])
    own = stages.main(second, reference, cfg, device=dev, eq=eq)
    _, own_taps = run(dev, (second, reference), 4096, eq)
    assert not np.array_equal(own_taps, first_taps) and not np.array_equal(album[1][0], own[0])
    with dev.lock:
        fir = dev.upload(first_taps)
        try:
            given = stages.main(second, reference, cfg, device=dev, fir=fir)
        finally:
            fir.release()
    assert np.array_equal(album[1][0], given[0])
