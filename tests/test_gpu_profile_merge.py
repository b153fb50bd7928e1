"""Reference sets on the GPU (include/mgx.h: mgx_profile_merge; profile.py: ReferenceProfile.merge): several
reference profiles pooled into one over the union of their loud pieces, and targets mastered against the result.

Bounds.  Outputs: 1e-5 RMS (RMS_TOL of tests/test_gpu_parity.py / test_gpu_profile.py); the FIR pair: 1e-6 of the peak
tap; the report's scalars: 1e-6 relative.  The merge's own arithmetic is a fixed-order float64 sum of R non-negative
products, one division and, for the two RMS fields, one square root: first-order error (R + 3) / 2 * 2^-52 relative at
most, and every float field is held to twice that, (R + 3) * 2^-52, of the exact value -- computed here from the source
blobs in rationals (``fractions.Fraction``; the square roots in 60-digit decimals), and for the large shapes in x87
extended precision, whose own error of R * 2^-64 is a thousandth of the bound.  Integer fields are exact.
"""

import ctypes
import decimal
import math
from fractions import Fraction

import numpy as np
import pytest
from scipy import signal

import mastering_oracle as mo
from cases import CASES, build_inputs, hard_material, oracle_params
from conftest import rms_error
from test_gpu_profile import RMS_TOL, make_config, master_on_device

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52


def merge_bound(sources):
    return (sources + 3) * ULP


# ---- forged sources: no audio needed, so the kernel's edge shapes are cheap ------------------------------------------
def forge(cfg, seed, **fields):
    """The bytes of a profile as the device would pack it for ``cfg``, from made-up analysis results."""
    from matchering_amd import _native

    rng = np.random.RandomState(seed)
    fft = fields.get("fft_size", cfg.fft_size)               # (a foreign block is as long as its OWN fft_size makes it)
    divisions = int(rng.randint(1, 12))
    piece = int(rng.randint(fft, 4 * fft + 2))
    peak = float(rng.uniform(0.2, 1.0))
    header = dict(
        magic=_native.PROFILE_MAGIC, version=_native.PROFILE_VERSION, internal_sample_rate=cfg.internal_sample_rate,
        fft_size=fft, max_piece_size=float(cfg.max_piece_size), threshold=float(cfg.threshold),
        min_value=float(cfg.min_value), frames=piece * divisions + int(rng.randint(0, divisions)), piece=piece,
        divisions=divisions, loud_count=int(rng.randint(1, divisions + 1)), peak=peak,
        amplitude_coefficient=min(1.0, peak / cfg.threshold), average_rms=float(rng.uniform(0.01, 0.3)),
        match_rms=float(rng.uniform(0.02, 0.5)))
    header.update(fields)
    spectra = np.abs(rng.randn(2, fft // 2 + 1)) * 10.0 ** rng.uniform(-6, -1, (2, 1))
    return bytes(_native.MgxProfileHeader(**header)) + spectra.astype("<f8").tobytes()


def forged_profiles(cfg, count, seed=0):
    from matchering_amd import ReferenceProfile

    return [ReferenceProfile(forge(cfg, 1000 * seed + i)) for i in range(count)]


def exact_sqrt(value):
    """The square root of a Fraction to 60 digits, as a Fraction."""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        root = (decimal.Decimal(value.numerator) / decimal.Decimal(value.denominator)).sqrt()
    return Fraction(root)


def check_merged(merged, sources, weights, bound):
    """Every field of ``merged`` against the table of include/mgx.h, evaluated exactly from the sources' bytes."""
    weights = [1] * len(sources) if weights is None else weights
    first = sources[0]
    for name in ("internal_sample_rate", "fft_size", "max_piece_size", "threshold", "min_value"):
        assert getattr(merged, name) == getattr(first, name), name
    counts = [w * s.loud_count for w, s in zip(weights, sources)]
    pieces = [w * s.divisions for w, s in zip(weights, sources)]
    total = sum(counts)
    assert merged.loud_count == total
    assert merged.divisions == sum(pieces)
    assert merged.frames == sum(w * s.frames for w, s in zip(weights, sources))
    assert merged.piece == (first.piece if all(s.piece == first.piece for s in sources) else 0)
    assert merged.peak == max(s.peak for s in sources)
    assert merged.amplitude_coefficient == max(s.amplitude_coefficient for s in sources)
    worst = 0.0
    for name, ns in (("match_rms", counts), ("average_rms", pieces)):
        exact = exact_sqrt(sum(n * Fraction(getattr(s, name)) ** 2 for n, s in zip(ns, sources)) / sum(ns))
        error = float(abs(Fraction(getattr(merged, name)) - exact) / exact)
        worst = max(worst, error)
        assert error <= bound, (name, error, bound)
    got = merged.spectra.reshape(-1)
    planes = [s.spectra.reshape(-1) for s in sources]
    if got.size * len(sources) <= 4096:
        for k in range(got.size):
            exact = sum(n * Fraction(float(p[k])) for n, p in zip(counts, planes)) / total
            error = float(abs(Fraction(float(got[k])) - exact) / exact)
            worst = max(worst, error)
            assert error <= bound, (k, error, bound)
    else:
        assert np.finfo(np.longdouble).nmant >= 63                       # (x87 extended: R * 2^-64 of its own)
        exact = np.zeros(got.size, np.longdouble)
        for n, p in zip(counts, planes):
            exact += np.longdouble(n) * p.astype(np.longdouble)
        exact /= np.longdouble(total)
        error = float((np.abs(got.astype(np.longdouble) - exact) / exact).max())
        worst = max(worst, error)
        assert error <= bound, (error, bound)
    return worst


# ---- 1. shapes --------------------------------------------------------------------------------------------------------
# fft_size 8: 10 values, one partial workgroup; 4096: 8196 values, 32 workgroups and a tail of 4; 65536: 65538 values.
# 65 and 130 sources go through Python's grouping (64 + 1 and 64 + 64 + 2, then the group results).
@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "mixed"])
@pytest.mark.parametrize("count", [1, 2, 3, 64, 65, 130])
@pytest.mark.parametrize("fft", [8, 4096, 65536])
def test_merge_shapes(fft, count, weighted):
    import matchering_amd as mg
    from matchering_amd import ReferenceProfile
    from matchering_amd.profile import profile_bytes

    cfg = mg.Config(fft_size=fft, max_piece_size=3.0)
    sources = forged_profiles(cfg, count, seed=fft % 97 + count)
    weights = None
    if weighted:
        rng = np.random.RandomState(count)
        weights = [int(w) for w in rng.randint(1, 65537, count)]
        weights[0], weights[-1] = 65536, 1
    merged = ReferenceProfile.merge(sources, weights)
    assert len(merged.tobytes()) == profile_bytes(cfg) and merged.matches(cfg)
    worst = check_merged(merged, sources, weights, merge_bound(count))
    print(f"fft {fft}, {count} sources, weights {'mixed' if weighted else 'ones'}: worst error {worst / ULP:.2f} x 2^-52, "
          f"bound {count + 3}")
    if count == 1 and (not weighted or weights == [1]):
        assert merged.tobytes() == sources[0].tobytes()


def test_merge_of_one_source_is_that_source_byte_for_byte():
    import matchering_amd as mg
    from matchering_amd import ReferenceProfile

    for fft in (8, 4096, 65536):
        cfg = mg.Config(fft_size=fft, max_piece_size=3.0)
        for source in forged_profiles(cfg, 3, seed=7):                    # (loud counts that are no powers of two among them)
            assert ReferenceProfile.merge([source]).tobytes() == source.tobytes()
            assert ReferenceProfile.merge([source], [1]).tobytes() == source.tobytes()
            twice = ReferenceProfile.merge([source], [2])
            assert (twice.loud_count, twice.divisions, twice.frames) == (2 * source.loud_count, 2 * source.divisions, 2 * source.frames)
            check_merged(twice, [source], [2], merge_bound(1))


# ---- 2. associativity ---------------------------------------------------------------------------------------------------
def same_but_for_rounding(x, y, bound):
    for name in ("internal_sample_rate", "fft_size", "max_piece_size", "threshold", "min_value", "frames", "piece",
                 "divisions", "loud_count", "peak", "amplitude_coefficient"):
        assert getattr(x, name) == getattr(y, name), name
    for name in ("match_rms", "average_rms"):
        assert abs(getattr(x, name) / getattr(y, name) - 1.0) <= bound, name
    assert np.abs(x.spectra / y.spectra - 1.0).max() <= bound


@pytest.mark.parametrize("fft", [8, 4096])
def test_merging_is_associative(fft):
    import matchering_amd as mg
    from matchering_amd import ReferenceProfile

    cfg = mg.Config(fft_size=fft, max_piece_size=3.0)
    a, b, c = forged_profiles(cfg, 3, seed=11)
    flat = ReferenceProfile.merge([a, b, c])
    nested = ReferenceProfile.merge([ReferenceProfile.merge([a, b]), c])
    # each is within the bound for three sources of the exact value (the nested one: twice over)
    same_but_for_rounding(nested, flat, 2 * merge_bound(3))
    check_merged(nested, [a, b, c], None, 2 * merge_bound(3))
    same_but_for_rounding(ReferenceProfile.merge([a, b], weights=[2, 1]), ReferenceProfile.merge([a, a, b]), 2 * merge_bound(3))
    same_but_for_rounding(ReferenceProfile.merge([c, ReferenceProfile.merge([a, b])]), ReferenceProfile.merge([c, a, b]),
                          2 * merge_bound(3))


# ---- 3. refusals, straight through the C ABI ------------------------------------------------------------------------------
def raw_merge(dev, blobs, weights, cfg, count=None, out=None):
    """mgx_profile_merge on uploaded bytes: (return code, message, the sources' buffers, the output buffer)."""
    from matchering_amd import _native
    from matchering_amd.profile import profile_bytes

    lib = _native.library()
    native = cfg.to_native()
    bufs = [dev.upload(np.frombuffer(blob, dtype=np.uint8), dtype=None) for blob in blobs]
    out = dev.alloc(profile_bytes(cfg)) if out is None else out
    count = len(bufs) if count is None else count
    pointers = (ctypes.c_void_p * max(1, count, len(bufs)))(*[b.ptr for b in bufs])
    counted = None if weights is None else (ctypes.c_int32 * len(weights))(*weights)
    rc = lib.mgx_profile_merge(dev.handle, pointers, counted, count, ctypes.byref(native), ctypes.c_void_p(getattr(out, "ptr", out)))
    return rc, lib.mgx_last_error().decode(), bufs, out


def header_of(dev, buf):
    from matchering_amd import _native

    raw = np.array(dev.download(buf, (ctypes.sizeof(_native.MgxProfileHeader),), np.uint8))
    return _native.MgxProfileHeader.from_buffer_copy(raw.tobytes())


REFUSED = {
    "fft_size at 0": (0, "fft_size", lambda blob, cfg: forge(cfg, 5, fft_size=8)),          # 176 bytes where 8304 are expected
    "threshold at 2": (2, "threshold", lambda blob, cfg: forge(cfg, 5, threshold=0.9)),
    "magic at 1": (1, "magic", lambda blob, cfg: bytes([blob[0] ^ 0x40]) + blob[1:]),
    "loud_count at 2": (2, "loud_count", lambda blob, cfg: forge(cfg, 5, loud_count=0)),
    "counts beyond int32": (1, "loud_count", lambda blob, cfg: forge(cfg, 5, loud_count=40000, divisions=40000)),
}


@pytest.mark.parametrize("which", sorted(REFUSED))
def test_a_source_that_does_not_fit_is_refused_by_name_and_position(which):
    import matchering_amd as mg
    from matchering_amd import ReferenceProfile, stages
    from matchering_amd._native import ERR_ARGUMENT, MgxError
    from matchering_amd.device import default_device
    from matchering_amd.synth import make_pair

    position, field, spoil = REFUSED[which]
    cfg = mg.Config(fft_size=1024, max_piece_size=1.0)
    good = [forge(cfg, seed) for seed in (1, 2, 3)]
    blobs = list(good)
    blobs[position] = spoil(blobs[position], cfg)
    weights = [1, 65536, 1] if which == "counts beyond int32" else None          # 40000 * 65536 > 2^31 - 1
    target, _ = make_pair(1.5, 44100, pair=3)
    dev = default_device()
    with dev.lock:
        rc, message, bufs, out = raw_merge(dev, blobs, weights, cfg)
        try:
            assert rc == 0, message                                # only queued: the device finds out
            with pytest.raises(MgxError, match=field) as caught:
                dev.synchronize()                                  # the next blocking call
            assert caught.value.code == ERR_ARGUMENT and f"source {position} of the merge" in str(caught.value)
            assert header_of(dev, out).magic == 0                  # never a usable profile
            td, res = dev.upload(target), dev.alloc(target.shape[0] * 8)
            try:
                with pytest.raises(MgxError, match="magic") as caught:
                    dev.master(td, target.shape[0], None, 0, cfg.to_native(), res, profile=out)
                assert caught.value.code == ERR_ARGUMENT and "of the merge" not in str(caught.value)
            finally:
                td.release(), res.release()
        finally:
            for b in bufs + [out]:
                b.release()
    # the same handle then merges and masters correctly
    sources = [ReferenceProfile(blob) for blob in good]
    merged = ReferenceProfile.merge(sources, device=dev)
    check_merged(merged, sources, None, merge_bound(3))
    again = stages.main(target, merged, cfg, device=dev)[0]
    assert np.isfinite(again).all() and np.array_equal(again, stages.main(target, ReferenceProfile(merged.tobytes()), cfg, device=dev)[0])


def test_host_side_refusals_of_the_entry_point():
    import matchering_amd as mg
    from matchering_amd import _native
    from matchering_amd._native import ERR_ARGUMENT
    from matchering_amd.device import default_device
    from matchering_amd.profile import profile_bytes

    cfg = mg.Config(fft_size=1024, max_piece_size=1.0)
    blobs = [forge(cfg, seed) for seed in (1, 2)]
    nbytes = profile_bytes(cfg)
    native = cfg.to_native()
    merge = _native.library().mgx_profile_merge
    dev = default_device()
    with dev.lock:
        keep = []
        try:
            for kwargs, word in ((dict(count=0), "1 to 64"), (dict(count=65), "1 to 64"), (dict(weights=[1, 0]), "weight"),
                                 (dict(weights=[65537, 1]), "weight")):
                rc, message, bufs, out = raw_merge(dev, blobs, kwargs.pop("weights", None), cfg, **kwargs)
                keep += bufs + [out]
                assert rc == ERR_ARGUMENT and word in message, (rc, message)
            # the output on a source, and overlapping one from either side
            rc, message, bufs, out = raw_merge(dev, blobs, None, cfg)
            keep += bufs + [out]
            assert rc == 0, message
            room = dev.alloc(3 * nbytes)
            keep.append(room)
            for src, dst in ((bufs[1].ptr, bufs[1].ptr), (room.ptr + nbytes, room.ptr + 8), (room.ptr + nbytes, room.ptr + 2 * nbytes - 8)):
                pointers = (ctypes.c_void_p * 2)(bufs[0].ptr, src)       # (refused before anything is launched on them)
                rc = merge(dev.handle, pointers, None, 2, ctypes.byref(native), ctypes.c_void_p(dst))
                assert rc == ERR_ARGUMENT and b"overlaps the source at position 1" in _native.library().mgx_last_error()
            null = (ctypes.c_void_p * 2)(bufs[0].ptr, None)
            assert merge(dev.handle, null, None, 2, ctypes.byref(native), ctypes.c_void_p(out.ptr)) == ERR_ARGUMENT
            assert merge(dev.handle, pointers, None, 2, ctypes.byref(native), None) == ERR_ARGUMENT
            assert merge(dev.handle, pointers, None, 2, None, ctypes.c_void_p(out.ptr)) == ERR_ARGUMENT
            dev.synchronize()                                       # nothing that was refused left anything behind
        finally:
            for b in keep:
                b.release()


def test_a_source_that_carries_a_nan_makes_no_merged_profile():
    import matchering_amd as mg
    from matchering_amd import ReferenceProfile
    from matchering_amd._native import ERR_ARGUMENT, MgxError

    cfg = mg.Config(fft_size=1024, max_piece_size=1.0)
    good = ReferenceProfile(forge(cfg, 1))
    for field in ("match_rms", "amplitude_coefficient"):
        bad = ReferenceProfile(forge(cfg, 2, **{field: float("nan")}))
        with pytest.raises(MgxError, match="not finite") as caught:
            ReferenceProfile.merge([good, bad])
        assert caught.value.code == ERR_ARGUMENT
    check_merged(ReferenceProfile.merge([good, good]), [good, good], None, merge_bound(2))


# ---- 4. against the oracle, on real audio ---------------------------------------------------------------------------------
def pooled_master(target, references, cfg, trace=None):
    """``mo.master`` with the reference's three contributions pooled over the loud pieces of several references, each
    normalised, cut and selected on its own: stage 1 per source, the reference's formulas (match_levels.py:62-71,
    match_frequencies.py:30-42) over the union of the loud-piece lists with the piece as the unit, then stages 2-4 of
    ``mo.master`` restated with the pooled match RMS, spectra and coefficient."""
    target = np.asarray(target, dtype=np.float64)
    eps = cfg.min_value
    sources, coefficients = [], []
    for reference in references:
        reference, c = mo.peak_normalize(np.asarray(reference, dtype=np.float64), cfg.threshold, eps, always=False)
        sources.append(mo.analyze(reference, cfg))
        coefficients.append(c)
    final_c = max(coefficients)                       # normalize_reference on the concatenation: its peak is the largest
    counts = [len(r.loud_idx) for r in sources]
    total = sum(counts)
    loudest = [r.rmses[r.loud_idx] for r in sources]
    match = math.sqrt(sum(float(sel @ sel) for sel in loudest) / total)            # get_average_rms over the union
    t = mo.analyze(target, cfg)
    c0 = match / max(eps, t.match_rms)
    t_mid, t_side = t.mid * c0, t.side * c0

    firs, designs = [], []
    for mine, theirs in ((t.mid_loud, [r.mid_loud for r in sources]), (t.side_loud, [r.side_loud for r in sources])):
        a_t = mo.average_spectrum(mine * c0, cfg.fft_size)
        a_r = sum((n / total) * mo.average_spectrum(rows, cfg.fft_size) for n, rows in zip(counts, theirs))
        raw = a_r / np.maximum(cfg.min_value, a_t)
        taps = np.fft.irfft(mo.smooth_matching_curve(raw, cfg))
        firs.append(np.fft.ifftshift(taps) * signal.windows.hann(taps.shape[0]))
        designs.append(a_r)
    y, y_mid = mo.convolve_same(t_mid, firs[0], t_side, firs[1])

    coeffs = []
    for _ in range(cfg.rms_correction_steps):
        clipped = np.clip(y_mid, -1.0, 1.0)
        _, rm, avg = mo.piece_rms(clipped, t.piece, t.divisions)
        _, m = mo.loud_pieces(rm, avg)
        c = match / max(eps, m)
        coeffs.append(c)
        y_mid = y_mid * c
        y = y * c

    out_norm, norm_c = mo.peak_normalize(y, cfg.threshold, eps, always=True)
    out = mo.limit(y, cfg) * final_c
    if trace is not None:
        trace.update(final_amplitude_coefficient=final_c, coefficients=coefficients, rms_coefficient=c0, match_rms=match,
                     target_match_rms=t.match_rms, loud_counts=counts, divisions=[r.divisions for r in sources],
                     pieces=[r.piece for r in sources], fir_mid=firs[0], fir_side=firs[1], spectra=designs,
                     correction_coefficients=np.array(coeffs), normalize_coefficient=norm_c)
    return out, y, out_norm


LOUD_COUNTS = {"cd_default": (2, 2, 4), "quiet_reference": (3, 2, 6), "hot_lowrate": (1, 1, 4)}
COEFFICIENTS = {"cd_default": (1, 0.476, 0.740), "quiet_reference": (0.480, 0.476, 1), "hot_lowrate": (1, 0.476, 1)}


@pytest.fixture(scope="module")
def pooled():
    """name -> what the oracle says about the case's target against the set [A, B, C]; computed once, left unchanged."""
    from matchering_amd.synth import make_pair

    cache = {}

    def run(name):
        if name not in cache:
            case = CASES[name]
            sr, seconds = case["sample_rate"], case["reference_seconds"]
            target, a = build_inputs(case)
            b = (0.5 * hard_material("panned_chirp_impulses", 0.77 * seconds, sr, 3)).astype(np.float32)
            c = make_pair(1.0, sr, 11, reference_seconds=2.3 * seconds, reference_gain=1.2)[1]
            params = oracle_params(case["config"])
            # the composition with ONE source is mo.master itself
            alone = [mo.master(target, r, params, True, True, True) for r in (a, b, c)]
            for mine, theirs in zip(pooled_master(target, [a], params), alone[0]):
                assert np.array_equal(mine, theirs)
            sets = {"abc": [a, b, c]}
            if name == "quiet_reference":
                sets["ab"] = [a, b]
            want = {}
            for key, members in sets.items():
                trace = {}
                outs = pooled_master(target, members, params, trace)
                # not vacuous: the pooled master is nobody's own
                apart = [rms_error(outs[0], single[0]) for single in alone[:len(members)]]
                print(f"{name} {key}: pooled against each single source, rms {apart}")
                assert min(apart) >= 1e-3
                want[key] = (members, outs, trace)
            cache[name] = (target, make_config(case["config"]), want)
        return cache[name]

    return run


@pytest.mark.parametrize("name, key", [("cd_default", "abc"), ("quiet_reference", "abc"), ("quiet_reference", "ab"),
                                       ("hot_lowrate", "abc")])
def test_pooled_master_matches_the_oracle(name, key, pooled):
    from matchering_amd import ReferenceProfile

    target, cfg, want = pooled(name)
    members, outs, trace = want[key]
    assert tuple(trace["loud_counts"]) == LOUD_COUNTS[name][:len(members)]
    assert [round(c, 3) for c in trace["coefficients"]] == list(COEFFICIENTS[name][:len(members)])
    assert len(set(trace["pieces"])) > 1                              # the pieces differ: the merged `piece` is 0
    if key == "ab":
        assert trace["final_amplitude_coefficient"] < 1.0            # the final scaling is exercised
    profile = ReferenceProfile.analyze(members, cfg)
    assert profile.loud_count == sum(trace["loud_counts"]) and profile.divisions == sum(trace["divisions"])
    assert profile.piece == 0 and profile.frames == sum(m.shape[0] for m in members)
    rep, res, fir = master_on_device(target, cfg, profile=profile)
    errs = [rms_error(mine, theirs) for mine, theirs in zip(res, outs)]
    taps = [float(np.abs(mine - theirs).max() / np.abs(theirs).max()) for mine, theirs in ((fir[0], trace["fir_mid"]), (fir[1], trace["fir_side"]))]
    rel = lambda x, y: abs(x / y - 1.0)                                          # noqa: E731
    scalars = {"reference_match_rms": rel(rep.reference_match_rms, trace["match_rms"]),
               "final_amplitude_coefficient": rel(rep.final_amplitude_coefficient, trace["final_amplitude_coefficient"]),
               "rms_coefficient": rel(rep.rms_coefficient, trace["rms_coefficient"]),
               "target_match_rms": rel(rep.target_match_rms, trace["target_match_rms"]),
               "normalize_coefficient": rel(rep.normalize_coefficient, trace["normalize_coefficient"]),
               "correction_coefficients": float(np.abs(np.array(rep.correction_coefficients[:cfg.rms_correction_steps])
                                                       / trace["correction_coefficients"] - 1.0).max())}
    print(f"{name} {key}: outputs rms {errs}, taps {taps} of the peak tap, scalars {scalars}")
    assert max(errs) <= RMS_TOL
    assert max(taps) <= 1e-6
    assert max(scalars.values()) <= 1e-6, scalars
    assert (rep.reference_loud_count, rep.reference_divisions, rep.reference_piece) == (profile.loud_count, profile.divisions, 0)
    for mine, theirs in zip(profile.spectra, trace["spectra"]):
        assert np.abs(mine - theirs).max() <= 2e-6 * theirs.max()              # (test_gpu_profile.py's bound for a profile's spectra)


# ---- 5. tie to the unmodified reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cd_default", "quiet_reference"])
def test_a_profile_merged_with_itself_masters_to_the_reference_golden(name, golden):
    from matchering_amd import ReferenceProfile, stages

    g = golden(name)
    target, reference = build_inputs(CASES[name])
    cfg = make_config(CASES[name]["config"])
    own = ReferenceProfile.analyze(reference, cfg)
    twice = ReferenceProfile.merge([own, own])
    assert twice.loud_count == 2 * own.loud_count and twice != own
    res, res_nl, res_nln = stages.main(target, twice, cfg, True, True, True)
    assert rms_error(res, g["result_f32"]) <= RMS_TOL
    assert rms_error(res_nl, g["result_no_limiter_f32"]) <= RMS_TOL
    assert rms_error(res_nln[g["sparse_index"]], g["result_no_limiter_normalized_sparse"]) <= RMS_TOL


# ---- 6. files end to end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    import matchering_amd as mg
    from matchering_amd import ReferenceProfile, audio_io
    from matchering_amd.synth import make_pair

    folder = tmp_path_factory.mktemp("reference_set")
    sr = 44100
    cfg = mg.Config(max_piece_size=1.0)
    paths = {}
    for i, name in enumerate(("a", "b", "c")):
        paths[name] = str(folder / f"{name}.wav")
        audio_io.write_wav(paths[name], make_pair(2.0, sr, pair=60 + i, reference_seconds=1.6 + 0.5 * i, reference_gain=1.0 + i)[1],
                           sr, "PCM_16")
    for i in range(3):
        paths[f"t{i}"] = str(folder / f"target{i}.wav")
        audio_io.write_wav(paths[f"t{i}"], make_pair(2.0 + 0.3 * i, sr, pair=70 + i)[0], sr, "FLOAT")
    paths["b_saved"] = str(folder / "b.profile")
    ReferenceProfile.analyze(paths["b"], cfg).save(paths["b_saved"])
    return folder, cfg, paths


def test_process_with_a_set_of_files(files):
    import matchering_amd as mg
    from matchering_amd import ReferenceProfile, audio_io, stages

    folder, cfg, paths = files
    several = [paths["a"], paths["b_saved"], paths["c"]]
    out = str(folder / "set.wav")
    codes = []
    mg.log(lambda m: codes.append(m.split(":")[0]), show_codes=True)
    try:
        mg.process(paths["t0"], several, [mg.Result(out, "FLOAT")], config=cfg)
    finally:
        mg.log()
    assert [c for c in codes if c.startswith("20")] == ["2003", "2004", "2005", "2006", "2007", "2008", "2010"]
    profile = ReferenceProfile.analyze(several, cfg)
    assert profile.loud_count == sum(ReferenceProfile.analyze(paths[k], cfg).loud_count for k in "abc")
    want = stages.main(audio_io.read_wav(paths["t0"])[0], profile, cfg)[0]
    assert np.array_equal(audio_io.read_wav(out)[0], want)
    assert ReferenceProfile.analyze(tuple(several), cfg) == profile            # (the same bytes, whoever asks)
    assert ReferenceProfile.analyze([paths["b"]], cfg) == ReferenceProfile.load(paths["b_saved"])


def test_a_two_lane_batch_of_reference_sets(files):
    import matchering_amd as mg
    from matchering_amd import audio_io, batch

    folder, cfg, paths = files
    sets = ([paths["a"], paths["b"]], [paths["b_saved"], paths["c"]], [paths["a"], paths["b"]])
    written = {}
    for how, share in (("shared", True), ("alone", False)):
        jobs = [{"target": paths[f"t{i}"], "references": several, "results": [mg.Result(str(folder / f"{how}{i}.wav"), "FLOAT")]}
                for i, several in enumerate(sets)]
        assert batch.process_batch(jobs, cfg, rank=0, world_size=1, device_index=0, lanes=2, share_references=share) == [0, 1, 2]
        written[how] = [audio_io.read_wav(job["results"][0].file)[0] for job in jobs]
    for i, (shared, alone) in enumerate(zip(written["shared"], written["alone"])):
        assert rms_error(shared, alone) <= RMS_TOL, i
    single = str(folder / "single.wav")
    mg.process(paths["t1"], sets[1], [mg.Result(single, "FLOAT")], config=cfg)
    assert rms_error(written["shared"][1], audio_io.read_wav(single)[0]) <= RMS_TOL
