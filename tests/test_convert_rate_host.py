"""The deliveries' sample-rate converter without a GPU: the per-thread phase functions of csrc/convert_rate_kernel.h driven
on the CPU by tests/emu/libmgx_emu_convert_rate.so and held bit for bit to the emulation of ``k_resample`` (which
tests/test_resample_plan.py holds to ``resample.resample``), the tiling rule, tiles far into a long track, and what
``Delivery(sample_rate=...)`` and ``mgx_convert_rate`` decide before they touch a device.
"""

import ctypes
import os

import numpy as np
import pytest

import emu_build
from matchering_amd import _native
from matchering_amd import resample as host

# fourteen rate pairs: the eight of the loader's design table (tests/test_resample_plan.py), the delivery pairs of the
# GPU tests that are not among them, 48 -> 96 kHz, and one the plan refuses (11014 phases)
REFUSED = (44100, 44056)
PAIRS = [(48000, 44100), (44100, 48000), (96000, 44100), (192000, 44100), (8000, 44100), (32000, 44100), (22050, 44100),
         (88200, 44100), (44100, 96000), (44100, 88200), (96000, 48000), (44100, 8000), (48000, 96000)]
assert len(PAIRS) + 1 == 14 and REFUSED not in PAIRS
# the rule's table: pair -> (L, M, W, P, span)
TABLE = {(44100, 48000): (160, 147, 130, 8, 2482), (48000, 44100): (147, 160, 140, 8, 2700),
         (96000, 44100): (147, 320, 280, 4, 2840), (192000, 44100): (147, 640, 562, 2, 3122),
         (44100, 8000): (80, 441, 714, 2, 4242), (44100, 88200): (2, 1, 130, 8, 1154)}
SPAN_MAX = 7680                     # RESAMPLE_SPAN_MAX: what a launch's LDS holds
SPAN_SHARED = 5120                  # CONVERT_RATE_SPAN_MAX: what the rule lets a tile of P > 1 stage (four workgroups on a CU)


@pytest.fixture(scope="module")
def emu():
    lib = emu_build.load("convert_rate")
    lib.emu_convert_rate_launch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p]
    lib.emu_convert_rate.restype = ctypes.c_longlong
    lib.emu_convert_rate.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def old():
    lib = emu_build.load("resample")
    lib.emu_resample.restype = ctypes.c_longlong
    lib.emu_resample.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_void_p, ctypes.c_void_p]
    return lib


def geometry(old, sr, new):
    g = (ctypes.c_int * 6)()
    assert old.emu_resample_geometry(sr, new, g) == 0
    return g[0], g[1], g[3]                                         # L, M, W


def tiling(emu, sr, new, forced=0):
    t = (ctypes.c_int * 3)()
    assert emu.emu_convert_rate_tiling(sr, new, forced, t) == 0
    return tuple(t)                                                 # P (0: it does not fit), S, span


def rule(L, M, W):
    """The rule restated: S = L ceil(256 / L); the largest P of 8, 4, 2 with P (S / L) M + W <= 5120 frames (40 KB: four
    workgroups on a CU), else P = 1 where (S / L) M + W <= 7680 frames.  (The issue's first rule took the largest P that
    fits 7680; the A/B of DESIGN.md section 3.14 moved it: 96 -> 44.1 kHz from 8 to 4, 192 -> 44.1 kHz from 4 to 2.)"""
    S = L * -(-256 // L)
    for P in (8, 4, 2, 1):
        if P * (S // L) * M + W <= (SPAN_SHARED if P > 1 else SPAN_MAX):
            return P, S, P * (S // L) * M + W
    return None


def length(n, sr, new):
    return int(n * (float(new) / sr))


def inputs_for(n_out, sr, new):
    """An input length that gives exactly n_out outputs, or None where the ratio steps over it."""
    n = max(0, int(n_out * sr / new) - 2)
    while length(n, sr, new) < n_out:
        n += 1
    return n if length(n, sr, new) == n_out else None


def converted(emu, x, sr, new, forced=0):
    n = x.shape[0]
    n_out = length(n, sr, new)
    sums, out = np.zeros((n_out, 2)), np.full((n_out, 2), np.nan, dtype=np.float32)
    rc = emu.emu_convert_rate(x.ctypes.data, n, 0, sr, new, forced, 0, sums.ctypes.data, out.ctypes.data)
    assert rc == n_out, rc
    return sums, out


def resampled(old, x, sr, new):
    n = x.shape[0]
    n_out = length(n, sr, new)
    sums, out = np.zeros((n_out, 2)), np.full((n_out, 2), np.nan, dtype=np.float32)
    assert old.emu_resample(x.ctypes.data, n, 2, sr, new, sums.ctypes.data, out.ctypes.data) == n_out
    return sums, out


def test_the_tiling_rule_gives_the_table(emu, old):
    for pair, (L, M, W, P, span) in TABLE.items():
        assert geometry(old, *pair) == (L, M, W), pair
        got = tiling(emu, *pair)
        assert got == rule(L, M, W), pair
        assert got[0] == P and got[2] == span and got[1] == L * -(-256 // L), (pair, got)
    for pair in PAIRS:
        assert tiling(emu, *pair) == rule(*geometry(old, *pair)), pair
    t = (ctypes.c_int * 3)()
    assert emu.emu_convert_rate_tiling(*REFUSED, 0, t) == -1
    # forcing a P: that P where the launch's LDS holds it, or nothing
    assert tiling(emu, 192000, 44100, 8)[0] == 0 and tiling(emu, 192000, 44100, 4) == (4, 294, 5682)
    assert tiling(emu, 96000, 44100, 8) == (8, 294, 5400)
    assert tiling(emu, 44100, 8000, 4)[0] == 0 and tiling(emu, 44100, 8000, 1)[0] == 1


@pytest.mark.parametrize("sr,new", PAIRS)
def test_the_launch_is_the_tilings(emu, sr, new):
    """What ``convert_rate_launch`` gives ``mgx_convert_rate`` and the emulation alike, for the rule's P and every
    forced one that fits: the tiling's P, LDS for its span as float2 frames, within what a launch may ask for
    (RESAMPLE_SPAN_MAX frames), and a workgroup per tile of P S outputs."""
    launch = (ctypes.c_longlong * 3)()
    for forced in (0, 1, 2, 4, 8):
        P, S, span = tiling(emu, sr, new, forced)
        if not P:
            assert emu.emu_convert_rate_launch(sr, new, forced, 1, launch) == 0 and launch[0] == 0
            continue
        tile = P * S
        for n_out in (1, tile - 1, tile, tile + 1):
            assert emu.emu_convert_rate_launch(sr, new, forced, n_out, launch) == 0
            got_P, grid, lds = launch
            assert got_P == P
            assert lds == span * 8
            assert lds <= SPAN_MAX * 8
            assert grid == -(-n_out // tile), (forced, n_out, grid)
    assert emu.emu_convert_rate_launch(*REFUSED, 0, 1, launch) == -1


def test_p_1_is_always_reachable(emu, old):
    """A pair ``mgx_resample`` accepts whose single period does not fit the LDS (L >= 256, M + W > 7680 frames) is run
    at P = 1 on k_resample's own 256-output tile, and stays bit-identical."""
    sr, new = 150000, 7001                                          # L = 7001 > 4096: refused by the plan itself
    g = (ctypes.c_int * 6)()
    assert old.emu_resample_geometry(sr, new, g) == -1
    sr, new = 6 * 7993, 6 * 4001                                    # L = 4001, M = 7993: one period reaches 7993 + 258 frames
    assert old.emu_resample_geometry(sr, new, g) == 0 and g[0] == 4001 and g[1] == 7993
    P, S, span = tiling(emu, sr, new)
    assert (P, S, span) == (1, 256, g[5]) and rule(g[0], g[1], g[3]) is None
    x = (0.3 * np.random.RandomState(3).randn(40000, 2)).astype(np.float32)
    got, want = converted(emu, x, sr, new), resampled(old, x, sr, new)
    assert want[1].shape[0] == length(40000, sr, new) > 1000
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def lengths_for(sr, new, M, P, S):
    """The input lengths of the identity test for one forced P."""
    wanted = {1, 2, 5, M - 1, M, M + 1}
    for tiles in (1, 2, 3):
        for d in range(-3, 4):
            n = inputs_for(tiles * P * S + d, sr, new)
            if n is not None:
                wanted.add(n)
    n = inputs_for(3 * P * S + 77, sr, new)
    wanted.add(n if n is not None else inputs_for(3 * P * S + 78, sr, new))
    return sorted(v for v in wanted if v >= 1)


@pytest.mark.parametrize("sr,new", PAIRS)
def test_emulated_kernel_is_k_resample_bit_for_bit(emu, old, sr, new):
    """float32 output AND float64 accumulators equal those of ``k_resample<2>``'s emulation: every forced P that fits,
    the shortest tracks, M and its neighbours, every length around one, two and three whole tiles, three tiles + 77.
    LDS is pre-filled with 1e30 for each tile, so a read of a slot the stage did not write would show."""
    L, M, W = geometry(old, sr, new)
    rng = np.random.RandomState(sr % 991 + new % 97)
    ran = 0
    longest = max(max(lengths_for(sr, new, M, P, tiling(emu, sr, new, P)[1])) for P in (1, 2, 4, 8)
                  if tiling(emu, sr, new, P)[0])
    track = (0.3 * rng.randn(longest, 2)).astype(np.float32)
    reference = {}
    for P in (1, 2, 4, 8):
        fits, S, span = tiling(emu, sr, new, P)
        if not fits:
            assert P > rule(L, M, W)[0] and P * -(-256 // L) * M + W > SPAN_MAX
            continue
        assert span <= SPAN_MAX
        for n in lengths_for(sr, new, M, P, S):
            x = np.ascontiguousarray(track[:n])
            if n not in reference:
                reference[n] = resampled(old, x, sr, new)
            sums, out = converted(emu, x, sr, new, P)
            assert np.array_equal(sums, reference[n][0]), (sr, new, P, n)
            assert np.array_equal(out, reference[n][1]), (sr, new, P, n)          # (NaN where a frame was not stored: unequal)
            ran += 1
    assert ran >= 20
    # ... and the rule's own choice on the longest of them
    sums, out = converted(emu, track, sr, new)
    assert np.array_equal(out, reference[longest][1]) and np.array_equal(sums, reference[longest][0])


def test_tiles_far_into_a_long_track(emu, old):
    """Tiles whose input and output byte offsets lie beyond 2^31 (the library converts up to 500 M frames), run without
    the frames before them: the track is zero up to a cut at a multiple of M and real after it, so the host resampler
    on the tail alone computes the same outputs; phases and slots come from 64-bit t M / L.  Bound as in
    tests/test_resample_plan.py: max|x| (sum|w| W 2^-53 + W 2e-15)."""
    sr, new = 48000, 44100
    L, M, W = geometry(old, sr, new)
    P, S, _ = tiling(emu, sr, new)
    n = 300_000_000 + 1234
    cut = (n - 2 * sr) // M * M
    assert cut * 8 > 2 ** 31
    tail = (0.3 * np.random.RandomState(8).randn(n - cut, 2)).astype(np.float32)
    want = host.resample(tail.astype(np.float64), sr, new)
    first_out = cut // M * L                                        # the output that sits exactly on frame `cut`
    n_out = length(n, sr, new)
    assert first_out + want.shape[0] == n_out and first_out * 8 > 2 ** 31
    # the first tile all of whose taps lie at or behind the cut
    first_tile = -(-(first_out + (W // 2) * L // M + L) // (P * S))
    begin = first_tile * P * S
    assert begin - first_out < 4000 and n_out - begin > 20 * P * S
    sums, out = np.zeros((n_out - begin, 2)), np.full((n_out - begin, 2), np.nan, dtype=np.float32)
    rc = emu.emu_convert_rate(tail.ctypes.data, n, cut, sr, new, 0, first_tile, sums.ctypes.data, out.ctypes.data)
    assert rc == n_out, rc
    rows = np.zeros((L, W))
    row_sum = ctypes.c_double()
    assert old.emu_resample_rows(sr, new, rows.ctypes.data_as(ctypes.c_void_p), ctypes.byref(row_sum)) == 0
    bound = float(np.abs(tail).max()) * (row_sum.value * W * 2.0 ** -53 + W * 2e-15)
    worst = float(np.abs(sums - want[begin - first_out:]).max())
    print(f"{n_out - begin} outputs from {begin}: {worst:.2e} (bound {bound:.2e})")
    assert worst <= bound
    assert np.array_equal(out, sums.astype(np.float32))
    # a tile that would need frames before the cut is refused by the emulation, not read
    assert emu.emu_convert_rate(tail.ctypes.data, n, cut, sr, new, 0, first_out // (P * S) - 1, sums.ctypes.data,
                                out.ctypes.data) == -3


def test_mgx_convert_rate_decides_before_it_touches_the_handle():
    lib = _native.library()
    n_out = ctypes.c_int64(-7)

    def call(n, rate_in, rate_out, out=None, capacity=0):
        return lib.mgx_convert_rate(None, None, n, rate_in, rate_out, out, capacity, ctypes.byref(n_out))

    assert call(1000, 0, 44100) == -1 and call(1000, 48000, -5) == -1                          # MGX_ERR_ARGUMENT
    assert call(1000, 44100, 44100) == -1
    assert call(-1, 44100, 48000) == -1
    assert call(1000, *REFUSED) == _native.ERR_UNSUPPORTED and b"4096" in lib.mgx_last_error()
    assert b"44100 -> 44056" in lib.mgx_last_error()
    assert call(600_000_000, 44100, 48000) == _native.ERR_UNSUPPORTED
    assert call(480_000_000, 44100, 48000) == _native.ERR_UNSUPPORTED                           # 522 M outputs
    assert n_out.value == -7                                                                    # nothing reported so far
    assert call(44100 * 480, 44100, 48000) == 0 and n_out.value == 48000 * 480                  # the length only
    assert call(1, 48000, 44100) == 0 and n_out.value == 0
    somewhere = ctypes.c_void_p(4096)
    assert call(1000, 48000, 44100, somewhere, 918) == -1                                       # somewhere to write: a handle is needed
    assert lib.mgx_convert_rate(None, None, 1000, 48000, 44100, None, 0, None) == -1


def test_delivery_sample_rate_is_validated_at_construction():
    import matchering_amd as mg
    from matchering_amd.delivery import Delivery

    assert Delivery().sample_rate is None and Delivery().rate(44100) == 44100
    assert Delivery(sample_rate=48000).rate(44100) == 48000
    assert Delivery(sample_rate=8000).sample_rate == 8000
    for bad in (7999, 0, -48000, 48000.0, "48000", True):
        with pytest.raises(ValueError, match="sample_rate"):
            Delivery(sample_rate=bad)
    assert Delivery.from_json({"loudness": -14, "sample_rate": 48000}) == Delivery(loudness=-14, sample_rate=48000)
    assert Delivery.from_json({"sample_rate": 96000, "limiter": True, "true_peak": -1.0}).sample_rate == 96000
    with pytest.raises(ValueError, match="sample_rate"):
        Delivery.from_json({"sample_rate": 4000})
    # the refusals of results.py stand with a rate as without
    with pytest.raises(ValueError, match="WAVE"):
        mg.Result("x.aiff", "PCM_16", delivery=Delivery(sample_rate=48000))
    with pytest.raises(ValueError, match="dither"):
        mg.Result("x.wav", "FLOAT", delivery=Delivery(dither="tpdf", sample_rate=48000))
    assert mg.pcm24("x.wav", delivery=Delivery(sample_rate=48000)).delivery.sample_rate == 48000


def test_delivered_names_the_rate_when_it_differs():
    from dataclasses import replace

    from matchering_amd.delivery import Delivery, delivery_gain
    from matchering_amd.loudness import Loudness

    fields = {name: 0 for name in Loudness.__dataclass_fields__}
    measured = Loudness(**{**fields, "integrated": -16.0, "true_peak": 0.5, "sample_rate": 48000})
    record = delivery_gain(Delivery(loudness=-14.0, true_peak=-1.0, sample_rate=48000), 24, measured)
    assert record.sample_rate is None and record.frames is None and " Hz" not in str(record)
    there = replace(record, sample_rate=48000, frames=1000, internal_rate=44100)
    assert str(there).startswith(str(record)) and " at 48000 Hz" in str(there)
    assert " Hz" not in str(replace(record, sample_rate=44100, frames=1000, internal_rate=44100))


def test_a_refused_pair_is_a_value_error_before_anything_else(tmp_path):
    """44100 -> 44056 Hz: ``process``, ``process_batch`` and ``stages.main`` raise ValueError naming both rates and the
    library's reason before a file is opened or a device asked for (the files named here do not exist, and ``main``
    would fail on its arguments)."""
    import matchering_amd as mg
    from matchering_amd import stages
    from matchering_amd.batch import process_batch
    from matchering_amd.delivery import Delivery, DeliveryRequest

    spec = Delivery(true_peak=-1.0, sample_rate=REFUSED[1])
    results = [mg.pcm24(str(tmp_path / "out.wav"), delivery=spec)]
    missing = str(tmp_path / "missing.wav")
    for run in (lambda: mg.process(missing, missing, results),
                lambda: process_batch([{"target": missing, "reference": missing, "results": results}], rank=0, world_size=1),
                lambda: stages.main(np.zeros((10, 2), np.float32), np.zeros((10, 2), np.float32), mg.Config(),
                                    device=object(), deliveries=DeliveryRequest([("k", 0, "PCM_24", spec)]))):
        with pytest.raises(ValueError) as refused:
            run()
        assert "44100" in str(refused.value) and "44056" in str(refused.value) and "4096" in str(refused.value)
    assert not os.listdir(tmp_path)
    # pairs the library takes: the lengths it will make, without a device
    request = DeliveryRequest([("a", 0, "PCM_24", Delivery(sample_rate=48000)), ("b", 1, "FLOAT", Delivery(sample_rate=96000)),
                               ("c", 0, "PCM_16", Delivery(sample_rate=44100)), ("d", 0, "PCM_16", Delivery())])
    assert request.check_rates(44100, 44100 * 3) == {48000: 144000, 96000: 288000}
