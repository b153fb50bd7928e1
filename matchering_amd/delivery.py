"""Delivery renditions: a result written AT a delivery specification -- a loudness target, a true-peak ceiling, dithered
integer PCM -- from the frames ``stages.main`` still holds in HBM.  The reference has none of this (saver.py:27-33 rounds
without dither, and its limiter's ceiling, hyrax.py:78-99, is a sample-peak ceiling).

    import matchering_amd as mg
    mg.process(target, reference, [
        mg.pcm24("streaming.wav", delivery=mg.Delivery(loudness=-14.0, true_peak=-1.0)),
        mg.pcm16("cd.wav", delivery=mg.Delivery(dither="tpdf_hp")),
        mg.pcm24("master.wav"),
    ])

The rendering is measured once (``mgx_loudness``), ``mgx_delivery_gain`` turns the measurement into ONE linear gain -- what
EBU R 128 normalisation is; never an approximation of a limiter -- and ``mgx_deliver`` applies it, dithers, quantises and
packs in one pass.  The ceiling holds for the written file as a BS.1770 meter reads it back: the gain leaves the quantiser
its head-room (include/mgx.h).  Where the ceiling keeps the loudness under the target the
``Delivered`` record says by how much (``shortfall_lu``).

A delivery may carry a ``TruePeakLimiter``: where the ceiling binds -- and only there -- the rendering is first limited by
``mgx_tp_limit``, a true-peak look-ahead limiter of its own (not the mastering limiter), in as many passes as
``mgx_delivery_limit_step`` asks for; the linear policy above is then applied to the limited frames, so the ceiling's proof is
unchanged and ``shortfall_lu`` says what is still missing.

    mg.pcm16("club.wav", delivery=mg.Delivery(loudness=-9.0, true_peak=-1.0, dither="tpdf_hp", limiter=mg.TruePeakLimiter()))

A delivery may name a ``sample_rate``: the rendering is converted to it in HBM (``mgx_convert_rate``) BEFORE all of the
above, which then runs on the converted frames at that rate, so the ceiling holds for the file at the rate it is written
at.

    mg.pcm24("video.wav", delivery=mg.Delivery(loudness=-14.0, true_peak=-1.0, sample_rate=48000))

A 16 or 24-bit delivery may be NOISE-SHAPED: ``dither`` names a preset ("lipshitz5", "wannamaker9": published
error-feedback filters for 44.1 kHz, handed out for file rates of 44.1 to 48 kHz) or is a ``NoiseShaper`` with
coefficients of its own.  The TPDF-dithered quantiser's error is then fed back through that filter
(``mgx_deliver_shaped``), which moves the noise out of the 2-5 kHz region; the gain leaves the larger head-room such a
quantiser needs (``mgx_delivery_gain_shaped``), so the ceiling holds as before.

    mg.pcm16("cd.wav", delivery=mg.Delivery(true_peak=-1.0, dither="wannamaker9"))
"""

import ctypes
import math
import os
from dataclasses import dataclass, field, fields
from functools import lru_cache

from .audio_io import save
from .loudness import Loudness, _db

DITHERS = {None: 0, "tpdf": 1, "tpdf_hp": 2}
SHAPER_PRESETS = {"lipshitz5": 1, "wannamaker9": 2}                  # the ids of mgx_noise_shaper_preset
SHAPER_TAPS_MAX = 16                                                 # MGX_SHAPER_TAPS_MAX
SUBTYPE_BITS = {"PCM_16": 16, "PCM_24": 24, "PCM_32": 32}            # every other subtype is delivered as float32 frames
LIMITED_BY = (None, "loudness", "true_peak")


LOOKAHEAD_MAX = 2048                # frames: TPL_LOOKAHEAD_MAX (csrc/tp_limit_kernel.h)
RELEASE_MAX = 2 ** 22               # frames
PASSES_MAX = 16                     # MGX_LIMIT_PASSES_MAX
RATE_MIN = 8000                     # Hz: the meter's floor (mgx_loudness, include/mgx.h)


@dataclass(frozen=True)
class TruePeakLimiter:
    """The limiter of a delivery whose ceiling binds (``mgx_tp_limit``).  ``lookahead_ms``: the look-ahead, the hold and
    the length of each of the two smoothing box-cars; ``release_ms``: the time constant of the gain's exponential recovery;
    ``max_passes``: the most passes the pre-gain is searched in; ``tolerance_lu``: the shortfall that ends the search."""

    lookahead_ms: float = 1.5
    release_ms: float = 50.0
    max_passes: int = 4
    tolerance_lu: float = 0.1

    def __post_init__(self):
        for name in ("lookahead_ms", "release_ms", "tolerance_lu"):
            value = getattr(self, name)
            if isinstance(value, bool) or not (isinstance(value, (int, float)) and math.isfinite(value)):
                raise ValueError(f"TruePeakLimiter: {name} must be a finite number, got {value!r}")
        if self.lookahead_ms <= 0.0:
            raise ValueError(f"TruePeakLimiter: lookahead_ms must be positive, got {self.lookahead_ms!r}")
        if self.release_ms < 0.0 or self.tolerance_lu < 0.0:
            raise ValueError("TruePeakLimiter: release_ms and tolerance_lu must not be negative")
        if isinstance(self.max_passes, bool) or not (isinstance(self.max_passes, int) and 1 <= self.max_passes <= PASSES_MAX):
            raise ValueError(f"TruePeakLimiter: max_passes must be an integer in [1, {PASSES_MAX}], got {self.max_passes!r}")

    def frames(self, rate):
        """(L, R) at ``rate`` Hz: L = max(1, round(lookahead_ms rate / 1000)) frames, R = release_ms rate / 1000."""
        lookahead = max(1, int(round(self.lookahead_ms * rate / 1000.0)))
        release = self.release_ms * rate / 1000.0
        if lookahead > LOOKAHEAD_MAX:
            raise ValueError(f"TruePeakLimiter: lookahead_ms={self.lookahead_ms!r} is {lookahead} frames at {rate} Hz, "
                             f"more than {LOOKAHEAD_MAX}")
        if release > RELEASE_MAX:
            raise ValueError(f"TruePeakLimiter: release_ms={self.release_ms!r} is more than {RELEASE_MAX} frames at {rate} Hz")
        return lookahead, release

    @classmethod
    def from_json(cls, entry):
        """``true`` for the defaults, or ``{"lookahead_ms": ..., "release_ms": ..., "max_passes": ..., "tolerance_lu": ...}``."""
        if isinstance(entry, cls) or entry is None:
            return entry
        if entry is True:
            return cls()
        if not isinstance(entry, dict):
            raise ValueError(f"a limiter is true or an object with lookahead_ms / release_ms / max_passes / tolerance_lu, got {entry!r}")
        unknown = set(entry) - {f.name for f in fields(cls)}
        if unknown:
            raise ValueError(f"limiter: unknown keys {sorted(unknown)}")
        return cls(**entry)


@dataclass(frozen=True)
class NoiseShaper:
    """The error-feedback filter of a noise-shaped delivery: ``coefficients`` c[1..K], K at most 16, of the noise transfer
    function H(z) = 1 - sum c[k] z^-k (include/mgx.h, ``mgx_noise_shaper``).  ``preset`` is not an argument: it is the
    name of the library's preset on what ``NoiseShaper.lipshitz5()`` / ``.wannamaker9()`` return -- their coefficients come
    from the library's table -- and None on coefficients of one's own, which are taken at any file rate."""

    coefficients: tuple
    preset: str = field(default=None, init=False)

    def __post_init__(self):
        try:
            values = tuple(self.coefficients)
        except TypeError:
            raise ValueError(f"NoiseShaper: coefficients must be a sequence of numbers, got {self.coefficients!r}") from None
        for value in values:
            if isinstance(value, bool) or not (isinstance(value, (int, float)) and math.isfinite(value)):
                raise ValueError(f"NoiseShaper: every coefficient must be a finite number, got {value!r}")
        if len(values) > SHAPER_TAPS_MAX:
            raise ValueError(f"NoiseShaper: at most {SHAPER_TAPS_MAX} coefficients, got {len(values)}")
        object.__setattr__(self, "coefficients", tuple(float(v) for v in values))

    @classmethod
    def lipshitz5(cls):
        """Lipshitz, Vanderkooy, Wannamaker 1991: 5 taps for 44.1 kHz (the library's preset 1)."""
        return preset_shaper("lipshitz5")

    @classmethod
    def wannamaker9(cls):
        """Wannamaker 1992, F-weighted: 9 taps for 44.1 kHz (the library's preset 2)."""
        return preset_shaper("wannamaker9")

    def native(self):
        from ._native import MgxNoiseShaper

        out = MgxNoiseShaper()
        out.taps = len(self.coefficients)
        for k, value in enumerate(self.coefficients):
            out.c[k] = value
        return out

    def __str__(self):
        return self.preset if self.preset is not None else f"noise-shaped, {len(self.coefficients)} taps"


@lru_cache(maxsize=None)
def preset_shaper(name):
    """The ``NoiseShaper`` of the library's preset ``name``, its coefficients read from the library's one table
    (``mgx_noise_shaper_preset``) the first time it is asked for.  Needs no GPU."""
    from . import _native

    out = _native.MgxNoiseShaper()
    _native.check(_native.library().mgx_noise_shaper_preset(SHAPER_PRESETS[name], 44100, ctypes.byref(out)))
    shaper = NoiseShaper(tuple(out.c[:out.taps]))
    object.__setattr__(shaper, "preset", name)
    return shaper


def check_preset_rate(name, rate):
    """``ValueError`` where the library does not hand the preset ``name`` out for a file at ``rate`` Hz
    (``mgx_noise_shaper_preset``).  Needs no GPU."""
    from . import _native

    rc = _native.library().mgx_noise_shaper_preset(SHAPER_PRESETS[name], int(rate), ctypes.byref(_native.MgxNoiseShaper()))
    if rc == _native.ERR_UNSUPPORTED:
        raise ValueError(f"a delivery at {rate} Hz cannot be shaped with '{name}': "
                         + _native.library().mgx_last_error().decode("utf-8", "replace"))
    _native.check(rc)


@dataclass(frozen=True)
class Delivery:
    """What a result is to meet.  ``loudness``: integrated loudness in LUFS, ``true_peak``: the ceiling in dBTP (at most
    0), either may be None; ``dither``: None, "tpdf" or "tpdf_hp" (high-passed TPDF), or noise-shaped TPDF -- "lipshitz5",
    "wannamaker9" or a ``NoiseShaper`` -- for 16 and 24-bit files;
    ``seed``: the dither generator's key -- the same seed writes the same file; ``limiter``: a ``TruePeakLimiter`` to run
    where the ceiling keeps the linear gain under the target (it needs ``true_peak``), None for the linear gain alone;
    ``sample_rate``: the rate of the written file in Hz -- the rendering is converted in HBM (``mgx_convert_rate``)
    before it is measured, so the loudness and the ceiling hold for the file at THAT rate -- None for the Config's
    internal rate."""

    loudness: float = None
    true_peak: float = None
    dither: str = None
    seed: int = 0
    limiter: TruePeakLimiter = None
    sample_rate: int = None

    def __post_init__(self):
        for name in ("loudness", "true_peak"):
            value = getattr(self, name)
            if value is not None and not (isinstance(value, (int, float)) and math.isfinite(value)):
                raise ValueError(f"Delivery: {name} must be a finite number or None, got {value!r}")
        if self.true_peak is not None and self.true_peak > 0.0:
            raise ValueError(f"Delivery: a true-peak ceiling above 0 dBTP would clip, got {self.true_peak!r}")
        if not isinstance(self.dither, NoiseShaper) and not (
                (self.dither is None or isinstance(self.dither, str)) and (self.dither in DITHERS or self.dither in SHAPER_PRESETS)):
            raise ValueError("Delivery: dither must be None, 'tpdf', 'tpdf_hp', 'lipshitz5', 'wannamaker9' or a NoiseShaper, "
                             f"got {self.dither!r}")
        if not (isinstance(self.seed, int) and 0 <= self.seed < 2 ** 64):
            raise ValueError(f"Delivery: seed must be an integer in [0, 2**64), got {self.seed!r}")
        if self.limiter is not None:
            if not isinstance(self.limiter, TruePeakLimiter):
                raise ValueError(f"Delivery: limiter must be a TruePeakLimiter or None, got {self.limiter!r}")
            if self.true_peak is None:
                raise ValueError("Delivery: a limiter needs a true_peak ceiling to hold")
        if self.sample_rate is not None:
            if isinstance(self.sample_rate, bool) or not isinstance(self.sample_rate, int):
                raise ValueError(f"Delivery: sample_rate must be an integer number of Hz or None, got {self.sample_rate!r}")
            if self.sample_rate < RATE_MIN:
                raise ValueError(f"Delivery: sample_rate must be at least {RATE_MIN} Hz, got {self.sample_rate!r}")

    def rate(self, internal_rate):
        """The rate of the written file: ``sample_rate``, or the Config's internal rate where it is None."""
        return int(internal_rate) if self.sample_rate is None else self.sample_rate

    @property
    def shaper(self):
        """The ``NoiseShaper`` of a noise-shaped delivery (a preset's from the library's table), else None."""
        if isinstance(self.dither, NoiseShaper):
            return self.dither
        return preset_shaper(self.dither) if self.dither in SHAPER_PRESETS else None

    @property
    def shaped(self):
        return isinstance(self.dither, NoiseShaper) or self.dither in SHAPER_PRESETS

    def check_shaper_rate(self, internal_rate):
        """``ValueError`` for a preset shaper at a file rate it is not handed out for.  Needs no GPU."""
        shaper = self.shaper
        if shaper is not None and shaper.preset is not None:
            check_preset_rate(shaper.preset, self.rate(internal_rate))

    def check_subtype(self, subtype):
        """The error ``Result`` raises at construction for a width this delivery cannot be written at."""
        if self.dither is not None and subtype not in ("PCM_16", "PCM_24"):
            raise ValueError(f"Delivery: dither is for PCM_16 and PCM_24 results, not {subtype}")

    def native(self, bits):
        from ._native import MgxDelivery

        return MgxDelivery(math.nan if self.loudness is None else float(self.loudness),
                           math.nan if self.true_peak is None else float(self.true_peak), int(bits),
                           1 if self.shaped else DITHERS[self.dither], int(self.seed))     # (a shaper's dither is TPDF)

    @classmethod
    def from_json(cls, entry):
        """``{"loudness": ..., "true_peak": ..., "dither": ..., "seed": ..., "limiter": ..., "sample_rate": ...}`` of a
        batch job (every key optional; ``"limiter"``: ``true`` for ``TruePeakLimiter()``, or an object with its fields;
        ``"dither"``: a name, ``{"coefficients": [...]}`` for a ``NoiseShaper`` of one's own, or such an object itself)."""
        if isinstance(entry, cls):
            return entry
        if not isinstance(entry, dict):
            raise ValueError(f"a delivery is an object with loudness / true_peak / dither / seed / limiter / sample_rate, got {entry!r}")
        unknown = set(entry) - {"loudness", "true_peak", "dither", "seed", "limiter", "sample_rate"}
        if unknown:
            raise ValueError(f"delivery: unknown keys {sorted(unknown)}")
        if isinstance(entry.get("dither"), dict):
            if set(entry["dither"]) != {"coefficients"} or not isinstance(entry["dither"]["coefficients"], list):
                raise ValueError(f"delivery: a dither object is {{\"coefficients\": [...]}}, got {entry['dither']!r}")
            entry = {**entry, "dither": NoiseShaper(tuple(entry["dither"]["coefficients"]))}
        elif isinstance(entry.get("dither"), list):
            raise ValueError(f"delivery: dither is a name or {{\"coefficients\": [...]}}, got {entry['dither']!r}")
        if entry.get("limiter") in (None, False):
            return cls(**{key: value for key, value in entry.items() if key != "limiter"})
        return cls(**{**entry, "limiter": TruePeakLimiter.from_json(entry["limiter"])})


@dataclass(frozen=True)
class Delivered:
    """What became of one delivery: ``mgx_delivery_result``'s fields, the measurement they were derived from and the
    request.  ``achieved_lufs`` / ``achieved_true_peak`` (linear) are predicted from the measurement of the rendering.
    ``sample_rate`` / ``frames``: the rate and length of the written file (None / None from ``delivery_gain`` alone, which
    sees a measurement and no audio); for a delivery at another rate than the internal one ``measured`` is the
    measurement of the CONVERTED rendering at the delivery's rate -- the one the gain was derived from.
    Where the delivery's limiter ran (``limiter_passes`` > 0) ``measured`` is still the rendering's measurement, ``limited``
    the one of the last pass's frames -- which ``gain`` and the achieved values refer to -- ``pre_gain_db`` that pass's
    pre-gain and ``max_reduction_db`` its deepest gain reduction (a negative number of dB)."""

    gain: float
    achieved_lufs: float
    achieved_true_peak: float
    shortfall_lu: float
    limited_by: str                 # None, "loudness" or "true_peak"
    measured: Loudness
    delivery: Delivery
    bits: int
    limiter_passes: int = 0         # 0: the limiter did not run
    pre_gain_db: float = 0.0
    max_reduction_db: float = 0.0
    limited: Loudness = None
    sample_rate: int = None
    frames: int = None
    internal_rate: int = None       # the rate of the rendering it was made from

    @property
    def gain_db(self):
        return _db(self.gain)

    @property
    def achieved_true_peak_db(self):
        """dBTP"""
        return _db(self.achieved_true_peak)

    def __str__(self):
        text = (f"gain {self.gain_db:+.2f} dB: {self.achieved_lufs:.2f} LUFS, true peak {self.achieved_true_peak_db:.2f} dBTP "
                f"({'float32' if self.bits == 0 else f'{self.bits} bit'}"
                f"{'' if self.delivery.dither is None else ', ' + str(self.delivery.dither)})")
        if self.sample_rate is not None and self.sample_rate != self.internal_rate:
            text += f" at {self.sample_rate} Hz"
        if self.limiter_passes > 0:
            text += (f"; limited in {self.limiter_passes} pass{'' if self.limiter_passes == 1 else 'es'}: pre-gain "
                     f"{self.pre_gain_db:+.2f} dB, at most {self.max_reduction_db:.2f} dB of reduction")
        if self.shortfall_lu > 0.0:
            text += f"; the ceiling keeps it {self.shortfall_lu:.2f} LU under the {self.delivery.loudness:g} LUFS target"
        return text


def delivery_gain(delivery: Delivery, bits: int, measured: Loudness) -> Delivered:
    """``mgx_delivery_gain`` (host only, needs no GPU): the gain that brings a rendering measured as ``measured`` to
    ``delivery`` at ``bits`` (0: float32); ``mgx_delivery_gain_shaped`` for a noise-shaped delivery."""
    from . import _native

    report = _native.MgxLoudnessReport()
    report.integrated, report.true_peak = measured.integrated, measured.true_peak
    out = _native.MgxDeliveryResult()
    shaper = delivery.shaper
    if shaper is None:
        _native.check(_native.library().mgx_delivery_gain(ctypes.byref(delivery.native(bits)), ctypes.byref(report),
                                                          ctypes.byref(out)))
    else:
        _native.check(_native.library().mgx_delivery_gain_shaped(ctypes.byref(delivery.native(bits)), ctypes.byref(shaper.native()),
                                                                 ctypes.byref(report), ctypes.byref(out)))
    return Delivered(out.gain, out.achieved_lufs, out.achieved_true_peak, out.shortfall_lu, LIMITED_BY[out.limited_by],
                     measured, delivery, int(bits))


def _report(measured):
    from . import _native

    report = _native.MgxLoudnessReport()
    report.integrated, report.true_peak = measured.integrated, measured.true_peak
    return report


def limit_step(delivery: Delivery, bits: int, measured: Loudness, pre_gains_db=(), integrated=()):
    """``mgx_delivery_limit_step`` (host only, needs no GPU; ``mgx_delivery_limit_step_shaped`` for a noise-shaped
    delivery): ``(run, pre_gain_db, ceiling)`` after the passes whose pre-gains (dB) and integrated loudness are given --
    none yet: whether the limiter is needed at all."""
    from . import _native

    if delivery.limiter is None:
        raise ValueError("limit_step: the delivery carries no limiter")
    passes = len(pre_gains_db)
    if len(integrated) != passes:
        raise ValueError("limit_step: one integrated loudness per pass")
    array = ctypes.c_double * max(passes, 1)
    plan = _native.MgxDeliveryLimitPlan()
    rest = (ctypes.byref(_report(measured)), passes, array(*map(float, pre_gains_db)), array(*map(float, integrated)),
            int(delivery.limiter.max_passes), float(delivery.limiter.tolerance_lu), ctypes.byref(plan))
    shaper = delivery.shaper
    if shaper is None:
        _native.check(_native.library().mgx_delivery_limit_step(ctypes.byref(delivery.native(bits)), *rest))
    else:
        _native.check(_native.library().mgx_delivery_limit_step_shaped(ctypes.byref(delivery.native(bits)),
                                                                       ctypes.byref(shaper.native()), *rest))
    return bool(plan.run), plan.pre_gain_db, plan.ceiling


RENDERINGS = ("result", "result_no_limiter", "result_no_limiter_normalized")


class DeliveryRequest:
    """What ``stages.main(..., deliveries=request)`` needs to cut the deliveries on the device, and where it leaves them
    (the pattern of ``preview.PreviewRequest``).  ``items``: (key, rendering, subtype, Delivery) each -- ``rendering`` 0
    the limited result, 1 the unlimited one, 2 the unlimited one normalised, as in ``main``'s triple; ``subtype`` a file
    subtype: PCM_16 / PCM_24 / PCM_32 come back as the integer samples of such a file, everything else as float32
    frames.  After ``main``: ``arrays[key]`` the host array, ``delivered[key]`` the ``Delivered`` record."""

    def __init__(self, items=()):
        self.items = []
        self.arrays, self.delivered = {}, {}
        for key, rendering, subtype, delivery in items:
            self.add(key, rendering, subtype, delivery)

    def add(self, key, rendering, subtype, delivery):
        if rendering not in (0, 1, 2):
            raise ValueError(f"DeliveryRequest: rendering must be 0, 1 or 2, got {rendering!r}")
        if not isinstance(delivery, Delivery):
            raise TypeError(f"DeliveryRequest: expected a Delivery, got {delivery!r}")
        delivery.check_subtype(subtype)
        if any(key == k for k, *_ in self.items):
            raise ValueError(f"DeliveryRequest: {key!r} is delivered twice")
        self.items.append((key, int(rendering), subtype, delivery))

    @classmethod
    def for_results(cls, results):
        """The request of ``process``: one item per Result that carries a delivery, keyed by its file."""
        request = cls()
        for item in results:
            if getattr(item, "delivery", None) is not None:
                request.add(item.file, rendering_of(item), item.subtype, item.delivery)
        return request

    def check_rates(self, internal_rate, frames=0):
        """``{rate: frames of a rendering of ``frames`` frames converted to it}`` for every delivery rate other than
        ``internal_rate``; ``ValueError`` naming both rates and the library's reason for a pair ``mgx_convert_rate``
        refuses, or a preset noise shaper and the file rate ``mgx_noise_shaper_preset`` does not hand it out for.  Needs
        no GPU (the entry points' device-free forms): ``process`` calls it before any audio is loaded."""
        from .device import delivery_length

        lengths = {}
        for _, _, _, delivery in self.items:
            delivery.check_shaper_rate(internal_rate)
            rate = delivery.rate(internal_rate)
            if rate != internal_rate and rate not in lengths:
                lengths[rate] = delivery_length(frames, internal_rate, rate)
        return lengths

    def needs(self):
        """Which of ``main``'s three renderings the items are cut from."""
        return tuple(any(r == slot for _, r, _, _ in self.items) for slot in range(3))

    def __bool__(self):
        return bool(self.items)


def rendering_of(item):
    """The rendering a ``Result`` is made from (core.py:99-108)."""
    return 0 if item.use_limiter else (2 if item.normalize else 1)


def plain_results(results):
    """The results that take the ordinary route: no delivery."""
    return [item for item in results if getattr(item, "delivery", None) is None]


def file_encoding(item):
    """The integer subtype of one WAVE file (quantised on the GPU, ``mgx_pcm_encode``), or None (float frames, host
    codec: saver.py:27-33)."""
    if item is None or os.path.splitext(item.file)[1][1:].upper() not in ("WAV", "WAVE"):
        return None
    return item.subtype if item.subtype in SUBTYPE_BITS else None


def renderings_wanted(results):
    """(needs, encodings) of ``stages.main`` for a list of results.  ``needs``: which of its three outputs the files need
    (core.py:77-86); ``encodings``: per output the PCM subtype the GPU can quantise to directly -- every file made from
    that rendering is a WAVE file of one and the same integer subtype -- else None.  Results with a delivery are cut
    from the renderings in HBM and come back in the ``DeliveryRequest``: they take no part in either."""
    wanted = [set(), set(), set()]
    for item in plain_results(results):
        wanted[rendering_of(item)].add(file_encoding(item))
    return tuple(bool(w) for w in wanted), tuple(next(iter(w)) if len(w) == 1 else None for w in wanted)


def write_results(results, renderings, sample_rate, deliveries=None):
    """One file per Result, each from the rendering it asked for (core.py:95-108); a Result with a delivery from the
    array ``stages.main`` left in the ``DeliveryRequest``, at its delivery's own rate."""
    for item in plain_results(results):
        save(item.file, renderings[rendering_of(item)], sample_rate, item.subtype)
    if deliveries:
        write_deliveries(results, deliveries, sample_rate)


def write_deliveries(results, request, sample_rate):
    """One file per Result that carries a delivery, from the arrays ``stages.main`` left in ``request``, each at its own
    rate (``sample_rate``: the internal one, for the deliveries that name none); one log line each: gain, achieved LUFS
    and dBTP, and the shortfall where the ceiling bound the loudness."""
    from .log import debug

    for item in results:
        if getattr(item, "delivery", None) is None:
            continue
        debug(f"delivery '{item.file}': {request.delivered[item.file]}")
        save(item.file, request.arrays[item.file], item.delivery.rate(sample_rate), item.subtype)
