"""Matching EQ controls: how much of the matching curve is applied, how far it may boost and cut, and the phase of the
FIR (include/mgx.h, ``mgx_eq_shape``) -- and its tone controls: which part of the spectrum is matched, an amount of its
own for the side channel, mono bass, a tilt and up to eight bells and shelves on top of the match (``mgx_eq_tone``).  The
reference has none of this: ``get_fir`` (match_frequencies.py:78-101) turns the whole smoothed curve into one linear-phase
FIR, and that is what ``eq=None`` and ``MatchingEq()`` still give.
"""

import ctypes
import math
from dataclasses import asdict, dataclass, fields

import numpy as np

from ._native import EQ_BANDS_MAX, MgxEqBand, MgxEqShape, MgxEqTone, MgxError, check, library

PHASES = {"linear": 0, "minimum": 1}
BAND_KINDS = {"bell": 0, "low_shelf": 1, "high_shelf": 2}
BAND_CHANNELS = {"mid": 1, "side": 2, "both": 3}


def _number(value):
    return not isinstance(value, bool) and isinstance(value, (int, float)) and math.isfinite(value)


@dataclass(frozen=True)
class ToneBand:
    """One manual trim on top of the match: ``kind`` "bell", "low_shelf" or "high_shelf"; ``hz`` its centre or corner;
    ``gain_db`` in [-24, 24]; ``q`` in [0.1, 20] (a shelf's steepness); ``channels`` "mid", "side" or "both"."""

    kind: str
    hz: float
    gain_db: float
    q: float = 0.7071
    channels: str = "both"

    def __post_init__(self):
        if self.kind not in BAND_KINDS:
            raise ValueError(f"ToneBand: kind must be one of {sorted(BAND_KINDS)}, got {self.kind!r}")
        if not _number(self.hz) or self.hz <= 0.0:
            raise ValueError(f"ToneBand: hz must be a positive number, got {self.hz!r}")
        if not _number(self.gain_db) or not -24.0 <= self.gain_db <= 24.0:
            raise ValueError(f"ToneBand: gain_db must be a number in [-24, 24], got {self.gain_db!r}")
        if not _number(self.q) or not 0.1 <= self.q <= 20.0:
            raise ValueError(f"ToneBand: q must be a number in [0.1, 20], got {self.q!r}")
        if self.channels not in BAND_CHANNELS:
            raise ValueError(f"ToneBand: channels must be one of {sorted(BAND_CHANNELS)}, got {self.channels!r}")

    @classmethod
    def from_json(cls, entry):
        if isinstance(entry, cls):
            return entry
        if not isinstance(entry, dict):
            raise ValueError(f"a band is an object with kind / hz / gain_db / q / channels, got {entry!r}")
        unknown = set(entry) - {f.name for f in fields(cls)}
        if unknown:
            raise ValueError(f"band: unknown keys {sorted(unknown)}")
        missing = {"kind", "hz", "gain_db"} - set(entry)
        if missing:
            raise ValueError(f"band: missing keys {sorted(missing)}")
        return cls(**entry)

    def to_native(self):
        return MgxEqBand(BAND_KINDS[self.kind], BAND_CHANNELS[self.channels], float(self.hz), float(self.gain_db),
                         float(self.q))


def _hz(value):
    return f"{value / 1000.0:g} kHz" if value >= 1000.0 else f"{value:g} Hz"


def _signed(value):
    return f"{'−' if value < 0 else '+'}{abs(value):g}"


@dataclass(frozen=True)
class MatchingEq:
    """``amount``: the share of the matching curve, in dB, that is applied -- 1.0 all of it, 0.5 "match 50 %", 0 none, up
    to 2; ``max_boost_db`` / ``max_cut_db``: caps on what the shaped curve may boost and cut (not negative), None for no
    cap; ``phase``: "linear" (the reference's FIR, symmetric, pre-ringing) or "minimum" (the same magnitude response with
    nothing before the main tap, time-aligned with the linear-phase master).  Level matching is untouched.

    The tone controls (include/mgx.h, ``mgx_eq_tone``): ``match_range`` ``(low, high)`` in Hz, either None for open --
    outside it the target's own spectrum is left alone, over raised-cosine edges ``range_octaves`` wide; ``side_amount``:
    an amount of its own for the side channel (0: match the tone, keep the stereo image), None for ``amount``;
    ``mono_below_hz``: the side channel removed below this frequency, over an edge ``mono_octaves`` wide;
    ``tilt_db_per_octave`` around ``tilt_pivot_hz`` and ``bands`` (up to eight ``ToneBand``): trims on top of the match,
    which the caps do not bound.  With none of them set the object is the one without them."""

    amount: float = 1.0
    max_boost_db: float = None
    max_cut_db: float = None
    phase: str = "linear"
    match_range: tuple = None
    range_octaves: float = 1.0
    side_amount: float = None
    mono_below_hz: float = None
    mono_octaves: float = 1.0
    tilt_db_per_octave: float = 0.0
    tilt_pivot_hz: float = 1000.0
    bands: tuple = ()

    def __post_init__(self):
        number = _number
        if not number(self.amount) or not 0.0 <= self.amount <= 2.0:
            raise ValueError(f"MatchingEq: amount must be a number in [0, 2], got {self.amount!r}")
        for name in ("max_boost_db", "max_cut_db"):
            value = getattr(self, name)
            if value is not None and (not number(value) or value < 0.0):
                raise ValueError(f"MatchingEq: {name} must be None or a number that is not negative, got {value!r}")
        if self.phase not in PHASES:
            raise ValueError(f"MatchingEq: phase must be one of {sorted(PHASES)}, got {self.phase!r}")
        # ---- the tone controls (what depends on the sample rate is ``check``'s)
        if self.match_range is not None:
            if not isinstance(self.match_range, (tuple, list)) or len(self.match_range) != 2:
                raise ValueError(f"MatchingEq: match_range must be None or (low, high), got {self.match_range!r}")
            low, high = self.match_range
            for value in (low, high):
                if value is not None and (not number(value) or value <= 0.0):
                    raise ValueError(f"MatchingEq: match_range holds positive numbers or None, got {self.match_range!r}")
            if low is not None and high is not None and not low < high:
                raise ValueError(f"MatchingEq: match_range must be (low, high) with low < high, got {self.match_range!r}")
            object.__setattr__(self, "match_range", None if low is None and high is None else (low, high))
        for name in ("range_octaves", "mono_octaves"):
            value = getattr(self, name)
            if not number(value) or not 0.0 <= value <= 4.0:
                raise ValueError(f"MatchingEq: {name} must be a number in [0, 4], got {value!r}")
        if self.side_amount is not None and (not number(self.side_amount) or not 0.0 <= self.side_amount <= 2.0):
            raise ValueError(f"MatchingEq: side_amount must be None or a number in [0, 2], got {self.side_amount!r}")
        if self.mono_below_hz is not None and (not number(self.mono_below_hz) or self.mono_below_hz <= 0.0):
            raise ValueError(f"MatchingEq: mono_below_hz must be None or a positive number, got {self.mono_below_hz!r}")
        if not number(self.tilt_db_per_octave) or not -6.0 <= self.tilt_db_per_octave <= 6.0:
            raise ValueError(f"MatchingEq: tilt_db_per_octave must be a number in [-6, 6], got {self.tilt_db_per_octave!r}")
        if not number(self.tilt_pivot_hz) or self.tilt_pivot_hz <= 0.0:
            raise ValueError(f"MatchingEq: tilt_pivot_hz must be a positive number, got {self.tilt_pivot_hz!r}")
        if isinstance(self.bands, (str, bytes, dict)) or not hasattr(self.bands, "__iter__"):
            raise ValueError(f"MatchingEq: bands must be a sequence of ToneBand, got {self.bands!r}")
        bands = tuple(self.bands)
        if not all(isinstance(band, ToneBand) for band in bands):
            raise ValueError(f"MatchingEq: bands must be a sequence of ToneBand, got {self.bands!r}")
        if len(bands) > EQ_BANDS_MAX:
            raise ValueError(f"MatchingEq: at most {EQ_BANDS_MAX} bands, got {len(bands)}")
        object.__setattr__(self, "bands", bands)

    @classmethod
    def from_json(cls, entry):
        """``{"amount": ..., "max_boost_db": ..., "max_cut_db": ..., "phase": ..., "match_range": [low, high], ...,
        "bands": [{"kind": ..., "hz": ..., "gain_db": ...}, ...]}`` of a batch job, every key optional."""
        if isinstance(entry, cls) or entry is None:
            return entry
        if not isinstance(entry, dict):
            raise ValueError(f"an eq is an object with amount / max_boost_db / max_cut_db / phase and the tone controls, "
                             f"got {entry!r}")
        unknown = set(entry) - {f.name for f in fields(cls)}
        if unknown:
            raise ValueError(f"eq: unknown keys {sorted(unknown)}")
        entry = dict(entry)
        if "bands" in entry:
            if not isinstance(entry["bands"], (list, tuple)):
                raise ValueError(f"eq: bands is a list of objects, got {entry['bands']!r}")
            entry["bands"] = tuple(ToneBand.from_json(band) for band in entry["bands"])
        if isinstance(entry.get("match_range"), list):
            entry["match_range"] = tuple(entry["match_range"])
        return cls(**entry)

    def to_json(self):
        """The object ``from_json`` takes back: plain numbers, strings, lists and None."""
        out = asdict(self)
        out["match_range"] = None if self.match_range is None else list(self.match_range)
        out["bands"] = [asdict(band) for band in self.bands]
        return out

    @property
    def is_default(self):
        """Nothing to apply: the call is the one without an ``eq``."""
        return self == MatchingEq()

    @property
    def has_tone(self):
        """A tone control is set: the design runs the tone stage (``mgx_master_eq``)."""
        return (self.match_range is not None or self.side_amount is not None or self.mono_below_hz is not None
                or self.tilt_db_per_octave != 0.0 or bool(self.bands))

    def to_native(self):
        """The ``mgx_eq_shape`` of this object (NaN: no cap)."""
        nan = float("nan")
        return MgxEqShape(float(self.amount), nan if self.max_boost_db is None else float(self.max_boost_db),
                          nan if self.max_cut_db is None else float(self.max_cut_db), PHASES[self.phase], 0)

    def _tone(self):
        def value(v):
            return float("nan") if v is None else float(v)

        low, high = self.match_range or (None, None)
        tone = MgxEqTone(value(low), value(high), float(self.range_octaves), value(self.side_amount),
                         value(self.mono_below_hz), float(self.mono_octaves), float(self.tilt_db_per_octave),
                         float(self.tilt_pivot_hz), len(self.bands), 0)
        for i, band in enumerate(self.bands):
            tone.bands[i] = band.to_native()
        return tone

    def tone_native(self):
        """The ``mgx_eq_tone`` of this object, None where no tone control is set (the call without a tone)."""
        return self._tone() if self.has_tone else None

    def check(self, config):
        """``mgx_eq_tone_check`` against a ``Config``: ValueError, with the library's message, for what it refuses (a
        minimum-phase EQ at an ``fft_size`` the device chain does not run, a frequency beyond half the sample rate).
        Needs no GPU."""
        try:
            check(library().mgx_eq_tone_check(ctypes.byref(config.to_native()), ctypes.byref(self.to_native()),
                                              ctypes.byref(self._tone())))
        except MgxError as exc:
            raise ValueError(f"MatchingEq: {exc}") from None

    def curves(self, config):
        """What a front end plots, from ``mgx_eq_tone_curve``: ``{"hz": f_k, "mid": {...}, "side": {...}}`` with, per
        channel, ``weight`` (the amount times the matching range's weight), ``trim_db`` (tilt and bands) and ``gate``
        (mono bass), each ``fft_size / 2 + 1`` float64 values.  Needs no GPU."""
        native = config.to_native()
        bins = config.fft_size // 2 + 1
        as_p = ctypes.POINTER(ctypes.c_double)
        out = {"hz": np.arange(bins) * float(native.internal_sample_rate) / config.fft_size}
        for channel, name in enumerate(("mid", "side")):
            terms = {key: np.zeros(bins) for key in ("weight", "trim_db", "gate")}
            try:
                check(library().mgx_eq_tone_curve(ctypes.byref(native), ctypes.byref(self.to_native()),
                                                  ctypes.byref(self._tone()), channel,
                                                  *(terms[key].ctypes.data_as(as_p) for key in ("weight", "trim_db", "gate"))))
            except MgxError as exc:
                raise ValueError(f"MatchingEq: {exc}") from None
            out[name] = terms
        return out

    def describe(self):
        """What the FIR stage's log line says: ``matching EQ: 50 %, +6/−6 dB, minimum phase``, and behind it the tone
        controls that are set: ``…, 60 Hz – 12 kHz, side 0 %, mono below 120 Hz, tilt −0.5 dB/oct, 2 bands``."""
        def cap(value, sign):
            return "no cap" if value is None else f"{sign}{value:g}"

        caps = "no caps" if self.max_boost_db is None and self.max_cut_db is None else \
            f"{cap(self.max_boost_db, '+')}/{cap(self.max_cut_db, '−')} dB"
        parts = [f"matching EQ: {100.0 * self.amount:g} %, {caps}, {self.phase} phase"]
        if self.match_range is not None:
            low, high = self.match_range
            parts.append(f"from {_hz(low)}" if high is None else f"up to {_hz(high)}" if low is None
                         else f"{_hz(low)} – {_hz(high)}")
        if self.side_amount is not None:
            parts.append(f"side {100.0 * self.side_amount:g} %")
        if self.mono_below_hz is not None:
            parts.append(f"mono below {_hz(self.mono_below_hz)}")
        if self.tilt_db_per_octave != 0.0:
            parts.append(f"tilt {_signed(self.tilt_db_per_octave)} dB/oct")
        if self.bands:
            parts.append(f"{len(self.bands)} band{'s' if len(self.bands) != 1 else ''}")
        return ", ".join(parts)


def as_eq(eq):
    """None, a ``MatchingEq`` or the JSON object of one -> None or a ``MatchingEq``."""
    return MatchingEq.from_json(eq)
