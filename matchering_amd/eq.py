"""Matching EQ controls: how much of the matching curve is applied, how far it may boost and cut, and the phase of the
FIR (include/mgx.h, ``mgx_eq_shape``).  The reference has none of this: ``get_fir`` (match_frequencies.py:78-101) turns
the whole smoothed curve into one linear-phase FIR, and that is what ``eq=None`` and ``MatchingEq()`` still give.
"""

import ctypes
import math
from dataclasses import dataclass, fields

from ._native import MgxEqShape, MgxError, check, library

PHASES = {"linear": 0, "minimum": 1}


@dataclass(frozen=True)
class MatchingEq:
    """``amount``: the share of the matching curve, in dB, that is applied -- 1.0 all of it, 0.5 "match 50 %", 0 none, up
    to 2; ``max_boost_db`` / ``max_cut_db``: caps on what the shaped curve may boost and cut (not negative), None for no
    cap; ``phase``: "linear" (the reference's FIR, symmetric, pre-ringing) or "minimum" (the same magnitude response with
    nothing before the main tap, time-aligned with the linear-phase master).  Level matching is untouched."""

    amount: float = 1.0
    max_boost_db: float = None
    max_cut_db: float = None
    phase: str = "linear"

    def __post_init__(self):
        def number(value):
            return not isinstance(value, bool) and isinstance(value, (int, float)) and math.isfinite(value)

        if not number(self.amount) or not 0.0 <= self.amount <= 2.0:
            raise ValueError(f"MatchingEq: amount must be a number in [0, 2], got {self.amount!r}")
        for name in ("max_boost_db", "max_cut_db"):
            value = getattr(self, name)
            if value is not None and (not number(value) or value < 0.0):
                raise ValueError(f"MatchingEq: {name} must be None or a number that is not negative, got {value!r}")
        if self.phase not in PHASES:
            raise ValueError(f"MatchingEq: phase must be one of {sorted(PHASES)}, got {self.phase!r}")

    @classmethod
    def from_json(cls, entry):
        """``{"amount": ..., "max_boost_db": ..., "max_cut_db": ..., "phase": ...}`` of a batch job, every key optional."""
        if isinstance(entry, cls) or entry is None:
            return entry
        if not isinstance(entry, dict):
            raise ValueError(f"an eq is an object with amount / max_boost_db / max_cut_db / phase, got {entry!r}")
        unknown = set(entry) - {f.name for f in fields(cls)}
        if unknown:
            raise ValueError(f"eq: unknown keys {sorted(unknown)}")
        return cls(**entry)

    @property
    def is_default(self):
        """Nothing to apply: the call is the one without an ``eq``."""
        return self == MatchingEq()

    def to_native(self):
        """The ``mgx_eq_shape`` of this object (NaN: no cap)."""
        nan = float("nan")
        return MgxEqShape(float(self.amount), nan if self.max_boost_db is None else float(self.max_boost_db),
                          nan if self.max_cut_db is None else float(self.max_cut_db), PHASES[self.phase], 0)

    def check(self, config):
        """``mgx_eq_shape_check`` against a ``Config``: ValueError, with the library's message, for what it refuses (a
        minimum-phase EQ at an ``fft_size`` the device chain does not run).  Needs no GPU."""
        try:
            check(library().mgx_eq_shape_check(ctypes.byref(config.to_native()), ctypes.byref(self.to_native())))
        except MgxError as exc:
            raise ValueError(f"MatchingEq: {exc}") from None

    def describe(self):
        """What the FIR stage's log line says: ``matching EQ: 50 %, +6/-6 dB, minimum phase``."""
        def cap(value, sign):
            return "no cap" if value is None else f"{sign}{value:g}"

        caps = "no caps" if self.max_boost_db is None and self.max_cut_db is None else \
            f"{cap(self.max_boost_db, '+')}/{cap(self.max_cut_db, '−')} dB"
        return f"matching EQ: {100.0 * self.amount:g} %, {caps}, {self.phase} phase"


def as_eq(eq):
    """None, a ``MatchingEq`` or the JSON object of one -> None or a ``MatchingEq``."""
    return MatchingEq.from_json(eq)
