"""Clip repair: the short flat tops of a target that was clipped, rebuilt in HBM before it is mastered (``mgx_declip``:
include/mgx.h has the definition, tests/declip_oracle.py the numpy form).  The reference warns that the target is
clipping and asks for an unclipped mix; most users have none.  Opt-in: nothing is repaired unless it is asked for.

    import matchering_amd as mg
    frames, found = mg.repair_clipping("my_song.wav")
    print(found.describe())
    mg.process(target, reference, results, repair=mg.ClipRepair())
    mg.process(target, reference, results, repair=(lambda name, found: print(name, found.describe()), mg.ClipRepair()))
"""

import dataclasses
import math
import os
from dataclasses import dataclass, fields

import numpy as np

from .config import Config


@dataclass(frozen=True)
class ClipRepair:
    """What counts as clipped and how far a repair may go.  A sample is at the rail from ``level`` (linear) up; with
    ``level=None`` the level is the track's own peak lowered by ``relative_db`` (<= 0), so that a clipped file that was
    attenuated afterwards is still found, and both rails of integer PCM.  Runs of ``min_run`` to ``max_run`` samples are
    rebuilt (at most 512; beyond some 32 samples at 44.1 kHz nothing recovers them); a rebuilt sample stays within
    ``max_rise_db`` of the level."""

    level: float = None
    relative_db: float = -0.1
    min_run: int = 2
    max_run: int = 32
    max_rise_db: float = 6.0

    @classmethod
    def from_json(cls, entry):
        """``true`` (the defaults) or ``{"level": ..., "relative_db": ..., "min_run": ..., "max_run": ...,
        "max_rise_db": ...}`` of a batch job, every key optional; None stays None and ``false`` is None: no repair (a
        job's way out of a batch-wide ``repair=``)."""
        if isinstance(entry, cls) or entry is None:
            return entry
        if entry is False:
            return None
        if entry is True:
            return cls()
        if not isinstance(entry, dict):
            raise ValueError(f"a repair is true or an object with level / relative_db / min_run / max_run / max_rise_db, got {entry!r}")
        unknown = set(entry) - {f.name for f in fields(cls)}
        if unknown:
            raise ValueError(f"repair: unknown keys {sorted(unknown)}")
        return cls(**entry)

    def level_for(self, peak):
        """The level this repair takes on a track whose largest magnitude is ``peak``."""
        return float(self.level) if self.level is not None else float(peak) * 10.0 ** (float(self.relative_db) / 20.0)

    def native(self, peak=1.0):
        from ._native import MgxDeclipParams

        return MgxDeclipParams(self.level_for(peak), 10.0 ** (float(self.max_rise_db) / 20.0), int(self.min_run), int(self.max_run))

    def check(self):
        """``ValueError`` for what ``mgx_declip_check`` refuses, in its words; needs no GPU."""
        from ._native import library

        for name in ("min_run", "max_run"):
            value = getattr(self, name)
            if isinstance(value, bool) or int(value) != value:
                raise ValueError(f"{name}: a whole number of samples, got {value!r}")
        for name in ("relative_db", "max_rise_db"):
            if not isinstance(getattr(self, name), (int, float)) or isinstance(getattr(self, name), bool):
                raise ValueError(f"{name}: a number of decibels, got {getattr(self, name)!r}")
        if self.level is None and not (math.isfinite(self.relative_db) and self.relative_db <= 0.0):
            raise ValueError(f"relative_db: must be finite and at most 0 (the level lies at or under the peak), got {self.relative_db}")
        if self.level is not None and (isinstance(self.level, bool) or not isinstance(self.level, (int, float))):
            raise ValueError(f"level: a linear level, got {self.level!r}")
        lib = library()
        try:
            params = self.native()
        except OverflowError:
            raise ValueError(f"max_rise: must be finite and at least 1, got {self.max_rise_db} dB") from None
        if lib.mgx_declip_check(params) != 0:
            raise ValueError(lib.mgx_last_error().decode("utf-8", "replace"))
        return self


@dataclass(frozen=True)
class Repaired:
    """What ``mgx_declip`` did.  Per-channel fields are (left, right) tuples; lengths and positions are frames.
    ``level``: the linear level that counted as the rail (0.0: the track's peak was 0 and nothing was looked at)."""

    level: float
    frames: int
    runs_repaired: tuple = (0, 0)
    samples_repaired: tuple = (0, 0)
    samples_raised: tuple = (0, 0)
    longest_repaired: tuple = (0, 0)
    first_repaired: tuple = (-1, -1)
    runs_short: tuple = (0, 0)
    runs_long: tuple = (0, 0)
    runs_edge: tuple = (0, 0)
    peak_before: tuple = (0.0, 0.0)
    peak_after: tuple = (0.0, 0.0)

    def as_dict(self):
        """The fields as plain Python values (tuples as lists): what a batch job's result carries."""
        return {k: list(v) if isinstance(v, tuple) else v for k, v in dataclasses.asdict(self).items()}

    def describe(self):
        """One line for the log."""
        from .utils import to_db

        if self.level <= 0.0:
            return "clip repair: the track is silent, nothing to repair"
        left = sum(self.runs_short) + sum(self.runs_long) + sum(self.runs_edge)
        return (f"clip repair at {to_db(self.level)}: {sum(self.runs_repaired)} runs ({sum(self.samples_repaired)} samples, "
                f"longest {max(self.longest_repaired)}) rebuilt, {sum(self.samples_raised)} samples raised, peak "
                f"{to_db(max(self.peak_before))} -> {to_db(max(self.peak_after))}; left alone: {left} runs "
                f"({sum(self.runs_short)} short, {sum(self.runs_long)} long, {sum(self.runs_edge)} at an edge)")


def from_report(report, level, frames):
    pair = lambda field, kind: tuple(kind(v) for v in field)                # noqa: E731
    return Repaired(float(level), int(frames), pair(report.runs_repaired, int), pair(report.samples_repaired, int),
                    pair(report.samples_raised, int), pair(report.longest_repaired, int), pair(report.first_repaired, int),
                    pair(report.runs_short, int), pair(report.runs_long, int), pair(report.runs_edge, int),
                    pair(report.peak_before, float), pair(report.peak_after, float))


def as_repair(repair):
    """``repair=`` as ``process`` and ``stages.main`` take it -- None, a ``ClipRepair``, its JSON (``True`` or an object)
    or a pair (callable, any of these) -- as (callable or None, ClipRepair or None), checked."""
    handler = None
    if isinstance(repair, tuple):
        handler, repair = repair
        if not callable(handler):
            raise ValueError(f"repair: a pair is (callable, ClipRepair), got {handler!r} first")
    repair = ClipRepair.from_json(repair)
    if repair is None:
        if handler is not None:
            raise ValueError("repair: a pair is (callable, ClipRepair), got no ClipRepair")
        return None, None
    return handler, repair.check()


def queue(dev, buf, frames, repair):
    """Queue the repair of (frames, 2) float32 in HBM: (the new DeviceBuffer or None, level).  With an explicit level
    nothing waits; ``level=None`` reads the track's peak first (``Device.peak_count``).  None where the track has no
    frames or its peak is 0: there is nothing to repair, and the caller goes on with the buffer it has.  The report is
    ``finish``'s, wherever the caller waits."""
    if frames == 0:
        return None, 0.0
    peak = 1.0
    if repair.level is None:
        peak, _ = dev.peak_count(buf, frames * 2)
        if not peak > 0.0:
            return None, 0.0
    params = repair.native(peak)
    out, _ = dev.declip(buf, frames, params, report=False)
    return out, params.level


def finish(dev, out, level, frames):
    """The ``Repaired`` of what ``queue`` queued last on this device."""
    if out is None:
        return Repaired(float(level), int(frames))
    return from_report(dev.declip_report(), level, frames)


def repair_clipping(source, repair: ClipRepair = None, sample_rate=None, config: Config = None, device=None):
    """The repaired frames of a file or an array, and what was done: ``((n, 2) float32 array, Repaired)``.

    ``source``: a path -- repaired as ``process`` would hear it, at ``config.internal_sample_rate`` after the same
    decoding and conversion; an (n, 2) or (n,) / (n, 1) array of floats or file PCM; or a ``device.DeviceFrames``, which
    is neither written nor released.  A mono source is repaired in two equal columns."""
    from .device import DeviceFrames, default_device

    _, repair = as_repair(ClipRepair() if repair is None else repair)
    config = Config() if config is None else config
    dev = device if device is not None else default_device()
    with dev.lock:
        owned = True
        if isinstance(source, DeviceFrames):
            frames, owned = source, False
        elif isinstance(source, (str, bytes, os.PathLike)):
            from .loudness import _path_frames

            frames = _path_frames(os.fspath(source), config, dev)
        else:
            array = np.asarray(source)
            if array.ndim == 1:
                array = array[:, None]
            if array.ndim != 2 or (array.dtype != np.uint8 and array.shape[1] not in (1, 2)):
                raise ValueError(f"audio to repair must have shape (n, 2) or (n,), got {array.shape}")
            if array.dtype != np.uint8 and array.shape[1] == 1:
                array = np.repeat(array, repeats=2, axis=1)
            frames = DeviceFrames(dev.upload_frames(array), array.shape[0])
        out = None
        try:
            n = frames.frames
            out, level = queue(dev, frames.buf, n, repair)
            host = np.array(dev.download(out if out is not None else frames.buf, (n, 2)))
            return host, finish(dev, out, level, n)
        finally:
            if out is not None:
                out.release()
            if owned:
                frames.release()
