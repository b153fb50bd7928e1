"""Audit: the quality-control pass a distributor's intake check makes -- DC offset, runs of samples at the rail, a stereo
image that cancels in mono, dropouts, head and tail silence, samples that are not finite numbers -- over a track, a
rendering or the integer samples of a file as written, while they are in HBM (``mgx_audit``: include/mgx.h has the
definitions, tests/audit_oracle.py the numpy form).  ``checker`` mirrors the reference's checks and ``measure`` gives
loudness and peaks; this answers the rest.

    import matchering_amd as mg
    report = mg.audit("my_song_master.wav")
    print(report)
    for name, value, limit in report.findings():
        print(name, value, limit)
    mg.process(target, reference, results, audit=lambda name, value: print(name, value.findings()))
"""

import dataclasses
import math
import os
from dataclasses import dataclass

import numpy as np

from .config import Config


def _db(value):
    return 20.0 * math.log10(value) if value > 0.0 else -math.inf


@dataclass(frozen=True)
class AuditLimits:
    """What counts as clipping and as silence: a sample is at the rail from ``clip_level`` (linear) up, ``clip_run``
    consecutive ones of a channel are an event; a frame is silent when both samples lie at or under ``silence_db``
    (dBFS; ``-inf``: exact zeros only)."""

    clip_level: float = 1 - 2 ** -15
    clip_run: int = 3
    silence_db: float = -90.0

    def __post_init__(self):
        if not (math.isfinite(self.clip_level) and self.clip_level > 0.0):
            raise ValueError(f"clip_level must be finite and positive, got {self.clip_level}")
        if int(self.clip_run) != self.clip_run or self.clip_run < 1:
            raise ValueError(f"clip_run must be a whole number of samples, at least 1, got {self.clip_run}")
        if math.isnan(self.silence_db) or self.silence_db == math.inf:
            raise ValueError(f"silence_db must be a level in dBFS or -inf, got {self.silence_db}")

    @property
    def silence_level(self):
        """linear"""
        return 0.0 if self.silence_db == -math.inf else 10.0 ** (self.silence_db / 20.0)

    def native(self):
        from ._native import MgxAuditLimits

        return MgxAuditLimits(float(self.clip_level), float(self.silence_level), int(self.clip_run), 0)


@dataclass(frozen=True)
class Audit:
    """What ``mgx_audit`` found.  Per-channel fields are (left, right) tuples; positions and lengths are frames, with
    their times in seconds beside them; levels are linear with their decibel forms beside them.  ``bits``: 0 for float
    frames, else the width of the integer samples that were read."""

    sample_rate: int
    frames: int
    bits: int
    nonfinite: tuple
    clip_events: tuple
    clip_samples: tuple
    clip_longest: tuple
    clip_first: tuple
    head_silence: int
    tail_silence: int
    gap_longest: int
    gap_at: int
    sub_blocks: int
    sub_block_frames: int
    sum: tuple
    sumsq: tuple
    peak: tuple
    sum_lr: float
    dc: tuple
    rms: tuple
    balance_db: float
    correlation: float
    mono_loss_db: float
    correlation_min: float
    correlation_min_at: int

    def _seconds(self, frames):
        return frames / self.sample_rate

    @property
    def duration_s(self):
        return self._seconds(self.frames)

    @property
    def dc_db(self):
        """dBFS of the magnitude of each channel's mean"""
        return tuple(_db(abs(v)) if not math.isnan(v) else math.nan for v in self.dc)

    @property
    def peak_db(self):
        """dBFS"""
        return tuple(_db(v) for v in self.peak)

    @property
    def head_silence_s(self):
        return self._seconds(self.head_silence)

    @property
    def tail_silence_s(self):
        return self._seconds(self.tail_silence)

    @property
    def gap_longest_s(self):
        return self._seconds(self.gap_longest)

    @property
    def gap_at_s(self):
        return None if self.gap_at < 0 else self._seconds(self.gap_at)

    @property
    def clip_first_s(self):
        return tuple(None if at < 0 else self._seconds(at) for at in self.clip_first)

    @property
    def correlation_min_at_s(self):
        return None if self.correlation_min_at < 0 else self._seconds(self.correlation_min_at * self.sub_block_frames)

    def findings(self, dc_db=-60.0, correlation_min=0.0, gap_s=0.05, head_s=None, tail_s=None):
        """What is out of bounds, as ``(name, value, limit)``: "nonfinite" (samples), "clipping" (events), "dc_offset"
        (the larger channel's dBFS above ``dc_db``), "out_of_phase" (the least 3 s correlation under
        ``correlation_min``), "dropout" (the longest inner gap of silence, seconds, above ``gap_s``) and, where asked
        for, "head_silence" / "tail_silence" (seconds above ``head_s`` / ``tail_s``)."""
        found = []
        if sum(self.nonfinite) > 0:
            found.append(("nonfinite", sum(self.nonfinite), 0))
        if sum(self.clip_events) > 0:
            found.append(("clipping", sum(self.clip_events), 0))
        offsets = [v for v in self.dc_db if not math.isnan(v)]
        if offsets and max(offsets) > dc_db:
            found.append(("dc_offset", max(offsets), dc_db))
        if not math.isnan(self.correlation_min) and self.correlation_min < correlation_min:
            found.append(("out_of_phase", self.correlation_min, correlation_min))
        if self.gap_longest_s > gap_s:
            found.append(("dropout", self.gap_longest_s, gap_s))
        if head_s is not None and self.head_silence_s > head_s:
            found.append(("head_silence", self.head_silence_s, head_s))
        if tail_s is not None and self.tail_silence_s > tail_s:
            found.append(("tail_silence", self.tail_silence_s, tail_s))
        return found

    def as_dict(self):
        """The fields as plain Python values (tuples as lists): what a batch job's result carries."""
        return {k: list(v) if isinstance(v, tuple) else v for k, v in dataclasses.asdict(self).items()}

    def __str__(self):
        kind = "float32" if self.bits == 0 else f"{self.bits}-bit PCM"
        return (f"{self.duration_s:.2f} s of {kind} at {self.sample_rate} Hz: peak {self.peak_db[0]:.2f} / {self.peak_db[1]:.2f} dBFS, "
                f"DC {self.dc_db[0]:.1f} / {self.dc_db[1]:.1f} dBFS, {sum(self.nonfinite)} samples not finite\n"
                f"clipping: {self.clip_events[0]} / {self.clip_events[1]} events, longest run {max(self.clip_longest)} samples; "
                f"silence: head {self.head_silence_s:.3f} s, tail {self.tail_silence_s:.3f} s, longest gap {self.gap_longest_s:.3f} s\n"
                f"stereo: balance {self.balance_db:.2f} dB, correlation {self.correlation:.3f} (least over 3 s: "
                f"{self.correlation_min:.3f}), mono loss {self.mono_loss_db:.2f} dB")


def from_report(report, sample_rate):
    pair = lambda field, kind: tuple(kind(v) for v in field)                # noqa: E731
    return Audit(
        int(sample_rate), int(report.frames), int(report.bits), pair(report.nonfinite, int), pair(report.clip_events, int),
        pair(report.clip_samples, int), pair(report.clip_longest, int), pair(report.clip_first, int), int(report.head_silence),
        int(report.tail_silence), int(report.gap_longest), int(report.gap_at), int(report.sub_blocks),
        int(report.sub_block_frames), pair(report.sum, float), pair(report.sumsq, float), pair(report.peak, float),
        float(report.sum_lr), pair(report.dc, float), pair(report.rms, float), float(report.balance_db),
        float(report.correlation), float(report.mono_loss_db), float(report.correlation_min), int(report.correlation_min_at))


def audit(source, sample_rate=None, config: Config = None, device=None, limits: AuditLimits = None):
    """The audit of a file, an array or frames in HBM: the sources ``measure`` takes.

    ``source``: a path -- audited as ``process`` would hear it, at ``config.internal_sample_rate`` after the same
    decoding and conversion; an (n, 2) or (n,) / (n, 1) array at ``sample_rate`` (default: the Config's internal rate)
    -- floats as float32 frames, file PCM (int16, int32, packed 24-bit uint8) as its integer samples, with the matching
    ``bits``; or a ``device.DeviceFrames`` at ``sample_rate``.  A mono source is audited in two equal columns."""
    from .device import DeviceFrames, _both_columns, default_device, pcm_bits

    config = Config() if config is None else config
    dev = device if device is not None else default_device()
    rate = config.internal_sample_rate if sample_rate is None else int(sample_rate)
    if isinstance(source, DeviceFrames):
        with dev.lock:
            return dev.audit(source, source.frames, rate, 0, limits)
    with dev.lock:
        if isinstance(source, (str, bytes, os.PathLike)):
            from .loudness import _path_frames

            frames = _path_frames(os.fspath(source), config, dev)
            try:
                return dev.audit(frames, frames.frames, config.internal_sample_rate, 0, limits)
            finally:
                frames.release()
        array = np.asarray(source)
        if array.ndim == 1:
            array = array[:, None]
        bits = pcm_bits(array)
        columns = array.shape[1] // 3 if bits == 24 and array.ndim == 2 else array.shape[1] if array.ndim == 2 else 0
        if columns not in (1, 2) or (bits == 24 and array.shape[1] % 3):
            raise ValueError(f"audio to audit must have shape (n, 2) or (n,), got {array.shape}")
        if columns == 1:
            array = _both_columns(array)
        buf = dev.upload(array, dtype=None) if bits else dev.upload(array)
        try:
            return dev.audit(buf, array.shape[0], rate, bits, limits)
        finally:
            buf.release()
