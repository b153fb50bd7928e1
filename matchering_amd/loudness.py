"""Loudness metering: ITU-R BS.1770-4 integrated loudness and true peak, EBU Tech 3341 momentary and short-term maxima,
EBU Tech 3342 loudness range -- the figures a delivery specification is written in ("-14 LUFS, -1 dBTP").  The reference
has no meter; here the frames are in HBM anyway and ``mgx_loudness`` reads them once more (include/mgx.h has the
definitions, tests/loudness_oracle.py the numpy form).

    import matchering_amd as mg
    print(mg.measure("my_song_master.wav"))
    mg.process(target, reference, results, loudness=lambda name, value: print(name, value))
"""

import math
import os
from dataclasses import dataclass

import numpy as np

from .config import Config


def _db(value):
    return 20.0 * math.log10(value) if value > 0.0 else -math.inf


@dataclass(frozen=True)
class Loudness:
    """What ``mgx_loudness`` measured.  Loudness in LUFS, the range in LU, the peaks linear (1.0 is full scale) with
    their decibel forms beside them.  A track with no gated block -- silence, less than 400 ms -- has ``-inf`` loudness."""

    integrated: float
    range: float
    momentary_max: float
    short_term_max: float
    true_peak: float
    sample_peak: float
    sample_rate: int
    frames: int
    sub_blocks: int
    sub_block_frames: int

    @property
    def true_peak_db(self):
        """dBTP"""
        return _db(self.true_peak)

    @property
    def sample_peak_db(self):
        """dBFS"""
        return _db(self.sample_peak)

    def __str__(self):
        return (f"{self.integrated:.2f} LUFS integrated, range {self.range:.2f} LU, momentary max {self.momentary_max:.2f}, "
                f"short-term max {self.short_term_max:.2f}, true peak {self.true_peak_db:.2f} dBTP "
                f"(sample peak {self.sample_peak_db:.2f} dBFS)")


def from_report(report, sample_rate, frames):
    return Loudness(report.integrated, report.range, report.momentary_max, report.short_term_max, report.true_peak,
                    report.sample_peak, int(sample_rate), int(frames), int(report.sub_blocks), int(report.sub_block_frames))


def _path_frames(path, config, dev):
    """A file -> ``DeviceFrames`` at the internal rate by ``process``'s own route for a track (``intake.file_frames``)."""
    from . import intake

    return intake.file_frames(path, config, config.temp_folder or os.path.dirname(os.path.abspath(path)), dev)


def measure(source, sample_rate=None, config: Config = None, device=None):
    """The loudness of a file, an array or frames in HBM.

    ``source``: a path -- measured as ``process`` would hear it, at ``config.internal_sample_rate`` after the same
    decoding and conversion; an (n, 2) or (n,) / (n, 1) array of floats or file PCM -- measured at ``sample_rate``
    (default: the Config's internal rate) as it is; or a ``device.DeviceFrames`` at ``sample_rate``."""
    from .device import DeviceFrames, default_device

    config = Config() if config is None else config
    dev = device if device is not None else default_device()
    if isinstance(source, DeviceFrames):
        rate = config.internal_sample_rate if sample_rate is None else int(sample_rate)
        with dev.lock:
            return dev.loudness(source, source.frames, rate)
    with dev.lock:
        if isinstance(source, (str, bytes, os.PathLike)):
            frames, rate = _path_frames(os.fspath(source), config, dev), config.internal_sample_rate
        else:
            array = np.asarray(source)
            if array.ndim == 1:
                array = array[:, None]
            if array.ndim != 2 or (array.dtype != np.uint8 and array.shape[1] not in (1, 2)):
                raise ValueError(f"audio to measure must have shape (n, 2) or (n,), got {array.shape}")
            if array.dtype != np.uint8 and array.shape[1] == 1:
                array = np.repeat(array, repeats=2, axis=1)
            rate = config.internal_sample_rate if sample_rate is None else int(sample_rate)
            frames = DeviceFrames(dev.upload_frames(array), array.shape[0])
        try:
            return dev.loudness(frames, frames.frames, rate)
        finally:
            frames.release()
