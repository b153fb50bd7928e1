"""Intake: how a file becomes what ``stages.main`` receives (core.py:52-74 of the reference, cut to this package's shape).

A ``Track`` is made in two steps, because ``process_batch`` takes them on different threads:

* ``read`` -- host only: the file is loaded (integer PCM and float32 WAVE mapped, not decoded), ``device.takes_resident``
  decides whether it goes to the GPU as the file holds it, and ``checker.check`` does everything else: limits, log codes,
  and the conversion of the tracks the device does not take;
* ``Track.to_device`` -- under the device's lock: ``Device.track_frames`` decodes the track there and converts it when it is
  mono or off-rate (``mgx_resample``), and the target's peak statistics are taken there (``mgx_peak_count``) for the
  warnings of checker.py:118-130.

``Track.for_main`` is the resident frames where there are some, else the checked array.  ``validate`` is the
``ERROR_VALIDATION`` rule, ``equality_guard`` the guard in front of it.  ``process`` finishes the target before it reads
the reference (``read_single`` / ``read_pair``); ``process_batch`` reads both on a loader thread and finishes them on a lane.
``device.takes_resident``, ``device.final_frames`` and ``Device.track_frames`` are looked up when they are called.
"""

from contextlib import contextmanager

import numpy as np

from .audio_io import load, pcm_channels, unpack24
from .checker import LATER, check, check_equality, count_max_peaks, on_host, peak_warnings
from .log import Code, ModuleError, debug

NO_EQUALITY_CHECK = ("the reference is a profile, not audio: whether it was made from the target itself "
                     "(checker.py:140-142) cannot be checked and is not")


class Track:
    """One loaded and checked file.  ``array``: what ``check`` returned -- the file's own samples, or the track the host
    made of them; ``rate``: ``check``'s; ``file_rate``: the file's; ``resident``: it goes to the GPU as the file holds it;
    ``converts``: the device changes its rate or its channels there, so ``array`` is not the final track; ``final``: the
    final track's frame count; ``host_peaks``: the target's peak statistics are still to be taken, on the host
    (``process_batch`` with a stand-in for the GPU); ``frames``: the ``DeviceFrames`` that ``to_device`` made."""

    def __init__(self, role, array, rate, file_rate, resident, converts, final, host_peaks):
        self.role, self.array, self.rate, self.file_rate = role, array, rate, file_rate
        self.resident, self.converts, self.final, self.host_peaks = resident, converts, final, host_peaks
        self.frames = None

    @property
    def channels(self):
        return 2 if self.converts else pcm_channels(self.array)

    @property
    def for_main(self):
        return self.frames if self.frames is not None else self.array

    def to_device(self, dev, config):
        """The device step (``dev``: None without a GPU); what it made is released when it fails."""
        target = self.role == "target"
        with released_on_error(self):
            if self.resident:
                with dev.lock:
                    self.frames = dev.track_frames(self.array, self.file_rate, config.internal_sample_rate)
                    peaks = dev.peak_count(self.frames, 2 * self.frames.frames) if target else None
            elif self.host_peaks:
                peaks = count_max_peaks(unpack24(self.array) if self.array.dtype == np.uint8 else self.array)
            else:
                return
            if target:
                peak_warnings(peaks, config)

    def release(self):
        if self.frames is not None:
            self.frames.release()
            self.frames = None


@contextmanager
def released_on_error(*tracks):
    """The resident frames of ``tracks`` (anything else among them is passed over) do not outlive an exception."""
    try:
        yield
    except Exception:
        for track in tracks:
            if isinstance(track, Track):
                track.release()
        raise


def _load(path, role, config, temp_folder, gpu):
    """(samples as the file holds them, the file's rate, whether they go to the GPU that way)"""
    audio, rate = load(path, role, temp_folder, pcm=True)        # 16/24/32-bit WAVE: decoded on the GPU
    resident = False
    if gpu:
        from . import device

        resident = device.takes_resident(audio, rate, config.internal_sample_rate)
    return audio, rate, resident


def read(path, role, config, temp_folder, gpu, host_peaks=False):
    """The host step: load and check one file (``gpu``: whether there is one).  ``host_peaks``: without a GPU, a target the
    host has nothing to convert of -- two channels of integers or float32 at the internal rate -- keeps its peak
    statistics for ``to_device``, as a resident one does."""
    internal = config.internal_sample_rate
    audio, rate, resident = _load(path, role, config, temp_folder, gpu)
    changes = rate != internal or pcm_channels(audio) != 2
    converts = resident and changes
    host_peaks = (host_peaks and not gpu and role == "target" and not changes
                  and (audio.dtype.kind in "iu" or audio.dtype == np.float32))
    array, checked_rate = check(audio, rate, config, role, peaks=LATER if resident or host_peaks else None,
                                on_device=converts)
    final = array.shape[0]
    if converts:
        from . import device

        final = device.final_frames(audio, rate, internal)
    return Track(role, array, checked_rate, rate, resident, converts, final, host_peaks)


def file_frames(path, config, temp_folder, dev):
    """A file -> ``DeviceFrames`` at the internal rate by the route of a track, with none of ``check``'s limits and log
    codes (``loudness.measure``); a load error names the target."""
    from .device import DeviceFrames

    audio, rate, resident = _load(path, "target", config, temp_folder, True)
    if resident:
        return dev.track_frames(audio, rate, config.internal_sample_rate)
    audio = on_host(audio, rate, config.internal_sample_rate)
    return DeviceFrames(dev.upload_frames(audio), audio.shape[0])


def validate(config, *tracks):
    """core.py:66-74: every track at the internal rate, in two channels, longer than the FFT."""
    for track in tracks:
        if track.rate != config.internal_sample_rate or track.channels != 2 or track.final <= config.fft_size:
            raise ModuleError(Code.ERROR_VALIDATION)


def no_equality_check(config):
    """A target whose reference is a profile: the equality guard has nothing to compare, and says so."""
    if not config.allow_equality:
        debug(NO_EQUALITY_CHECK)


def guard_needs_frames(target, reference, config):
    """Whether the equality guard has to compare frames that the device converts, so that it can only run behind
    ``to_device``: the Config does not allow equality, a track is converted there, and the final lengths agree."""
    return not config.allow_equality and (target.converts or reference.converts) and target.final == reference.final


def equality_guard(target, reference, config):
    """checker.py:140-142, unless the Config allows equality.  Neither track converted on the device: the host arrays are
    compared; final lengths differ: not equal, nothing is copied; otherwise the converted frames are downloaded."""
    if guard_needs_frames(target, reference, config):
        check_equality(target.array, reference.array, [t.frames if t.converts else None for t in (target, reference)])
    elif not config.allow_equality and not (target.converts or reference.converts):
        check_equality(target.array, reference.array)


def read_single(path, role, config, temp_folder, dev):
    """Both steps for ONE track (its partner is a profile, or it is becoming one), validated."""
    track = read(path, role, config, temp_folder, dev is not None)
    track.to_device(dev, config)
    with released_on_error(track):
        validate(config, track)
    return track


def read_pair(target_path, reference_path, config, temp_folder, dev):
    """``process``'s pair: the target is finished before the reference is read, so its peak warnings come first."""
    target = read(target_path, "target", config, temp_folder, dev is not None)
    target.to_device(dev, config)
    with released_on_error(target):
        reference = read(reference_path, "reference", config, temp_folder, dev is not None)
        reference.to_device(dev, config)
        with released_on_error(reference):
            equality_guard(target, reference, config)
            validate(config, target, reference)
    return target, reference
