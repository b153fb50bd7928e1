"""``ReferenceProfile``: what ``stages.main`` takes from a reference track -- ``final_amplitude_coefficient``
(match_levels.py:29-44), ``reference_match_rms`` (match_levels.py:134-161) and the loud pieces' average spectra of mid
and side (match_frequencies.py:30-42) -- analysed once on the GPU (``mgx_reference_profile``) and kept as a few
kilobytes, so that any number of targets are mastered against it without its audio (``mgx_master_with_profile``).

    profile = ReferenceProfile.analyze("reference.wav", config)
    profile.save("reference.mgxp")
    mg.process("target.wav", "reference.mgxp", [mg.pcm16("out.wav")], config)

The bytes are those of the device block (``mgx_profile_header`` + 2 x (fft_size / 2 + 1) float64, little-endian);
a saved file puts eight bytes of its own magic in front.  A profile belongs to the ``Config`` fields its analysis
depends on (``internal_sample_rate``, ``fft_size``, ``max_piece_size``, ``threshold``, ``min_value``): ``matches``
refuses any other before anything reaches the GPU.
"""

import ctypes
import os
import sys
import threading
import weakref

import numpy as np

from . import _native
from ._native import MgxProfileHeader

FILE_MAGIC = b"MGXPROF1"
HEADER_BYTES = ctypes.sizeof(MgxProfileHeader)
# (name in the header, name in Config): the fields a profile is tied to
CONFIG_FIELDS = ("internal_sample_rate", "fft_size", "max_piece_size", "threshold", "min_value")


def profile_bytes(config):
    """Size of a profile's device block for ``config`` (``mgx_profile_bytes``; needs no GPU)."""
    n = ctypes.c_size_t()
    native = config.to_native()
    _native.check(_native.library().mgx_profile_bytes(ctypes.byref(native), ctypes.byref(n)))
    return n.value


def is_profile_file(path):
    """Whether ``path`` is a saved profile: by the file's first bytes, never by its name."""
    try:
        with open(path, "rb") as fh:
            return fh.read(len(FILE_MAGIC)) == FILE_MAGIC
    except (OSError, TypeError, ValueError):
        return False


class ReferenceProfile:
    """A reference's analysis results on the host; uploaded to a ``Device`` on first use there and kept."""

    def __init__(self, blob):
        if sys.byteorder != "little":
            raise RuntimeError("reference profiles are little-endian; this host is not")
        blob = bytes(blob)
        if len(blob) < HEADER_BYTES:
            raise ValueError(f"not a reference profile: {len(blob)} bytes, a header alone has {HEADER_BYTES}")
        header = MgxProfileHeader.from_buffer_copy(blob[:HEADER_BYTES])
        if header.magic != _native.PROFILE_MAGIC:
            raise ValueError(f"not a reference profile: magic {header.magic:#010x}, expected {_native.PROFILE_MAGIC:#010x}")
        if header.version != _native.PROFILE_VERSION:
            raise ValueError(f"reference profile of layout version {header.version}; this package reads version "
                             f"{_native.PROFILE_VERSION}")
        fft = header.fft_size
        if fft < 8 or fft > 65536 or fft & (fft - 1):
            raise ValueError(f"reference profile with fft_size {fft}: not a power of two in [8, 65536]")
        want = HEADER_BYTES + 2 * (fft // 2 + 1) * 8
        if len(blob) != want:
            raise ValueError(f"reference profile is truncated or padded: {len(blob)} bytes, fft_size {fft} makes {want}")
        self._blob = blob
        self._header = header
        self._resident = weakref.WeakKeyDictionary()       # Device -> DeviceBuffer
        self._lock = threading.Lock()

    # ---- making one ------------------------------------------------------------------------
    @classmethod
    def analyze(cls, reference, config, device=None):
        """Analyse a reference: a path (loaded, checked and brought to the internal rate as ``process`` does with its
        reference, same log codes), an (n, 2) array (float, or integer PCM as a file holds it) or ``DeviceFrames``
        (left alone, not released)."""
        from .device import DeviceFrames, default_device

        dev = device if device is not None else default_device()
        if isinstance(reference, (str, bytes, os.PathLike)):
            frames = _load_reference(reference, config, dev)
            try:
                return cls.analyze(frames, config, dev)
            finally:
                if isinstance(frames, DeviceFrames):
                    frames.release()
        from .stages import _as_frames

        reference = _as_frames(reference, "reference")
        with dev.lock:
            if isinstance(reference, DeviceFrames):
                return cls(dev.reference_profile(reference.buf, reference.frames, config.to_native()))
            buf = dev.upload_frames(reference)
            try:
                return cls(dev.reference_profile(buf, reference.shape[0], config.to_native()))
            finally:
                buf.release()

    # ---- files -----------------------------------------------------------------------------
    def save(self, path):
        with open(path, "wb") as fh:
            fh.write(FILE_MAGIC)
            fh.write(self._blob)

    @classmethod
    def load(cls, path):
        with open(path, "rb") as fh:
            data = fh.read()
        if data[:len(FILE_MAGIC)] != FILE_MAGIC:
            raise ValueError(f"{path!r} is not a saved reference profile (it does not begin with {FILE_MAGIC!r})")
        try:
            return cls(data[len(FILE_MAGIC):])
        except ValueError as exc:
            raise ValueError(f"{path!r}: {exc}") from None

    def tobytes(self):
        """The device block: ``mgx_profile_header`` + spectra."""
        return self._blob

    # ---- what it holds -----------------------------------------------------------------------
    def matches(self, config):
        """True, or ``ValueError`` naming the first Config field this profile was not made with."""
        for name in CONFIG_FIELDS:
            have, want = getattr(self._header, name), getattr(config, name)
            if have != (int(want) if isinstance(have, int) else float(want)):
                raise ValueError(f"the reference profile was made with {name} = {have!r}, this Config has "
                                 f"{name} = {want!r}: analyse the reference again with this Config")
        return True

    internal_sample_rate = property(lambda self: self._header.internal_sample_rate)
    fft_size = property(lambda self: self._header.fft_size)
    max_piece_size = property(lambda self: self._header.max_piece_size)
    threshold = property(lambda self: self._header.threshold)
    min_value = property(lambda self: self._header.min_value)
    frames = property(lambda self: self._header.frames)
    piece = property(lambda self: self._header.piece)
    divisions = property(lambda self: self._header.divisions)
    loud_count = property(lambda self: self._header.loud_count)
    peak = property(lambda self: self._header.peak)
    amplitude_coefficient = property(lambda self: self._header.amplitude_coefficient)
    average_rms = property(lambda self: self._header.average_rms)
    match_rms = property(lambda self: self._header.match_rms)

    @property
    def spectra(self):
        """(2, fft_size / 2 + 1) float64: the loud pieces' average |rfft| / fft_size of mid and side (a copy)."""
        return np.frombuffer(self._blob, dtype="<f8", offset=HEADER_BYTES).reshape(2, -1).copy()

    def __eq__(self, other):
        return isinstance(other, ReferenceProfile) and self._blob == other._blob

    __hash__ = object.__hash__

    def __repr__(self):
        return (f"ReferenceProfile({self.frames} frames at {self.internal_sample_rate} Hz, fft_size {self.fft_size}, "
                f"{self.loud_count} of {self.divisions} pieces loud, match rms {self.match_rms:.6g})")

    # ---- on a device -------------------------------------------------------------------------
    def resident(self, device):
        """This profile's DeviceBuffer on ``device``: uploaded on the first call, the same buffer afterwards."""
        with device.lock:                   # (the device's lock first: callers hold it already, stages.main among them)
            with self._lock:
                buf = self._resident.get(device)
                if buf is None or buf.ptr is None:
                    buf = device.upload(np.frombuffer(self._blob, dtype=np.uint8), dtype=None)
                    self._resident[device] = buf
                return buf


def _load_reference(path, config, dev):
    """``process``'s route for a reference file (core.read_track): ``DeviceFrames`` or a checked host array."""
    from .core import read_track

    temp_folder = config.temp_folder or os.path.dirname(os.path.abspath(os.fspath(path)))
    array, frames = read_track(path, "reference", config, temp_folder, dev)
    return frames if frames is not None else array
