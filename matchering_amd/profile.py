"""``ReferenceProfile``: what ``stages.main`` takes from a reference track -- ``final_amplitude_coefficient``
(match_levels.py:29-44), ``reference_match_rms`` (match_levels.py:134-161) and the loud pieces' average spectra of mid
and side (match_frequencies.py:30-42) -- analysed once on the GPU (``mgx_reference_profile``) and kept as a few
kilobytes, so that any number of targets are mastered against it without its audio (``mgx_master_with_profile``).

    profile = ReferenceProfile.analyze("reference.wav", config)
    profile.save("reference.mgxp")
    mg.process("target.wav", "reference.mgxp", [mg.pcm16("out.wav")], config)

Several references make one profile too -- "master this to the sound of these five records": every source is analysed
on its own as above, and ``ReferenceProfile.merge`` pools their loud pieces (``mgx_profile_merge``); a list or tuple
in a reference's place (``analyze``, ``process``, a job's "references") means exactly that.

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
MAX_WEIGHT = 65536          # of one source of a merge (include/mgx.h, mgx_profile_merge)


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


def is_reference_set(reference):
    """Whether ``reference`` names a SET of references: a list or tuple whose elements are paths (audio files or saved
    profiles), ``ReferenceProfile``s, ``DeviceFrames`` or (n, channels) arrays.  Anything else -- nested lists of
    numbers among them -- is what it was before there were sets: one track."""
    from .device import DeviceFrames

    if not isinstance(reference, (list, tuple)):
        return False
    return all(isinstance(item, (str, bytes, os.PathLike, ReferenceProfile, DeviceFrames))
               or (isinstance(item, np.ndarray) and item.ndim == 2) for item in reference)


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
        (left alone, not released).  A SET of references (``is_reference_set``: a list or tuple of any of these, of
        ``ReferenceProfile``s and of saved profiles' paths) becomes one profile: each element is made into a profile as
        above -- a profile must have been made with this Config, ``matches`` -- and the lot is merged (``merge``)."""
        from .device import DeviceFrames, default_device

        if is_reference_set(reference):
            profiles = []
            for item in reference:
                if isinstance(item, (str, bytes, os.PathLike)) and is_profile_file(item):
                    item = cls.load(item)
                if isinstance(item, ReferenceProfile):
                    item.matches(config)
                    profiles.append(item)
                else:
                    profiles.append(cls.analyze(item, config, device))
            return cls.merge(profiles, device=device)
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

    @classmethod
    def merge(cls, profiles, weights=None, device=None):
        """One profile out of several: the reference's own means (match_levels.py:62-71, match_frequencies.py:30-42)
        over the UNION of the sources' loud pieces -- every source stays what its own analysis made of it, so saved
        profiles merge without anybody's audio.  ``weights``: positive integers up to 65536, "count this reference w
        times" (default 1 each).  The sources must share the five Config fields a profile is tied to; the first that
        differs from source 0 is a ``ValueError`` naming the field and its position, before anything reaches a device.
        The result is an ordinary profile (include/mgx.h, ``mgx_profile_merge``, has the formulas) and may be merged
        again; one source with weight 1 comes back byte for byte.  More than 64 sources are merged in groups of up to
        64 and the group results merged again: that regroups the float64 sums, so the result may differ from a
        single merge's in the last bits (the integer fields are the same)."""
        profiles = list(profiles)
        if not profiles:
            raise ValueError("merge: the list of reference profiles is empty")
        for i, item in enumerate(profiles):
            if not isinstance(item, ReferenceProfile):
                raise TypeError(f"merge: source {i} is {type(item).__name__}, not a ReferenceProfile")
        weights = [1] * len(profiles) if weights is None else list(weights)
        if len(weights) != len(profiles):
            raise ValueError(f"merge: {len(profiles)} profiles but {len(weights)} weights")
        for i, w in enumerate(weights):
            if isinstance(w, bool) or not isinstance(w, (int, np.integer)) or not 1 <= w <= MAX_WEIGHT:
                raise ValueError(f"merge: weight {w!r} of source {i} is not a positive integer up to {MAX_WEIGHT}")
        weights = [int(w) for w in weights]
        first = profiles[0]
        for i, item in enumerate(profiles[1:], 1):
            for name in CONFIG_FIELDS:
                have, want = getattr(item._header, name), getattr(first._header, name)
                if have != want:
                    raise ValueError(f"merge: source {i} was made with {name} = {have!r}, source 0 with {name} = {want!r}: "
                                     f"profiles merge only among those made with the same Config")
        for name in ("loud_count", "divisions"):
            if sum(w * getattr(item, name) for w, item in zip(weights, profiles)) > 2 ** 31 - 1:
                raise ValueError(f"merge: the merged {name} does not fit the profile's 32-bit field")
        from .device import default_device

        dev = device if device is not None else default_device()
        native = first._native_config()
        with dev.lock:
            while len(profiles) > _native.PROFILE_MERGE_MAX:
                groups = range(0, len(profiles), _native.PROFILE_MERGE_MAX)
                profiles = [cls(dev.profile_merge([p.resident(dev) for p in profiles[g:g + _native.PROFILE_MERGE_MAX]],
                                                  weights[g:g + _native.PROFILE_MERGE_MAX], native)) for g in groups]
                weights = [1] * len(profiles)
            return cls(dev.profile_merge([p.resident(dev) for p in profiles], weights, native))

    def _native_config(self):
        """An ``mgx_config`` with the five fields this profile was made with (the others at their defaults)."""
        native = _native.MgxConfig()
        _native.check(_native.library().mgx_config_default(ctypes.byref(native)))
        for name in CONFIG_FIELDS:
            setattr(native, name, getattr(self._header, name))
        return native

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
    """``process``'s route for a reference file (``intake``): ``DeviceFrames`` or a checked host array."""
    from . import intake

    temp_folder = config.temp_folder or os.path.dirname(os.path.abspath(os.fspath(path)))
    return intake.read_single(path, "reference", config, temp_folder, dev).for_main
