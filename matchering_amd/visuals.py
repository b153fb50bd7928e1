"""Visuals: the pictures a mastering front end shows beside the numbers -- a waveform overview and a spectrogram of a
track, a rendering or the reference, computed from the frames while they are in HBM (``mgx_overview``,
``mgx_spectrogram``; include/mgx.h has the definitions, tests/visuals_oracle.py the numpy form).  The reference has
nothing of the kind; what comes back is a few hundred kilobytes instead of every frame.

    import matchering_amd as mg
    mg.spectrogram("my_song.wav", columns=1024, bands=mg.visuals.log_bands(4096, 44100, 96)).save_png("before.png")
    mg.process(target, reference, results, visuals=lambda name, v: v.spectrogram.save_png(name + ".png"))
"""

import ctypes
import math
import os
import struct
import zlib
from dataclasses import dataclass

import numpy as np

from . import _native
from .config import Config


def log_bands(fft_size, sample_rate, bands, f_lo=20.0, f_hi=None):
    """Band edges (bin indices, int32) for a spectrogram of ``fft_size`` points at ``sample_rate`` Hz: ``bands + 1``
    edges spaced logarithmically from ``f_lo`` to ``f_hi`` (default: Nyquist), the last one ``fft_size // 2 + 1`` where
    ``f_hi`` is Nyquist so that the top band holds the Nyquist bin.  Edges are forced strictly ascending, so the low
    bands, where several logarithmic edges fall on one bin, come out one bin wide each and push the following edges
    up; edges pushed past the last bin are dropped.  The table therefore holds HOWEVER MANY BANDS THAT LEAVES -- at
    most ``bands``, fewer when ``bands`` exceeds the bins between ``f_lo`` and ``f_hi``: read ``len(edges) - 1``."""
    fft_size, bands = int(fft_size), int(bands)
    half = fft_size // 2
    nyquist = sample_rate / 2.0
    f_hi = nyquist if f_hi is None else float(f_hi)
    if bands < 1 or not (0.0 < f_lo < f_hi <= nyquist):
        raise ValueError(f"log_bands: need bands >= 1 and 0 < f_lo < f_hi <= {nyquist:g} Hz")
    top = half + 1 if f_hi >= nyquist else min(half + 1, int(math.ceil(f_hi * fft_size / sample_rate)))
    freqs = f_lo * (f_hi / f_lo) ** (np.arange(bands + 1) / bands)
    raw = np.floor(freqs * fft_size / sample_rate + 0.5).astype(np.int64)
    raw[-1] = top
    edges = [int(max(raw[0], 0))]
    for e in raw[1:]:
        nxt = max(int(e), edges[-1] + 1)
        if nxt > top:
            break
        edges.append(nxt)
    if len(edges) < 2:
        raise ValueError("log_bands: no bin between f_lo and f_hi")
    edges[-1] = top                                               # (the last band always reaches f_hi)
    return np.asarray(edges, dtype=np.int32)


def linear_bands(fft_size):
    """The identity table: every bin 0 .. fft_size / 2 its own band."""
    return np.arange(int(fft_size) // 2 + 2, dtype=np.int32)


@dataclass(frozen=True)
class VisualsRequest:
    """The sizes of the pictures ``visuals=`` makes: overview columns; transform length, hop, columns (0: one per hop)
    of the spectrogram, its bands (a count of logarithmic bands from 20 Hz, or a table of bin edges; None: every bin)
    and channels ("lr" or "ms")."""

    overview_columns: int = 2048
    fft_size: int = 4096
    hop: int = 1024
    columns: int = 1024
    bands: object = 96
    channels: str = "lr"

    @classmethod
    def from_json(cls, item):
        if item is True or item is None:
            return cls()
        given = dict(item)
        if isinstance(given.get("bands"), list):
            given["bands"] = np.asarray(given["bands"], dtype=np.int32)
        return cls(**given)

    def edges(self, sample_rate):
        return _edges(self.bands, self.fft_size, sample_rate)


def _edges(bands, fft_size, sample_rate):
    if bands is None:
        return linear_bands(fft_size)
    if isinstance(bands, (int, np.integer)):
        return log_bands(fft_size, sample_rate, int(bands))
    edges = np.ascontiguousarray(bands, dtype=np.int32)
    if edges.ndim != 1 or edges.size < 2:
        raise ValueError("bands: a count, None or a table of at least two bin edges")
    return edges


def _log2_exact(fft_size):
    fft_size = int(fft_size)
    if fft_size < 1 or fft_size & (fft_size - 1):
        raise ValueError(f"fft_size: {fft_size} is not a power of two")
    return fft_size.bit_length() - 1


def spec_of(fft_size, hop, columns, channels, edges):
    """The ``mgx_spectrogram_spec`` of a request."""
    if channels not in ("lr", "ms"):
        raise ValueError(f"channels: {channels!r} is neither 'lr' nor 'ms'")
    return _native.MgxSpectrogramSpec(_log2_exact(fft_size), int(hop), int(columns), 1 if channels == "ms" else 0,
                                      int(len(edges) - 1))


def plan(frames, fft_size=4096, hop=1024, columns=0, bands=None, channels="lr", sample_rate=44100):
    """(hops, columns) of a spectrogram of ``frames`` frames, or ``ValueError`` with the library's reason: what
    ``mgx_spectrogram_plan`` settles from the numbers alone.  Needs no GPU."""
    edges = _edges(bands, fft_size, sample_rate)
    spec = spec_of(fft_size, hop, columns, channels, edges)
    hops, cols = ctypes.c_int64(), ctypes.c_int32()
    lib = _native.library()
    rc = lib.mgx_spectrogram_plan(int(frames), ctypes.byref(spec), edges.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                  ctypes.byref(hops), ctypes.byref(cols))
    if rc != 0:
        raise ValueError("spectrogram: " + lib.mgx_last_error().decode("utf-8", "replace"))
    return hops.value, cols.value


def _db10(power, floor_db):
    floor = 10.0 ** (floor_db / 10.0)
    return 10.0 * np.log10(np.maximum(np.asarray(power, dtype=np.float64), floor))


@dataclass(frozen=True)
class Overview:
    """``mgx_overview``: per column and channel the smallest and the largest sample and the sum of squares.
    ``lo`` / ``hi``: (columns, 2) float32; ``sumsq``: (columns, 2) float64; ``frames_per_column``: (columns,)."""

    sample_rate: int
    frames: int
    lo: np.ndarray
    hi: np.ndarray
    sumsq: np.ndarray

    @property
    def columns(self):
        return int(self.lo.shape[0])

    @property
    def frames_per_column(self):
        w = self.columns
        c = np.arange(w + 1, dtype=np.int64)
        return np.diff(c * self.frames // w) if w else np.zeros(0, dtype=np.int64)

    @property
    def rms(self):
        return np.sqrt(self.sumsq / np.maximum(self.frames_per_column, 1)[:, None])

    def rms_db(self, floor_db=-120.0):
        """dBFS of the RMS: 10 log10 of the mean square, not below ``floor_db``."""
        return _db10(self.sumsq / np.maximum(self.frames_per_column, 1)[:, None], floor_db)

    def as_dict(self):
        return {"sample_rate": self.sample_rate, "frames": self.frames, "columns": self.columns,
                "frames_per_column": self.frames_per_column.tolist(), "lo": self.lo.tolist(), "hi": self.hi.tolist(),
                "rms": self.rms.tolist()}


@dataclass(frozen=True)
class Spectrogram:
    """``mgx_spectrogram``: linear power, (columns, 2, bands) float32; a full-scale sine on a bin centre reads 1.0."""

    sample_rate: int
    frames: int
    fft_size: int
    hop: int
    hops: int
    channels: str
    edges: np.ndarray
    power: np.ndarray

    @property
    def columns(self):
        return int(self.power.shape[0])

    def db(self, floor_db=-120.0):
        return _db10(self.power, floor_db)

    @property
    def times_s(self):
        """The centre of every column in seconds: the mean of its hops' centres."""
        w, t = self.columns, self.hops
        c = np.arange(w + 1, dtype=np.int64)
        first, last = (c[:-1] * t // w), (c[1:] * t // w)
        return (first + last - 1) * 0.5 * self.hop / self.sample_rate if w else np.zeros(0)

    @property
    def band_hz(self):
        """(bands, 2): the frequencies of every band's first bin and of the bin behind its last."""
        e = self.edges.astype(np.float64) * self.sample_rate / self.fft_size
        return np.stack([e[:-1], e[1:]], axis=1)

    def image(self, top_db=0.0, range_db=96.0, channel=None):
        """uint8 (bands, columns) -- or (2 * bands, columns), the first channel above the second, where ``channel`` is
        None -- with the high frequencies at the top: 255 at ``top_db`` and above, 0 at ``top_db - range_db`` and below."""
        db = self.db(top_db - range_db - 1.0)
        picked = [0, 1] if channel is None else [int(channel)]
        rows = [np.flipud(db[:, ch, :].T) for ch in picked]
        scaled = (np.concatenate(rows, axis=0) - (top_db - range_db)) * (255.0 / range_db)
        return np.clip(np.floor(scaled + 0.5), 0, 255).astype(np.uint8)

    def save_png(self, path, top_db=0.0, range_db=96.0, channel=None):
        """``image`` as an 8-bit greyscale PNG (standard library only)."""
        write_png(path, self.image(top_db, range_db, channel))

    def as_dict(self):
        return {"sample_rate": self.sample_rate, "frames": self.frames, "fft_size": self.fft_size, "hop": self.hop,
                "hops": self.hops, "channels": self.channels, "edges": self.edges.tolist(), "power": self.power.tolist()}


@dataclass(frozen=True)
class Visuals:
    """Both pictures of one track or rendering."""

    overview: Overview
    spectrogram: Spectrogram

    def as_dict(self):
        return {"overview": self.overview.as_dict(), "spectrogram": self.spectrogram.as_dict()}


def write_png(path, image):
    """(rows, columns) uint8 -> an 8-bit greyscale PNG."""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    if image.ndim != 2 or image.size == 0:
        raise ValueError(f"a greyscale picture has shape (rows, columns), got {image.shape}")
    rows, columns = image.shape

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    raw = np.concatenate([np.zeros((rows, 1), dtype=np.uint8), image], axis=1).tobytes()      # filter 0 on every row
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", columns, rows, 8, 0, 0, 0, 0))
                 + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def make(dev, buf, frames, rate, request):
    """Both pictures of (frames, 2) float32 in HBM on ``dev`` by a ``VisualsRequest`` (a track shorter than the request's
    columns gets as many as it has frames or hops)."""
    request = VisualsRequest() if request is None else request
    edges = request.edges(rate)
    hops = (frames - 1) // request.hop + 1 if frames > 0 else 0
    return Visuals(dev.overview(buf, frames, rate, max(1, min(request.overview_columns, frames, 65536))),
                   dev.spectrogram(buf, frames, rate, request.fft_size, request.hop, min(request.columns, hops), edges,
                                   request.channels))


def handler_of(visuals):
    """``visuals=`` as ``process`` and ``stages.main`` take it -- a callable (the default sizes) or a pair (callable,
    VisualsRequest) -- as (callable, VisualsRequest)."""
    if isinstance(visuals, tuple):
        return visuals[0], visuals[1]
    return visuals, VisualsRequest()


def _frames_of(source, sample_rate, config, dev):
    """source -> (DeviceFrames, rate, owned)."""
    from .device import DeviceFrames

    rate = config.internal_sample_rate if sample_rate is None else int(sample_rate)
    if isinstance(source, DeviceFrames):
        return source, rate, False
    if isinstance(source, (str, bytes, os.PathLike)):
        from .loudness import _path_frames

        return _path_frames(os.fspath(source), config, dev), config.internal_sample_rate, True
    array = np.asarray(source)
    if array.ndim == 1:
        array = array[:, None]
    if array.ndim != 2 or (array.dtype != np.uint8 and array.shape[1] not in (1, 2)):
        raise ValueError(f"audio to draw must have shape (n, 2) or (n,), got {array.shape}")
    if array.dtype != np.uint8 and array.shape[1] == 1:
        array = np.repeat(array, repeats=2, axis=1)
    return DeviceFrames(dev.upload_frames(array), array.shape[0]), rate, True


def overview(source, columns=2048, sample_rate=None, config: Config = None, device=None):
    """The waveform overview of a file, an array or frames in HBM -- the sources ``measure`` and ``audit`` take; a mono
    source goes in two equal columns.  ``columns``: at most the frames of the track and 65536."""
    from .device import default_device

    config = Config() if config is None else config
    dev = device if device is not None else default_device()
    with dev.lock:
        frames, rate, owned = _frames_of(source, sample_rate, config, dev)
        try:
            return dev.overview(frames, frames.frames, rate, columns)
        finally:
            if owned:
                frames.release()


def spectrogram(source, fft_size=4096, hop=1024, columns=0, bands=None, channels="lr", sample_rate=None,
                config: Config = None, device=None):
    """The spectrogram of a file, an array or frames in HBM.  ``columns``: 0 for one per hop, 1 for the long-term
    average spectrum; ``bands``: None for every bin, a count of logarithmic bands from 20 Hz (``log_bands``) or a table
    of bin edges; ``channels``: "lr" or "ms".  What the library refuses is a ValueError before a file is read."""
    from .device import DeviceFrames, default_device

    config = Config() if config is None else config
    is_path = isinstance(source, (str, bytes, os.PathLike))
    rate = config.internal_sample_rate if sample_rate is None or is_path else int(sample_rate)
    edges = _edges(bands, fft_size, rate)
    # (a file's length is not known yet: with no frames the plan checks everything but the columns against the hops)
    known = 0 if is_path else source.frames if isinstance(source, DeviceFrames) else np.asarray(source).shape[0]
    plan(known, fft_size, hop, columns, edges, channels, rate)
    dev = device if device is not None else default_device()
    with dev.lock:
        frames, rate, owned = _frames_of(source, sample_rate, config, dev)
        try:
            return dev.spectrogram(frames, frames.frames, rate, fft_size, hop, columns, edges, channels)
        finally:
            if owned:
                frames.release()
