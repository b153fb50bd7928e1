"""Device-side plumbing for the Python host: one ``Device`` = one ``mgx_handle``
(one MI355X, one HIP stream).  Buffers are plain HBM allocations addressed by
integer pointers; numpy arrays cross the PCIe boundary only in ``upload`` /
``download``.  No PyTorch: the north star keeps the host a thin ctypes caller.
"""

import bisect
import ctypes
import threading
import weakref
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _native
from ._native import MgxError, MgxReport, check, library
from .audio_io import pcm_channels


class _PinnedPool:
    """Page-locked host blocks (``mgx_host_alloc``), recycled by size class.

    ``empty(shape, dtype)`` returns a numpy array living in such a block; when the array (and every
    view of it) is garbage collected the block goes back to the free list instead of to the OS --
    page-locking 170 MB costs milliseconds, about as much as the copy it is meant to speed up.  Arrays
    handed out here are recognised by ``Device.upload`` / ``download`` (``holds``), which then move them
    with asynchronous DMA instead of a staged copy."""

    KEEP = 8                                   # free blocks kept per size class
    MAX_FREE_BYTES = 4 << 30                   # ... and in total: above 16 MiB every track length is its own size
                                               # class, so a long batch of varied tracks would otherwise pile up
                                               # page-locked memory without bound

    def __init__(self):
        self.lock = threading.Lock()
        self.free = {}                         # size class -> [address, ...]
        self.free_bytes = 0
        self.order = []                        # (size, address) of the free blocks, oldest first
        self.starts, self.ends = [], []        # live blocks, sorted by address

    def empty(self, shape, dtype=np.float32):
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        size = _size_class(max(nbytes, 1))
        with self.lock:
            stack = self.free.get(size)
            address = stack.pop() if stack else None
            if address is not None:
                self.free_bytes -= size
                self.order.remove((size, address))
        if address is None:
            ptr = ctypes.c_void_p()
            check(library().mgx_host_alloc(size, ctypes.byref(ptr)))
            address = ptr.value
            with self.lock:
                i = bisect.bisect_left(self.starts, address)
                self.starts.insert(i, address)
                self.ends.insert(i, address + size)
        raw = (ctypes.c_char * size).from_address(address)
        array = np.frombuffer(raw, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        weakref.finalize(raw, self._give_back, address, size)
        return array

    def _give_back(self, address, size):
        doomed = []
        with self.lock:
            stack = self.free.setdefault(size, [])
            if len(stack) < self.KEEP and size <= self.MAX_FREE_BYTES:
                stack.append(address)
                self.order.append((size, address))
                self.free_bytes += size
                while self.free_bytes > self.MAX_FREE_BYTES:          # trim the blocks that have waited longest
                    old_size, old_address = self.order.pop(0)
                    self.free[old_size].remove(old_address)
                    self.free_bytes -= old_size
                    doomed.append(old_address)
            else:
                doomed.append(address)
            for a in doomed:
                i = bisect.bisect_left(self.starts, a)
                del self.starts[i], self.ends[i]
        for a in doomed:
            try:
                library().mgx_host_free(ctypes.c_void_p(a))
            except Exception:
                pass

    def trim(self):
        """Give every free block back to the OS (``process_batch`` calls this when it is done)."""
        with self.lock:
            doomed = [a for _, a in self.order]
            self.order, self.free, self.free_bytes = [], {}, 0
            for a in doomed:
                i = bisect.bisect_left(self.starts, a)
                del self.starts[i], self.ends[i]
        for a in doomed:
            try:
                library().mgx_host_free(ctypes.c_void_p(a))
            except Exception:
                pass

    def holds(self, array):
        """True when ``array``'s bytes lie inside one of this pool's blocks."""
        first = array.ctypes.data
        with self.lock:
            i = bisect.bisect_right(self.starts, first) - 1
            return i >= 0 and first + array.nbytes <= self.ends[i]


pinned = _PinnedPool()
_copiers = ThreadPoolExecutor(max_workers=4, thread_name_prefix="mgx-stage")
_STAGE_CHUNK = 8 << 20


def _size_class(nbytes):
    """Allocation sizes: powers of two up to 16 MiB, multiples of 16 MiB above."""
    size = 1 << 16
    while size < nbytes:
        size <<= 1
    return size if size <= (1 << 24) else -(-nbytes // (1 << 24)) * (1 << 24)


def pcm_bits(array):
    """Width of the integer PCM samples an array holds (16, 24, 32), 0 for a float array."""
    if array.dtype == np.int16:
        return 16
    if array.dtype == np.int32:
        return 32
    if array.dtype == np.uint8:
        return 24
    return 0


class DeviceFrames:
    """(frames, 2) float32 audio resident in HBM: what ``stages.main`` accepts in place of a numpy array when
    the caller has uploaded (and looked at) a track already -- ``core.process`` does, for the checks."""

    def __init__(self, buf, frames):
        self.buf, self.frames = buf, int(frames)

    @property
    def shape(self):
        return (self.frames, 2)

    def release(self):
        self.buf.release()

    def host(self):
        """The frames as a float32 (frames, 2) array (pinned): ``checker.check_equality`` of a converted track."""
        dev = self.buf.device
        with dev.lock:
            return dev.download(self.buf, (self.frames, 2))


def converted_length(frames, channels, rate_in, rate_out):
    """Frames ``mgx_resample`` makes of a track, ``int(frames * (rate_out / rate_in))``, or None when the library
    leaves this conversion to the host (``MGX_ERR_UNSUPPORTED``: more than 4096 phases, ...).  Needs no GPU."""
    from .log import debug

    n_out = ctypes.c_int64()
    rc = library().mgx_resample(None, None, int(frames), int(channels), int(rate_in), int(rate_out), None, 0,
                                ctypes.byref(n_out))
    if rc == _native.ERR_UNSUPPORTED:
        debug(f"{rate_in} Hz -> {rate_out} Hz is converted on the host: "
              + library().mgx_last_error().decode("utf-8", "replace"))
        return None
    check(rc)
    return n_out.value


def delivery_length(frames, rate_in, rate_out):
    """Frames ``mgx_convert_rate`` makes of a rendering for a delivery at ``rate_out``; ``ValueError`` naming both rates
    and the library's reason for a pair it refuses (a delivery has no host route to fall back to).  Needs no GPU."""
    n_out = ctypes.c_int64()
    rc = library().mgx_convert_rate(None, None, int(frames), int(rate_in), int(rate_out), None, 0, ctypes.byref(n_out))
    if rc == _native.ERR_UNSUPPORTED:
        raise ValueError(f"a delivery at {rate_out} Hz cannot be made from {rate_in} Hz: "
                         + library().mgx_last_error().decode("utf-8", "replace"))
    check(rc)
    return n_out.value


def takes_resident(audio, rate, internal_rate):
    """Whether a loaded track goes to the GPU as its file holds it, to become (frames, 2) float32 at the internal
    rate there (``Device.track_frames``): one or two channels of samples float32 holds exactly -- int16, packed
    24-bit, float32 -- at a rate ``mgx_resample`` converts; at the internal rate itself also 32-bit integers, which
    ``mgx_pcm_decode`` rounds as the host would.  An off-rate file of 32-bit integers or float64 keeps the host's
    float64 resampler, which sees every bit of it."""
    channels = pcm_channels(audio)
    if channels not in (1, 2) or audio.shape[0] == 0:
        return False
    if rate == internal_rate:
        return audio.dtype.kind in "iu" or audio.dtype == np.float32
    if audio.dtype not in (np.int16, np.uint8, np.float32):
        return False
    return converted_length(audio.shape[0], channels, rate, internal_rate) is not None


def final_frames(audio, rate, internal_rate):
    """Frame count of the track ``Device.track_frames`` makes of ``audio``."""
    if rate == internal_rate:
        return audio.shape[0]
    return converted_length(audio.shape[0], pcm_channels(audio), rate, internal_rate)


def _both_columns(audio):
    """A mono track in its file's encoding -> the same samples in two columns (dsp.py:45-46)."""
    if audio.dtype == np.uint8:                                   # packed 24-bit: (n, 3) -> (n, 6)
        return np.ascontiguousarray(np.repeat(audio.reshape(-1, 1, 3), 2, axis=1).reshape(-1, 6))
    return np.repeat(audio, repeats=2, axis=1)


class DeviceBuffer:
    """An HBM allocation owned by a Device.  ``release`` (or garbage collection) hands the block back to
    the device's free list -- hipMalloc / hipFree of a 170 MB block cost milliseconds and hipFree waits
    for the whole GPU, which would serialise the lanes of a batch -- and ``Device.close`` frees the lot."""

    def __init__(self, device, nbytes):
        self.device = device
        self.nbytes = int(nbytes)
        self.capacity = _size_class(max(self.nbytes, 1))
        self.ptr = device._take_block(self.capacity)

    def release(self):
        if self.ptr and self.device.handle:
            self.device._give_block(self.capacity, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class Device:
    """Handle to one GPU.  Raises ``MgxError`` when no GPU is visible: there is no CPU path."""

    def __init__(self, index=0):
        self.index = index
        self.handle = None
        # include/mgx.h: calls on one handle are serialised by the caller.  ctypes drops the GIL while a
        # call blocks, so two threads sharing a Device (the process-wide default one, typically) would
        # otherwise interleave inside the same stream and workspaces.  Every upload -> kernels ->
        # download sequence of this package runs under this lock.
        self.lock = threading.RLock()
        self._keep_until_sync = []            # host arrays with a queued DMA still reading them
        self._blocks = {}                     # free HBM blocks by size class
        self._free_hbm = 0                    # ... and their total size
        h = ctypes.c_void_p()
        check(library().mgx_create(index, ctypes.byref(h)))
        self.handle = h

    def close(self):
        if self.handle:
            for stack in self._blocks.values():
                for ptr in stack:
                    library().mgx_free(self.handle, ctypes.c_void_p(ptr))
            self._blocks.clear()
            library().mgx_destroy(self.handle)
            self.handle = None

    # HBM blocks are recycled: a block released while kernels of THIS handle may still read it is only
    # reused by later work on the same stream, which is ordered behind them
    KEEP_BLOCKS = 6
    MAX_FREE_HBM = 24 << 30                  # free HBM blocks kept per handle, in total (a lane's share of 288 GB)

    def _take_block(self, capacity):
        with self.lock:
            stack = self._blocks.get(capacity)
            if stack:
                self._free_hbm -= capacity
                return stack.pop()
        ptr = ctypes.c_void_p()
        check(library().mgx_malloc(self.handle, capacity, ctypes.byref(ptr)))
        return ptr.value

    def _give_block(self, capacity, ptr):
        with self.lock:
            stack = self._blocks.setdefault(capacity, [])
            if len(stack) < self.KEEP_BLOCKS and self._free_hbm + capacity <= self.MAX_FREE_HBM:
                stack.append(ptr)
                self._free_hbm += capacity
                return
        library().mgx_free(self.handle, ctypes.c_void_p(ptr))

    def trim(self):
        """Free every recycled HBM block of this handle."""
        with self.lock:
            stacks, self._blocks, self._free_hbm = self._blocks, {}, 0
        for stack in stacks.values():
            for ptr in stack:
                library().mgx_free(self.handle, ctypes.c_void_p(ptr))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- memory ----------------------------------------------------------------
    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def upload(self, array, dtype=np.float32):
        """numpy -> a new HBM buffer.  Returns as soon as the copy is queued on the stream: arrays from
        ``pinned.empty`` go by DMA straight from where they are; any other array is moved into a
        pinned block by four host threads, chunk by chunk, each chunk's DMA queued as it lands (about
        twice the rate of a pageable hipMemcpy).  The source must not be written before ``synchronize``
        or the next blocking call on this device.  ``dtype=None`` keeps the array's own type."""
        host = np.ascontiguousarray(array) if dtype is None else np.ascontiguousarray(array, dtype=dtype)
        buf = DeviceBuffer(self, max(host.nbytes, 1))
        if host.nbytes == 0:
            return buf
        lib = library()
        if pinned.holds(host):
            check(lib.mgx_memcpy_h2d_async(self.handle, ctypes.c_void_p(buf.ptr),
                                           host.ctypes.data_as(ctypes.c_void_p), host.nbytes))
            self._keep_until_sync.append(host)
            return buf
        stage = pinned.empty((host.nbytes,), np.uint8)
        src, dst = host.ctypes.data, stage.ctypes.data
        pieces = [(o, min(_STAGE_CHUNK, host.nbytes - o)) for o in range(0, host.nbytes, _STAGE_CHUNK)]
        landed = [_copiers.submit(ctypes.memmove, dst + o, src + o, n) for o, n in pieces]
        for (o, n), done in zip(pieces, landed):
            done.result()
            check(lib.mgx_memcpy_h2d_async(self.handle, ctypes.c_void_p(buf.ptr + o), ctypes.c_void_p(dst + o), n))
        self._keep_until_sync.append(stage)
        return buf

    def download(self, buf, shape, dtype=np.float32, wait=True):
        """HBM -> a numpy array in pinned memory (``pinned.empty``).  ``buf`` is a DeviceBuffer or a raw
        device address.  With ``wait=False`` the copy is only queued: call ``synchronize`` before
        reading the array."""
        out = pinned.empty(shape, dtype)
        ptr = buf if isinstance(buf, int) else buf.ptr
        if out.nbytes:
            check(library().mgx_memcpy_d2h_async(self.handle, out.ctypes.data_as(ctypes.c_void_p),
                                                 ctypes.c_void_p(ptr), out.nbytes))
        if wait:
            self.synchronize()
        return out

    # ---- integer PCM at the boundary (mgx_pcm_decode / mgx_pcm_encode) ---------------------------
    def upload_frames(self, array):
        """(n, channels) audio -> float32 frames in HBM.  Float arrays are uploaded as float32; integer
        arrays are what a PCM file holds (``audio_io.PCM_DTYPES``: int16, int32 with the sample in the high
        bits, or uint8 (n, channels * 3) of packed 24-bit samples): they cross PCIe as they are and become
        ``v / 2**(bits - 1)`` on the device."""
        bits = pcm_bits(array)
        if bits == 0:
            return self.upload(array)
        raw = self.upload(array, dtype=None)
        samples = array.size // 3 if bits == 24 else array.size
        out = DeviceBuffer(self, max(samples * 4, 1))
        check(library().mgx_pcm_decode(self.handle, ctypes.c_void_p(raw.ptr), samples, bits, ctypes.c_void_p(out.ptr)))
        raw.release()           # (recycled by later work on this stream only, which is ordered behind the decode)
        return out

    def resample_frames(self, buf, frames, channels, rate_in, rate_out):
        """checker.py:30-45 on float32 frames in HBM (``mgx_resample``): (frames, channels) at ``rate_in`` -> a new
        ``DeviceFrames`` of (n_out, 2) at ``rate_out``, queued on this device's stream.  Raises ``MgxError`` with
        ``code == ERR_UNSUPPORTED`` for the ratios the library leaves to the host."""
        lib = library()
        n_out = ctypes.c_int64()
        check(lib.mgx_resample(None, None, int(frames), int(channels), int(rate_in), int(rate_out), None, 0,
                               ctypes.byref(n_out)))
        out = DeviceBuffer(self, max(n_out.value * 8, 1))
        ptr = buf.ptr if hasattr(buf, "ptr") else buf.buf.ptr
        try:
            check(lib.mgx_resample(self.handle, ctypes.c_void_p(ptr), int(frames), int(channels), int(rate_in),
                                   int(rate_out), ctypes.c_void_p(out.ptr), n_out.value, ctypes.byref(n_out)))
        except Exception:
            out.release()
            raise
        return DeviceFrames(out, n_out.value)

    def convert_rate(self, buf, frames, rate_in, rate_out):
        """(frames, 2) float32 in HBM at ``rate_in`` -> a new ``DeviceFrames`` of (n_out, 2) at ``rate_out``
        (``mgx_convert_rate``: the deliveries' converter, bit-identical to ``resample_frames`` of two channels), queued on
        this device's stream.  Raises ``MgxError`` with ``code == ERR_UNSUPPORTED`` for the ratios the library refuses."""
        lib = library()
        n_out = ctypes.c_int64()
        check(lib.mgx_convert_rate(None, None, int(frames), int(rate_in), int(rate_out), None, 0, ctypes.byref(n_out)))
        out = DeviceBuffer(self, max(n_out.value * 8, 1))
        ptr = buf.ptr if hasattr(buf, "ptr") else buf.buf.ptr
        try:
            check(lib.mgx_convert_rate(self.handle, ctypes.c_void_p(ptr), int(frames), int(rate_in), int(rate_out),
                                       ctypes.c_void_p(out.ptr), n_out.value, ctypes.byref(n_out)))
        except Exception:
            out.release()
            raise
        return DeviceFrames(out, n_out.value)

    def resample_plan(self, rate_in, rate_out):
        """(device address of the weights, phases, entries per phase, plans designed on this handle so far) for a
        rate pair this handle has converted (``mgx_resample_plan``)."""
        ptr, phases, width, designed = ctypes.c_void_p(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        check(library().mgx_resample_plan(self.handle, int(rate_in), int(rate_out), ctypes.byref(ptr),
                                          ctypes.byref(phases), ctypes.byref(width), ctypes.byref(designed)))
        return ptr.value, phases.value, width.value, designed.value

    def track_frames(self, audio, rate, internal_rate):
        """A loaded track (``takes_resident``) -> ``DeviceFrames`` at the internal rate: uploaded as the file holds it,
        decoded (``mgx_pcm_decode``) and, off-rate, converted (``mgx_resample``, which also gives a mono track its
        second column).  A mono track at the internal rate is given its second column on the way up."""
        if rate == internal_rate:
            if pcm_channels(audio) == 1:
                audio = _both_columns(audio)
            return DeviceFrames(self.upload_frames(audio), audio.shape[0])
        decoded = self.upload_frames(audio)
        try:
            return self.resample_frames(decoded, audio.shape[0], pcm_channels(audio), rate, internal_rate)
        finally:
            decoded.release()         # (recycled by later work on this stream only, which is ordered behind the kernel)

    def peak_count(self, buf, samples):
        """dsp.py:49-54 count_max_peaks of float32 samples in HBM: (largest magnitude, samples on it)."""
        peak, count = ctypes.c_double(), ctypes.c_int64()
        ptr = buf.ptr if hasattr(buf, "ptr") else buf.buf.ptr
        check(library().mgx_peak_count(self.handle, ctypes.c_void_p(ptr), int(samples), ctypes.byref(peak),
                                       ctypes.byref(count)))
        return peak.value, count.value

    def loudness(self, buf, frames, rate, sub_energy=False):
        """BS.1770-4 loudness and true peak of (frames, 2) float32 in HBM at ``rate`` Hz (``mgx_loudness``): a
        ``loudness.Loudness``; with ``sub_energy=True`` also the (frames // S, 2) K-weighted sub-block energies."""
        from .loudness import from_report

        report, got = _native.MgxLoudnessReport(), ctypes.c_int64()
        ptr = buf.ptr if hasattr(buf, "ptr") else buf.buf.ptr
        capacity = int(frames) // ((int(rate) + 5) // 10) if sub_energy and rate > 0 else 0
        energy = np.zeros((capacity, 2)) if sub_energy else None
        check(library().mgx_loudness(self.handle, ctypes.c_void_p(ptr), int(frames), int(rate), ctypes.byref(report),
                                     None if energy is None else energy.ctypes.data_as(_native.c_double_p), capacity,
                                     ctypes.byref(got)))
        self._keep_until_sync.clear()          # (the call has waited for the stream: the uploads queued before it are done)
        value = from_report(report, rate, frames)
        return (value, energy) if sub_energy else value

    def audit(self, buf, frames, rate, bits=0, limits=None, sub_sums=False):
        """The quality-control pass over (frames, 2) samples in HBM at ``rate`` Hz (``mgx_audit``): float32 frames
        (``bits`` 0) or the integer PCM of a file (16, 24 packed, 32).  ``limits``: a ``qc.AuditLimits``, default its
        defaults.  Returns a ``qc.Audit``; with ``sub_sums=True`` also the (sub-blocks, 3) sums of L^2, R^2 and L R."""
        from .qc import AuditLimits, from_report

        limits = AuditLimits() if limits is None else limits
        report, got = _native.MgxAuditReport(), ctypes.c_int64()
        ptr = buf.ptr if hasattr(buf, "ptr") else buf.buf.ptr
        block = (int(rate) + 5) // 10
        capacity = -(-int(frames) // block) if sub_sums and block > 0 and frames > 0 else 0
        sums = np.zeros((capacity, 3)) if sub_sums else None
        check(library().mgx_audit(self.handle, ctypes.c_void_p(ptr), int(frames), int(bits), int(rate),
                                  ctypes.byref(limits.native()), ctypes.byref(report),
                                  None if sums is None else sums.ctypes.data_as(_native.c_double_p), capacity,
                                  ctypes.byref(got)))
        self._keep_until_sync.clear()          # (the call has waited for the stream: the uploads queued before it are done)
        value = from_report(report, rate)
        return (value, sums) if sub_sums else value

    def declip(self, buf, frames, params, report=True):
        """Clip repair of (frames, 2) float32 in HBM (``mgx_declip``): ``params`` is a ``_native.MgxDeclipParams``.
        Returns ``(out, report)``: the repaired frames in a new DeviceBuffer and the ``_native.MgxDeclipReport``, for
        which the call waits; with ``report=False`` it is only queued and the second value is None."""
        ptr = buf.ptr if hasattr(buf, "ptr") else buf.buf.ptr
        made = DeviceBuffer(self, max(int(frames) * 8, 1))
        found = _native.MgxDeclipReport() if report else None
        try:
            check(library().mgx_declip(self.handle, ctypes.c_void_p(ptr), int(frames), ctypes.byref(params),
                                       ctypes.c_void_p(made.ptr), ctypes.byref(found) if report else None))
        except Exception:
            made.release()
            raise
        if report and frames > 0:
            self._keep_until_sync.clear()      # (the call has waited for the stream)
        return made, found

    def declip_report(self):
        """The report of the most recent ``declip`` of this device, for one queued with ``report=False``
        (``mgx_declip_report_read``); waits for the stream."""
        found = _native.MgxDeclipReport()
        check(library().mgx_declip_report_read(self.handle, ctypes.byref(found)))
        return found

    def overview(self, buf, frames, rate, columns):
        """The waveform overview of (frames, 2) float32 in HBM (``mgx_overview``): a ``visuals.Overview`` of ``columns``
        columns."""
        from .visuals import Overview

        columns = int(columns) if frames > 0 else 0
        minmax, sumsq = np.zeros((columns, 2, 2), dtype=np.float32), np.zeros((columns, 2))
        ptr = buf.ptr if hasattr(buf, "ptr") else buf.buf.ptr
        check(library().mgx_overview(self.handle, ctypes.c_void_p(ptr), int(frames), columns,
                                     minmax.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                     sumsq.ctypes.data_as(_native.c_double_p)))
        self._keep_until_sync.clear()          # (the call has waited for the stream)
        return Overview(int(rate), int(frames), minmax[:, :, 0].copy(), minmax[:, :, 1].copy(), sumsq)

    def spectrogram(self, buf, frames, rate, fft_size=4096, hop=1024, columns=0, edges=None, channels="lr"):
        """The spectrogram of (frames, 2) float32 in HBM (``mgx_spectrogram``): a ``visuals.Spectrogram``.  ``edges``:
        the bands' bin edges (int32), default every bin."""
        from . import visuals

        edges = visuals.linear_bands(fft_size) if edges is None else np.ascontiguousarray(edges, dtype=np.int32)
        spec = visuals.spec_of(fft_size, hop, columns, channels, edges)
        edges_p = edges.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        hops, width = ctypes.c_int64(), ctypes.c_int32()
        check(library().mgx_spectrogram_plan(int(frames), ctypes.byref(spec), edges_p, ctypes.byref(hops), ctypes.byref(width)))
        power = np.zeros((width.value, 2, spec.bands), dtype=np.float32)
        got = ctypes.c_int64()
        ptr = buf.ptr if hasattr(buf, "ptr") else buf.buf.ptr
        check(library().mgx_spectrogram(self.handle, ctypes.c_void_p(ptr), int(frames), ctypes.byref(spec), edges_p,
                                        power.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), power.size, ctypes.byref(got)))
        self._keep_until_sync.clear()
        return visuals.Spectrogram(int(rate), int(frames), int(fft_size), int(hop), int(hops.value), channels, edges, power)

    def download_pcm(self, buf, frames, channels, bits, wait=True):
        """float32 frames in HBM -> integer PCM on the host (pinned): int16 / int32 (n, channels), or uint8
        (n, channels * 3) for packed 24-bit.  Quantised on the device as libsndfile would on the host."""
        samples = frames * channels
        nbytes = samples * bits // 8
        pcm = DeviceBuffer(self, max(nbytes, 1))
        check(library().mgx_pcm_encode(self.handle, ctypes.c_void_p(buf.ptr), samples, bits, ctypes.c_void_p(pcm.ptr)))
        shape, dtype = {16: ((frames, channels), np.int16), 32: ((frames, channels), np.int32),
                        24: ((frames, channels * 3), np.uint8)}[bits]
        out = self.download(pcm, shape, dtype, wait=False)
        pcm.release()
        if wait:
            self.synchronize()
        return out

    def deliver(self, buf, frames, channels, gain, bits, dither=0, seed=0, wait=True, inspect=None):
        """float32 frames in HBM -> a delivery rendition on the host (pinned), in one pass on the device
        (``mgx_deliver``): every sample times ``gain``, dithered (0 none, 1 TPDF, 2 high-passed TPDF, keyed by ``seed``),
        quantised and packed -- int16 / int32 (n, channels), uint8 (n, channels * 3) for packed 24-bit, or float32
        (n, channels) for ``bits`` 0.  ``inspect``: called with the DeviceBuffer the kernel wrote, before it is
        downloaded (the audit of the file as written)."""
        samples = int(frames) * int(channels)
        nbytes = samples * (bits // 8 if bits else 4)
        out_dev = DeviceBuffer(self, max(nbytes, 1))
        ptr = buf.ptr if hasattr(buf, "ptr") else buf.buf.ptr
        try:
            check(library().mgx_deliver(self.handle, ctypes.c_void_p(ptr), samples, float(gain), int(bits), int(dither),
                                        int(seed), ctypes.c_void_p(out_dev.ptr)))
            if inspect is not None:
                inspect(out_dev)
            shape, dtype = {0: ((frames, channels), np.float32), 16: ((frames, channels), np.int16),
                            32: ((frames, channels), np.int32), 24: ((frames, channels * 3), np.uint8)}[int(bits)]
            out = self.download(out_dev, shape, dtype, wait=False)
        finally:
            out_dev.release()   # (recycled by later work on this stream only, which is ordered behind the copy)
        if wait:
            self.synchronize()
        return out

    def deliver_shaped(self, buf, frames, gain, bits, shaper, seed=0, wait=True, inspect=None):
        """(frames, 2) float32 in HBM -> a noise-shaped 16 or 24-bit rendition on the host (pinned), in one launch
        (``mgx_deliver_shaped``): every sample times ``gain``, TPDF-dithered (keyed by ``seed``), quantised with the error
        fed back through ``shaper`` (a ``delivery.NoiseShaper``) and packed -- int16 (n, 2), or uint8 (n, 6) for packed
        24-bit.  ``inspect``: as ``deliver``'s."""
        nbytes = int(frames) * 2 * (int(bits) // 8)
        out_dev = DeviceBuffer(self, max(nbytes, 1))
        ptr = buf.ptr if hasattr(buf, "ptr") else buf.buf.ptr
        try:
            check(library().mgx_deliver_shaped(self.handle, ctypes.c_void_p(ptr), int(frames), float(gain), int(bits),
                                               ctypes.byref(shaper.native()), int(seed), ctypes.c_void_p(out_dev.ptr)))
            if inspect is not None:
                inspect(out_dev)
            shape, dtype = {16: ((frames, 2), np.int16), 24: ((frames, 6), np.uint8)}[int(bits)]
            out = self.download(out_dev, shape, dtype, wait=False)
        finally:
            out_dev.release()   # (recycled by later work on this stream only, which is ordered behind the copy)
        if wait:
            self.synchronize()
        return out

    def tp_limit(self, buf, frames, pre_gain, ceiling, lookahead, release, out=None, reduction=True):
        """The deliveries' true-peak look-ahead limiter on (frames, 2) float32 in HBM (``mgx_tp_limit``): pre-gain and
        ceiling linear, look-ahead and release in frames.  Returns ``(out, max_reduction)``: the limited frames in a new
        DeviceBuffer (or in ``out``) and the largest gain reduction s, for which the call waits; with ``reduction=False``
        it is only queued and the second value is None."""
        ptr = buf.ptr if hasattr(buf, "ptr") else buf.buf.ptr
        made = out if out is not None else DeviceBuffer(self, max(int(frames) * 8, 1))
        worst = ctypes.c_double()
        try:
            check(library().mgx_tp_limit(self.handle, ctypes.c_void_p(ptr), int(frames), float(pre_gain), float(ceiling),
                                         int(lookahead), float(release), ctypes.c_void_p(made.ptr),
                                         ctypes.byref(worst) if reduction else None))
        except Exception:
            if out is None:
                made.release()
            raise
        if reduction:
            self._keep_until_sync.clear()      # (the call has waited for the stream)
        return made, (worst.value if reduction else None)

    # ---- previews on frames that are still in HBM (mgx_window_energy / mgx_preview_cut) ----------
    def window_energy(self, buf, frames, size, step):
        """dsp.py:128-143: sum of squares (both channels) of every window of ``size`` frames every ``step``."""
        size = min(int(size), int(frames))
        count = (int(frames) - size) // int(step) + 1
        energy = (ctypes.c_double * count)()
        got = ctypes.c_int64()
        check(library().mgx_window_energy(self.handle, ctypes.c_void_p(buf.ptr), int(frames), size, int(step), energy,
                                          count, ctypes.byref(got)))
        return np.frombuffer(energy, dtype=np.float64, count=got.value).copy()

    def preview_cut(self, buf, frames, begin, size, fade, clip_limit=0.0):
        """Frames [begin, begin + size) clipped (``clip_limit`` > 0) and faded: a new DeviceBuffer."""
        out = DeviceBuffer(self, max(int(size) * 8, 1))
        check(library().mgx_preview_cut(self.handle, ctypes.c_void_p(buf.ptr), int(frames), int(begin), int(size),
                                        int(fade), float(clip_limit), ctypes.c_void_p(out.ptr)))
        return out

    def synchronize(self):
        check(library().mgx_synchronize(self.handle))
        self._keep_until_sync.clear()

    def timer_start(self):
        check(library().mgx_timer_start(self.handle))

    def timer_stop(self):
        ms = ctypes.c_float()
        check(library().mgx_timer_stop(self.handle, ctypes.byref(ms)))
        return ms.value

    # ---- per-stage device times of mgx_master (bench.py) ---------------------------
    def stage_timing(self, enable=True):
        check(library().mgx_stage_timing(self.handle, int(bool(enable))))

    def stage_times(self):
        """Milliseconds per stage of the last ``master`` call, keyed by stage name (``None`` = not run)."""
        ms = (ctypes.c_float * len(_native.STAGES))()
        check(library().mgx_stage_times(self.handle, ms))
        return {name: (float(v) if v >= 0 else None) for name, v in zip(_native.STAGES, ms)}

    # ---- the boundary ------------------------------------------------------------
    def reference_profile(self, reference, n_reference, native_config):
        """``mgx_reference_profile`` on a reference in HBM (a DeviceBuffer): the profile's bytes
        (``mgx_profile_header`` + spectra), downloaded.  ``profile.ReferenceProfile`` wraps them."""
        lib = library()
        nbytes = ctypes.c_size_t()
        check(lib.mgx_profile_bytes(ctypes.byref(native_config), ctypes.byref(nbytes)))
        with self.lock:
            block = DeviceBuffer(self, nbytes.value)
            try:
                check(lib.mgx_reference_profile(self.handle, ctypes.c_void_p(reference.ptr), int(n_reference),
                                                ctypes.byref(native_config), ctypes.c_void_p(block.ptr)))
                host = ctypes.create_string_buffer(nbytes.value)
                # (the blocking copy: a NaN or an infinity in the reference fails here)
                check(lib.mgx_memcpy_d2h(self.handle, host, ctypes.c_void_p(block.ptr), nbytes.value))
                self._keep_until_sync.clear()
                return host.raw
            finally:
                block.release()

    def profile_merge(self, sources, weights, native_config):
        """``mgx_profile_merge`` on profiles in HBM (DeviceBuffers, at most 64): the merged profile's bytes, downloaded.
        One launch and one copy; a source that does not fit fails at the copy, naming its field and position."""
        lib = library()
        nbytes = ctypes.c_size_t()
        check(lib.mgx_profile_bytes(ctypes.byref(native_config), ctypes.byref(nbytes)))
        count = len(sources)
        pointers = (ctypes.c_void_p * count)(*[b.ptr for b in sources])
        counted = (ctypes.c_int32 * count)(*weights)
        with self.lock:
            block = DeviceBuffer(self, nbytes.value)
            try:
                check(lib.mgx_profile_merge(self.handle, pointers, counted, count, ctypes.byref(native_config),
                                            ctypes.c_void_p(block.ptr)))
                host = ctypes.create_string_buffer(nbytes.value)
                check(lib.mgx_memcpy_d2h(self.handle, host, ctypes.c_void_p(block.ptr), nbytes.value))
                self._keep_until_sync.clear()
                return host.raw
            finally:
                block.release()

    def master(self, target, n_target, reference, n_reference, native_config, result=None,
               result_no_limiter=None, result_no_limiter_normalized=None, want_report=True, fir=None, profile=None,
               eq=None):
        """``mgx_master`` on device buffers.  Outputs are DeviceBuffers or None.  ``fir`` (a DeviceBuffer
        holding [2][fft_size] float32) replaces the designed matching FIR: ``mgx_master_with_fir``.  ``profile``
        (a DeviceBuffer holding a reference profile) stands for the reference, which is then None:
        ``mgx_master_with_profile``.  ``eq`` (an ``eq.MatchingEq``) shapes the FIR that is designed:
        ``mgx_master_shaped``, on either route -- ``mgx_master_eq`` where it carries tone controls that are not neutral; a
        given ``fir`` is used as given, whatever ``eq`` says."""
        report = MgxReport() if want_report else None

        def p(b):
            return ctypes.c_void_p(b.ptr) if b is not None else None

        rep = ctypes.byref(report) if report is not None else None
        if profile is not None and reference is not None:
            raise ValueError("master: a reference track or a reference profile, not both")
        tone = eq.tone_native() if eq is not None and fir is None else None
        if tone is not None:                                # (not neutral: k_eq_tone in place of k_eq_shape)
            check(library().mgx_master_eq(
                self.handle, p(target), n_target, p(reference), n_reference, p(profile), ctypes.byref(native_config),
                ctypes.byref(eq.to_native()), ctypes.byref(tone), p(result), p(result_no_limiter),
                p(result_no_limiter_normalized), rep))
        elif eq is not None and fir is None:
            check(library().mgx_master_shaped(
                self.handle, p(target), n_target, p(reference), n_reference, p(profile), ctypes.byref(native_config),
                ctypes.byref(eq.to_native()), p(result), p(result_no_limiter), p(result_no_limiter_normalized), rep))
        elif profile is not None:
            check(library().mgx_master_with_profile(
                self.handle, p(target), n_target, p(profile), ctypes.byref(native_config), p(fir),
                p(result), p(result_no_limiter), p(result_no_limiter_normalized), rep))
        elif fir is None:
            check(library().mgx_master(
                self.handle, p(target), n_target, p(reference), n_reference, ctypes.byref(native_config),
                p(result), p(result_no_limiter), p(result_no_limiter_normalized), rep))
        else:
            check(library().mgx_master_with_fir(
                self.handle, p(target), n_target, p(reference), n_reference, ctypes.byref(native_config), p(fir),
                p(result), p(result_no_limiter), p(result_no_limiter_normalized), rep))
        return report

    def last_fir(self):
        """(device address, taps) of the FIR pair the last ``master`` designed or was given."""
        ptr, taps = ctypes.c_void_p(), ctypes.c_int32()
        check(library().mgx_last_fir(self.handle, ctypes.byref(ptr), ctypes.byref(taps)))
        return ptr.value, taps.value

    # ---- RCCL: the FIR exchange of the multi-GPU path --------------------------------
    def comm_init(self, rank, world, exchange=None):
        """Join a communicator of ``world`` ranks.  ``exchange(payload, size) -> bytes`` must hand rank 0's
        128-byte id to every rank (bench.Ranks.broadcast_bytes does); not needed for world == 1."""
        from .ranks import single_node_rccl_defaults

        single_node_rccl_defaults()          # (only what the host has not set; nothing when the ranks span machines)
        lib = library()
        uid = ctypes.create_string_buffer(128)
        if rank == 0:
            check(lib.mgx_comm_unique_id(uid))
        payload = uid.raw if exchange is None else exchange(uid.raw, 128)
        check(lib.mgx_comm_init(self.handle, ctypes.c_char_p(payload), rank, world))

    def comm_broadcast(self, buf, count, root=0):
        ptr = buf if isinstance(buf, int) else buf.ptr
        check(library().mgx_comm_broadcast_f32(self.handle, ctypes.c_void_p(ptr), count, root))

    def comm_destroy(self):
        check(library().mgx_comm_destroy(self.handle))


_default = {}


def default_device(index=0):
    """Process-wide Device for GPU ``index`` (created on first use)."""
    if index not in _default:
        _default[index] = Device(index)
    return _default[index]


def device_count():
    n = ctypes.c_int()
    rc = library().mgx_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


def pci_bus_id(index=0):
    """PCI address of GPU ``index`` ("0000:0d:00.0"): which physical device a rank or lane sits on."""
    buf = ctypes.create_string_buffer(32)
    check(library().mgx_device_pci_bus_id(int(index), buf, 32))
    return buf.value.decode("ascii", "replace")
