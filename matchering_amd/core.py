"""``process``: the public entry point with the reference's signature, log codes and exceptions
(matchering/core.py:32-121).  The work is split the way this package needs it: two host-side steps
around the one call that runs on the GPU.

    files --_read_pair--> frames at the internal rate --stages.main (MI355X)--> three renderings
          --_write_results--> files (+ optional previews)

Integer PCM and float32 WAVE files are mapped, not decoded: their samples go to the GPU as the file holds
them (``mgx_pcm_decode``), the target's peak statistics are taken there (``mgx_peak_count``), and renderings
come back quantised for the ``Result`` files' subtype (``mgx_pcm_encode``) -- see ``_read_pair`` and
``_wanted_encodings``.
"""

import os

import numpy as np

from .audio_io import load, pcm_channels, pcm_to_float, save
from .checker import check, check_equality
from .config import Config
from .delivery import DeliveryRequest, plain_results, write_deliveries
from .log import Code, ModuleError, debug, debug_line, info
from .preview import PreviewRequest, create_preview, save_previews
from .results import Result
from .stages import main
from .utils import get_temp_folder


def _wanted_renderings(results):
    """Which of stages.main's three outputs the requested files need (core.py:77-86)."""
    limited = plain = normalized = False
    for item in results:
        if item.use_limiter:
            limited = True
        elif item.normalize:
            normalized = True
        else:
            plain = True
    return limited, plain, normalized


def _wanted_encodings(results):
    """Per rendering, the PCM subtype the GPU can quantise to directly: every file made from that rendering
    is a WAVE file of one and the same integer subtype (saver.py:27-33 would quantise on the host)."""
    from .stages import PCM_BITS

    wanted = [set(), set(), set()]
    for item in results:
        slot = 0 if item.use_limiter else (2 if item.normalize else 1)
        wave = os.path.splitext(item.file)[1][1:].upper() in ("WAV", "WAVE")
        wanted[slot].add(item.subtype if wave and item.subtype in PCM_BITS else None)
    return tuple(next(iter(w)) if len(w) == 1 else None for w in wanted)


def _file_encoding(item):
    """The integer subtype of one WAVE file (quantised on the GPU), or None (float frames, host codec)."""
    from .stages import PCM_BITS

    if item is None or os.path.splitext(item.file)[1][1:].upper() not in ("WAV", "WAVE"):
        return None
    return item.subtype if item.subtype in PCM_BITS else None


def _gpu():
    """The default device, or None where there is none (the CPU tests put a stand-in behind ``main``)."""
    try:
        from .device import default_device

        return default_device()
    except Exception:       # noqa: BLE001 -- no library, no GPU: the host-side checks do all of it
        return None


def _read_pair(target_path, reference_path, config, temp_folder):
    """Load and check both tracks (core.py:52-74); raises ModuleError with the reference's codes.  Integer
    PCM and float32 tracks go to the GPU at once, as their files hold them (``device.takes_resident``): they are
    decoded there, brought to two channels at the internal rate there when they are mono or off-rate
    (``mgx_resample``), the target's peak statistics (checker.py:118-130) are taken there, and ``main`` receives
    them resident.  ``check`` does everything else, for every track."""
    from .device import takes_resident

    dev = _gpu()
    internal = config.internal_sample_rate
    tracks, resident, converted = [], [], []
    for path, role in ((target_path, "target"), (reference_path, "reference")):
        audio, rate = load(path, role, temp_folder, pcm=True)    # 16/24/32-bit WAVE: decoded on the GPU
        peaks, frames = None, None
        if dev is not None and takes_resident(audio, rate, internal):
            with dev.lock:
                frames = dev.track_frames(audio, rate, internal)
                if role == "target":
                    peaks = dev.peak_count(frames, 2 * frames.frames)
        # (the host array is not the final track when the device has changed its rate or its channels)
        changed = frames is not None and (rate != internal or pcm_channels(audio) != 2)
        try:
            tracks.append(check(audio, rate, config, role, peaks=peaks, on_device=changed))
        except Exception:
            for f in resident + [frames]:
                if f is not None:
                    f.release()
            raise
        resident.append(frames)
        converted.append(frames if changed else None)
    (target, target_rate), (reference, reference_rate) = tracks
    try:
        if not config.allow_equality:
            check_equality(target, reference, converted)
        lengths = [array.shape[0] if frames is None else frames.frames
                   for array, frames in zip((target, reference), converted)]
        channels = [pcm_channels(array) if frames is None else 2 for array, frames in zip((target, reference), converted)]
        consistent = (
            target_rate == reference_rate == internal
            and channels[0] == channels[1] == 2
            and min(lengths) > config.fft_size
        )
        if not consistent:
            raise ModuleError(Code.ERROR_VALIDATION)
    except Exception:
        for f in resident:
            if f is not None:
                f.release()
        raise
    return target, reference, resident


def _as_profile(reference, config=None):
    """The ``ReferenceProfile`` that ``process`` was given in the reference's place -- the object itself, the path of
    a saved one, recognised by the file's magic and not by its name, or a SET of references (``is_reference_set``: each
    file loaded and analysed as ``process`` does with its reference, same log codes, and the lot merged into one
    profile) -- or None for an audio file."""
    from .profile import ReferenceProfile, is_profile_file, is_reference_set

    if isinstance(reference, ReferenceProfile):
        return reference
    if is_reference_set(reference):
        return ReferenceProfile.analyze(reference, config)
    if isinstance(reference, (str, bytes, os.PathLike)) and is_profile_file(reference):
        return ReferenceProfile.load(reference)
    return None


NO_EQUALITY_CHECK = ("the reference is a profile, not audio: whether it was made from the target itself "
                     "(checker.py:140-142) cannot be checked and is not")


def read_track(path, role, config, temp_folder, dev):
    """``_read_pair`` for ONE track in the given role (its partner is a profile, or it is becoming one): loaded,
    taken resident where ``device.takes_resident`` says so (the target's peak statistics then come from the GPU),
    checked and validated as core.py:52-74 does.  Returns (checked array, resident ``DeviceFrames`` or None)."""
    from .device import takes_resident

    internal = config.internal_sample_rate
    audio, rate = load(path, role, temp_folder, pcm=True)
    peaks, frames = None, None
    if dev is not None and takes_resident(audio, rate, internal):
        with dev.lock:
            frames = dev.track_frames(audio, rate, internal)
            if role == "target":
                peaks = dev.peak_count(frames, 2 * frames.frames)
    changed = frames is not None and (rate != internal or pcm_channels(audio) != 2)
    try:
        array, checked_rate = check(audio, rate, config, role, peaks=peaks, on_device=changed)
        length = frames.frames if changed else array.shape[0]
        channels = 2 if changed else pcm_channels(array)
        if checked_rate != internal or channels != 2 or length <= config.fft_size:
            raise ModuleError(Code.ERROR_VALIDATION)
    except Exception:
        if frames is not None:
            frames.release()
        raise
    return array, frames


def _same_file(a, b):
    try:
        return os.path.exists(a) and os.path.samefile(a, b)
    except OSError:
        return False


def _write_results(results, renderings, sample_rate, deliveries=None):
    """One file per Result, each from the rendering it asked for (core.py:95-108); a Result with a delivery from the
    array ``stages.main`` left in the ``DeliveryRequest``, at its delivery's own rate."""
    limited, plain, normalized = renderings
    for item in plain_results(results):
        audio = limited if item.use_limiter else (normalized if item.normalize else plain)
        save(item.file, audio, sample_rate, item.subtype)
    if deliveries:
        write_deliveries(results, deliveries, sample_rate)


def process(target: str, reference: str, results: list, config: Config = None,
            preview_target: Result = None, preview_result: Result = None, loudness=None, eq=None):
    # (``loudness``: no counterpart in the reference -- a callable that receives (name, loudness.Loudness) for "target",
    # for "reference" when its audio was loaded, and for each rendering the results need ("result", "result_no_limiter",
    # "result_no_limiter_normalized"), measured on the frames in HBM; None: nothing is measured, nothing else changes.
    # ``eq``: an eq.MatchingEq -- how much of the matching curve is applied, its boost and cut caps, the phase of the FIR;
    # None: the reference's FIR.  What the library refuses is a ValueError before a file is read.)
    from .eq import as_eq

    config = Config() if config is None else config
    eq = as_eq(eq)
    if eq is not None:
        eq.check(config)
    debug("matchering_amd: the MI355X path behind the API of https://github.com/sergree/matchering")
    debug_line()
    info(Code.INFO_LOADING)
    if not results:
        raise RuntimeError("The result list is empty")
    temp_folder = config.temp_folder or get_temp_folder(results)
    # (a delivery rate the device converter refuses is a ValueError here, before a file is read)
    DeliveryRequest.for_results(results).check_rates(config.internal_sample_rate)

    profile = _as_profile(reference, config)
    if profile is not None:
        # the reference is a profile (given, or just made of a set of references): only the target is loaded and checked
        profile.matches(config)
        target_audio, frames = read_track(target, "target", config, temp_folder, _gpu())
        reference_audio, resident = profile, [frames, profile]
        if not config.allow_equality:
            debug(NO_EQUALITY_CHECK)
    else:
        target_audio, reference_audio, resident = _read_pair(target, reference, config, temp_folder)
    previews = bool(preview_target or preview_result)
    # With a GPU the previews are cut on it from the frames stages.main leaves in HBM (preview.PreviewRequest):
    # only the two 30 s pieces cross PCIe, and the renderings keep their integer encodings.  Without one (the
    # CPU tests put a stand-in behind ``main``) they are cut from float renderings on the host.
    request = None
    if previews and _gpu() is not None:
        request = PreviewRequest(config, preview_target, preview_result,
                                 (_file_encoding(preview_target), _file_encoding(preview_result)))
    # results with a delivery are cut from the renderings in HBM and come back in the DeliveryRequest: they take no part
    # in which renderings are returned, or in the "one subtype per rendering" rule of _wanted_encodings
    ordinary = plain_results(results)
    deliveries = DeliveryRequest.for_results(results)
    encodings = None if (previews and request is None) else _wanted_encodings(ordinary)
    extra = {"preview": request} if request is not None else {}
    if loudness is not None:
        extra["loudness"] = loudness
    if deliveries:
        extra["deliveries"] = deliveries
    if eq is not None:
        extra["eq"] = eq
    renderings = main(resident[0] if resident[0] is not None else target_audio,
                      resident[1] if resident[1] is not None else reference_audio,
                      config, *_wanted_renderings(ordinary), encodings=encodings, **extra)   # (releases the resident frames)
    del reference_audio

    debug_line()
    info(Code.INFO_EXPORTING)
    if previews and request is None and any(_same_file(item.file, target) for item in results):
        # the target may be a read-only mapping of its file (audio_io.read_wav): a result written over that
        # file would pull the mapping from under the preview cut below
        target_audio = np.array(target_audio, copy=True)
    _write_results(results, renderings, config.internal_sample_rate, deliveries)

    if request is not None:
        save_previews(request, config, preview_target, preview_result)
    elif previews:
        mastered = next((audio for audio in renderings if audio is not None), None)
        if mastered is None:                                   # every result is a delivery: the first of them
            mastered = pcm_to_float(deliveries.arrays[results[0].file])
        create_preview(pcm_to_float(target_audio), mastered, config, preview_target, preview_result)

    debug_line()
    info(Code.INFO_COMPLETED)
