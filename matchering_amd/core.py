"""``process``: the public entry point with the reference's signature, log codes and exceptions
(matchering/core.py:32-121).  The work is split the way this package needs it: two host-side steps
around the one call that runs on the GPU.

    files --intake--> frames at the internal rate --stages.main (MI355X)--> three renderings
          --delivery.write_results--> files (+ optional previews)

How a file becomes a track is ``intake``'s to know, which renderings and encodings the results need and how they are
written ``delivery``'s (``renderings_wanted``, ``write_results``).
"""

import os

import numpy as np

from . import intake
from .audio_io import pcm_to_float
from .config import Config
from .delivery import DeliveryRequest, file_encoding, renderings_wanted, write_results
from .log import Code, debug, debug_line, info
from .preview import PreviewRequest, create_preview, save_previews
from .results import Result
from .stages import main
from .utils import get_temp_folder


def _gpu():
    """The default device, or None where there is none (the CPU tests put a stand-in behind ``main``)."""
    try:
        from .device import default_device

        return default_device()
    except Exception:       # noqa: BLE001 -- no library, no GPU: the host-side checks do all of it
        return None


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


def _same_file(a, b):
    try:
        return os.path.exists(a) and os.path.samefile(a, b)
    except OSError:
        return False


def process(target: str, reference: str, results: list, config: Config = None,
            preview_target: Result = None, preview_result: Result = None, loudness=None, eq=None, audit=None,
            visuals=None, repair=None):
    # (``loudness``: no counterpart in the reference -- a callable that receives (name, loudness.Loudness) for "target",
    # for "reference" when its audio was loaded, and for each rendering the results need ("result", "result_no_limiter",
    # "result_no_limiter_normalized"), measured on the frames in HBM; None: nothing is measured, nothing else changes.
    # ``eq``: an eq.MatchingEq -- how much of the matching curve is applied, its boost and cut caps, the phase of the FIR;
    # None: the reference's FIR.  What the library refuses is a ValueError before a file is read.
    # ``audit``: a callable that receives (name, qc.Audit) for the same names, and for "delivered:" + file the audit of the
    # integer samples a delivery writes, read in HBM before they are downloaded; None: nothing is launched.
    # ``visuals``: a callable, or a pair (callable, visuals.VisualsRequest) giving the sizes, that receives (name,
    # visuals.Visuals) -- waveform overview and spectrogram of the frames in HBM -- for "target", "reference" and each
    # rendering; None: nothing is launched.
    # ``repair``: a repair.ClipRepair, its JSON (True or an object), or a pair (callable, ClipRepair) whose callable receives
    # ("target", repair.Repaired) -- the target's short runs at the rail are rebuilt in HBM before it is mastered, and
    # everything downstream hears the repaired frames.  What the library refuses is a ValueError before a file is read.
    # None: nothing is launched.)
    from .eq import as_eq
    from .repair import as_repair

    config = Config() if config is None else config
    eq = as_eq(eq)
    if eq is not None:
        eq.check(config)
    as_repair(repair)
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
        target_track = intake.read_single(target, "target", config, temp_folder, _gpu())
        intake.no_equality_check(config)
        reference_audio = profile
    else:
        target_track, reference_track = intake.read_pair(target, reference, config, temp_folder, _gpu())
        reference_audio = reference_track.for_main
        del reference_track
    target_audio = target_track.array
    previews = bool(preview_target or preview_result)
    # With a GPU the previews are cut on it from the frames stages.main leaves in HBM (preview.PreviewRequest):
    # only the two 30 s pieces cross PCIe, and the renderings keep their integer encodings.  Without one (the
    # CPU tests put a stand-in behind ``main``) they are cut from float renderings on the host.
    request = None
    if previews and _gpu() is not None:
        request = PreviewRequest(config, preview_target, preview_result,
                                 (file_encoding(preview_target), file_encoding(preview_result)))
    deliveries = DeliveryRequest.for_results(results)
    needs, encodings = renderings_wanted(results)
    if previews and request is None:
        encodings = None                     # (the previews are cut from float renderings on the host)
    extra = {"preview": request} if request is not None else {}
    if loudness is not None:
        extra["loudness"] = loudness
    if deliveries:
        extra["deliveries"] = deliveries
    if eq is not None:
        extra["eq"] = eq
    if audit is not None:
        extra["audit"] = audit
    if visuals is not None:
        extra["visuals"] = visuals
    if repair is not None:
        extra["repair"] = repair
    # (main releases the resident frames)
    renderings = main(target_track.for_main, reference_audio, config, *needs, encodings=encodings, **extra)
    del reference_audio

    debug_line()
    info(Code.INFO_EXPORTING)
    if previews and request is None and any(_same_file(item.file, target) for item in results):
        # the target may be a read-only mapping of its file (audio_io.read_wav): a result written over that
        # file would pull the mapping from under the preview cut below
        target_audio = np.array(target_audio, copy=True)
    write_results(results, renderings, config.internal_sample_rate, deliveries)

    if request is not None:
        save_previews(request, config, preview_target, preview_result)
    elif previews:
        mastered = next((audio for audio in renderings if audio is not None), None)
        if mastered is None:                                   # every result is a delivery: the first of them
            mastered = pcm_to_float(deliveries.arrays[results[0].file])
        create_preview(pcm_to_float(target_audio), mastered, config, preview_target, preview_result)

    debug_line()
    info(Code.INFO_COMPLETED)
