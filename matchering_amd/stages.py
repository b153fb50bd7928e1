"""``main``: the drop-in for matchering/stages.py:210-272.

Same call signature and return convention as the reference -- two (n, 2) arrays
in, a triple ``(result, result_no_limiter, result_no_limiter_normalized)`` out
with ``None`` for outputs that were not requested -- but the four stages run as
HIP kernels on an MI355X through ``mgx_master`` (include/mgx.h).  Arrays come
back as float32 (n, 2) C-ordered; the reference returns float64.  The progress
codes 2004-2007 are emitted in the reference's order (stages.py:52,117,147,182)
and the per-stage scalars it prints through ``debug`` are reported from the
device-side values.
"""

import numpy as np

from .config import Config
from .device import DeviceFrames, default_device
from .log import Code, debug, debug_line, info
from .utils import to_db


PCM_BITS = {"PCM_16": 16, "PCM_24": 24, "PCM_32": 32}


def _as_frames(array, name):
    """(n, 2) frames as they will cross PCIe: float32, or the integer PCM of a file as it is (int16 / int32,
    or packed 24-bit uint8 (n, 6), audio_io): those are decoded on the device."""
    if isinstance(array, DeviceFrames):                  # uploaded by the caller already
        return array
    array = np.asarray(array)
    if array.dtype == np.uint8:                          # packed 24-bit PCM
        if array.ndim != 2 or array.shape[1] != 6:
            raise ValueError(f"{name} must hold (n, 2) packed 24-bit frames, got {array.shape}")
        return np.ascontiguousarray(array)
    if array.ndim != 2 or array.shape[1] != 2:
        raise ValueError(f"{name} must have shape (n, 2), got {array.shape}")
    if array.dtype in (np.int16, np.int32):
        return np.ascontiguousarray(array)
    return np.ascontiguousarray(array, dtype=np.float32)


def _is_profile(reference):
    from .profile import ReferenceProfile

    return isinstance(reference, ReferenceProfile)


def _limited(dev, rendering, n, rate, delivery, bits, measured):
    """The passes of a delivery's limiter (``mgx_tp_limit``, each from the rendering itself, each metered) as
    ``mgx_delivery_limit_step`` asks for them: ``(Delivered, the last pass's frames)``, or None where it asks for none.
    The record is ``mgx_delivery_gain``'s on the measurement of those frames (for a noise-shaped delivery both are the
    ``_shaped`` entry points: ``delivery.limit_step`` and ``delivery.delivery_gain`` choose)."""
    from dataclasses import replace

    from .delivery import delivery_gain, limit_step

    lookahead, release = delivery.limiter.frames(rate)
    pre, loud, scratch, reading, worst = [], [], None, None, 0.0
    try:
        while True:
            run, pre_gain_db, ceiling = limit_step(delivery, bits, measured, pre, loud)
            if not run:
                break
            scratch, worst = dev.tp_limit(rendering, n, 10.0 ** (pre_gain_db / 20.0), ceiling, lookahead, release, out=scratch)
            reading = dev.loudness(scratch, n, rate)
            pre.append(pre_gain_db)
            loud.append(reading.integrated)
        if not pre:
            return None
        record = replace(delivery_gain(delivery, bits, reading), measured=measured, limiter_passes=len(pre), pre_gain_db=pre[-1],
                         max_reduction_db=20.0 * float(np.log10(1.0 - worst)), limited=reading)
    except Exception:
        if scratch is not None:
            scratch.release()
        raise
    return record, scratch


def main(target: np.ndarray, reference: np.ndarray, config: Config, need_default: bool = True,
         need_no_limiter: bool = False, need_no_limiter_normalized: bool = False, device=None, fir=None,
         encodings=None, preview=None, loudness=None, deliveries=None, eq=None, audit=None, visuals=None, repair=None):
    # (``device``: the handle to run on, default the process-wide one; ``fir``: a DeviceBuffer with a
    # matching FIR to apply instead of designing one -- batch.master_album; ``encodings``: per output,
    # None for float32 frames or "PCM_16" / "PCM_24" / "PCM_32" for the integer samples a file of that
    # subtype holds, quantised on the device (saver.py:27-33 does it on the host) -- int16 / int32 (n, 2),
    # or uint8 (n, 6) for packed 24-bit.  All additions to the reference's signature, keyword-only in
    # spirit.  ``target`` / ``reference`` may be int16 or int32 PCM as read from a file.  ``preview``: a
    # preview.PreviewRequest -- the A/B previews of preview_creator.py:30-94 are cut from the first requested
    # output and from the target while both are still in HBM, and left in the request.  ``reference`` may be a
    # profile.ReferenceProfile: the reference's analysis results without its audio, made with this Config --
    # mgx_master_with_profile; stage 1 then runs on the target alone.  ``loudness``: a callable that receives
    # (name, loudness.Loudness) for "target", for "reference" when its audio is here, and for each requested output --
    # "result", "result_no_limiter", "result_no_limiter_normalized" -- measured on the float frames in HBM
    # (mgx_loudness), before any encoding; None: nothing is measured.  ``deliveries``: a delivery.DeliveryRequest --
    # renditions of the renderings at a loudness target, under a true-peak ceiling, dithered (mgx_delivery_gain,
    # mgx_deliver), made while the renderings are still in HBM and left in the request; a rendering that only a delivery
    # names is computed but not returned, and ``loudness`` also receives ("delivered:" + key, delivery.Delivered).  A
    # delivery that carries a limiter and whose ceiling binds is limited first (mgx_tp_limit, mgx_delivery_limit_step).  A
    # noise-shaped delivery takes the _shaped policy and mgx_deliver_shaped in their place.  A
    # delivery at another ``sample_rate`` than the internal one is made from the rendering converted to that rate in HBM
    # (mgx_convert_rate) and measured there; the renderings returned, the previews and the other callbacks do not change.
    # ``eq``: an eq.MatchingEq (or its JSON object) -- how much of the matching curve is applied, its boost and cut
    # caps, the FIR's phase (mgx_master_shaped); None: the reference's FIR.  A given ``fir`` is used as given.
    # ``audit``: a callable that receives (name, qc.Audit) for the names ``loudness`` receives -- the quality-control pass
    # (mgx_audit) over the float frames in HBM -- and for "delivered:" + key the audit of the buffer mgx_deliver /
    # mgx_deliver_shaped wrote, at the delivery's own rate and width, before it is downloaded: the file as written.  None:
    # nothing is launched.
    # ``visuals``: a callable, or a pair (callable, visuals.VisualsRequest) giving the sizes, that receives (name,
    # visuals.Visuals) -- the waveform overview and the spectrogram (mgx_overview, mgx_spectrogram) of the float frames
    # in HBM -- for the names ``audit`` receives for float frames.  None: nothing is launched.
    # ``repair``: a repair.ClipRepair, its JSON (True or an object), or a pair (callable, ClipRepair) whose callable
    # receives ("target", repair.Repaired) -- the target's short runs at the rail are rebuilt (mgx_declip) into a NEW buffer
    # right after upload, and that buffer is what the master step sees on every route (plain, ``eq``, ``fir``, a profile),
    # what the "target" callbacks of ``loudness`` / ``audit`` / ``visuals`` measure and what the target's preview is cut
    # from; the frames the caller handed in are not written (resident ``DeviceFrames`` are released at the end, as they
    # are without a repair; the new buffer is released with the outputs, on error too).  The repair is queued in front
    # of the master call and its report read behind it, where main has waited anyway: an explicit ``level`` adds no wait;
    # with ``level=None``, the default, the level comes from the track's own peak (Device.peak_count), which does wait
    # once in front of the master call.  None or False: nothing is launched.)
    from .eq import as_eq
    from .repair import as_repair

    notify_repair, repair = as_repair(repair)                # (ValueError before anything reaches the GPU)
    eq = as_eq(eq)
    if eq is not None:
        eq.check(config)                                     # (ValueError before anything reaches the GPU)
    dev = device if device is not None else default_device()
    target = _as_frames(target, "target")
    profile = reference if _is_profile(reference) else None
    if profile is not None:
        profile.matches(config)                              # (ValueError before anything reaches the GPU)
        reference, nr = None, 0
    else:
        reference = _as_frames(reference, "reference")
        nr = reference.shape[0]
    n = target.shape[0]
    native = config.to_native()
    if deliveries:
        # (ValueError before anything reaches the GPU: a rate pair mgx_convert_rate refuses has no other route)
        deliveries.check_rates(config.internal_sample_rate, n)

    debug_line()
    info(Code.INFO_MATCHING_LEVELS)
    debug(f"analysis pieces: at most {config.max_piece_size} frames "
          f"({config.max_piece_size / config.internal_sample_rate:.2f} s) each")
    with dev.lock:
        t_dev = target.buf if isinstance(target, DeviceFrames) else dev.upload_frames(target)
        if profile is not None:
            r_dev, p_dev = None, profile.resident(dev)       # (the profile's own buffer: kept, not released here)
        else:
            r_dev, p_dev = (reference.buf if isinstance(reference, DeviceFrames) else dev.upload_frames(reference)), None
        returned = (need_default, need_no_limiter, need_no_limiter_normalized)
        cut = deliveries.needs() if deliveries else (False, False, False)
        outs = [dev.alloc(n * 8) if need or extra else None for need, extra in zip(returned, cut)]
        uploaded, fixed = t_dev, None
        try:
            if repair is not None:
                from .repair import finish, queue

                fixed, rail = queue(dev, t_dev, n, repair)
                if fixed is not None:
                    t_dev = fixed                                # (from here on "the target" is the repaired buffer)
            route = {} if p_dev is None else {"profile": p_dev}
            if eq is not None:
                route["eq"] = eq
            report = dev.master(t_dev, n, r_dev, nr, native, *outs, fir=fir, **route)
            if repair is not None:
                found = finish(dev, fixed, rail, n)
                debug(found.describe())
                if notify_repair is not None:
                    notify_repair("target", found)
            debug(f"target: {report.target_divisions} pieces of {report.target_piece} frames, "
                  f"{report.target_loud_count} of them loud; reference: {report.reference_divisions} pieces of "
                  f"{report.reference_piece} frames, {report.reference_loud_count} loud")
            if not np.isclose(report.final_amplitude_coefficient, 1.0):
                debug("the reference peaks below the threshold: it was scaled up for matching and the result "
                      f"is scaled back by {to_db(report.final_amplitude_coefficient)}")
            debug(f"level match: {to_db(report.rms_coefficient)} on the target")
            debug_line()
            info(Code.INFO_MATCHING_FREQS)
            if eq is not None and fir is None:
                debug(eq.describe())
            debug_line()
            info(Code.INFO_CORRECTING_LEVELS)
            kept = len(report.correction_coefficients)               # (mgx_report keeps the first 16 coefficients)
            for step in range(min(config.rms_correction_steps, kept)):
                debug(f"correction round {step + 1}: {to_db(report.correction_coefficients[step])}")
            if config.rms_correction_steps > kept:
                debug(f"... and {config.rms_correction_steps - kept} more rounds")
            debug_line()
            info(Code.INFO_FINALIZING)
            if need_no_limiter_normalized:
                debug(f"unlimited result normalised by {to_db(report.normalize_coefficient)} to reach the threshold")
            if need_default and not report.limiter_active:
                debug("the result stays under the threshold: the limiter passes it through")
            rate = config.internal_sample_rate
            metered = {}                                         # rendering -> its measurement: one per rendering
            if loudness is not None:
                loudness("target", dev.loudness(t_dev, n, rate))
                if r_dev is not None:
                    loudness("reference", dev.loudness(r_dev, nr, rate))
                for slot, name in enumerate(("result", "result_no_limiter", "result_no_limiter_normalized")):
                    if returned[slot]:
                        metered[slot] = dev.loudness(outs[slot], n, rate)
                        loudness(name, metered[slot])
            if audit is not None:
                audit("target", dev.audit(t_dev, n, rate))
                if r_dev is not None:
                    audit("reference", dev.audit(r_dev, nr, rate))
                for slot, name in enumerate(("result", "result_no_limiter", "result_no_limiter_normalized")):
                    if returned[slot]:
                        audit(name, dev.audit(outs[slot], n, rate))
            if visuals is not None:
                from .visuals import handler_of, make

                draw, sizes = handler_of(visuals)
                draw("target", make(dev, t_dev, n, rate, sizes))
                if r_dev is not None:
                    draw("reference", make(dev, r_dev, nr, rate, sizes))
                for slot, name in enumerate(("result", "result_no_limiter", "result_no_limiter_normalized")):
                    if returned[slot]:
                        draw(name, make(dev, outs[slot], n, rate, sizes))
            if deliveries:
                from dataclasses import replace

                from .delivery import DITHERS, SUBTYPE_BITS, delivery_gain

                # a delivery at another rate is cut from the rendering CONVERTED to that rate (mgx_convert_rate), measured
                # at that rate: once per (rendering, rate), shared by every delivery that names the pair
                converted, at_rate = {}, {}
                try:
                    for key, slot, subtype, delivery in deliveries.items:
                        out_rate = delivery.rate(rate)
                        if out_rate == rate:
                            if slot not in metered:
                                metered[slot] = dev.loudness(outs[slot], n, rate)
                            source, length, reading = outs[slot], n, metered[slot]
                        else:
                            pair = (slot, out_rate)
                            if pair not in converted:
                                converted[pair] = dev.convert_rate(outs[slot], n, rate, out_rate)
                                at_rate[pair] = dev.loudness(converted[pair].buf, converted[pair].frames, out_rate)
                            source, length, reading = converted[pair].buf, converted[pair].frames, at_rate[pair]
                        bits = SUBTYPE_BITS.get(subtype, 0)          # (float subtypes: float32 frames)
                        limited = None
                        if delivery.limiter is not None:
                            # (None where the ceiling does not bind: the delivery then takes the route of one without a limiter)
                            limited = _limited(dev, source, length, out_rate, delivery, bits, reading)
                        if limited is None:
                            record, frames = delivery_gain(delivery, bits, reading), source
                        else:
                            record, frames = limited
                        record = replace(record, sample_rate=out_rate, frames=length, internal_rate=rate)
                        deliveries.delivered[key] = record
                        # queued behind the measurement; the array is valid after the one wait below
                        written = {}
                        if audit is not None:            # the buffer the kernel wrote, audited before it is downloaded
                            written["inspect"] = lambda b, k=key, m=length, r=out_rate, w=bits: audit(
                                "delivered:" + str(k), dev.audit(b, m, r, w))
                        try:
                            if delivery.shaped:          # (the policy above was the _shaped one: delivery.delivery_gain)
                                deliveries.arrays[key] = dev.deliver_shaped(frames, length, record.gain, bits, delivery.shaper,
                                                                            delivery.seed, wait=False, **written)
                            else:
                                deliveries.arrays[key] = dev.deliver(frames, length, 2, record.gain, bits,
                                                                     DITHERS[delivery.dither], delivery.seed, wait=False, **written)
                        finally:
                            if limited is not None:
                                frames.release() # (recycled by later work on this stream only, which is ordered behind the kernel)
                        if loudness is not None:
                            loudness("delivered:" + str(key), record)
                finally:
                    for frames in converted.values():
                        frames.release()         # (likewise: on every path, an exception's included)
            # queued one behind the other, then ONE wait; the arrays live in pinned host memory
            formats = encodings if encodings is not None else (None, None, None)
            pieces = []
            if preview is not None:
                # core.py:111: the first rendering there is (one that only a delivery asked for comes last)
                mastered = next((b for b, need in zip(outs, returned) if need), None) or next(b for b in outs if b is not None)
                begin, size, fade = preview.plan(dev.window_energy(mastered, n, preview.size, preview.step), n)
                for want, src, limit, fmt in ((preview.want_target, t_dev, preview.threshold, preview.encodings[0]),
                                              (preview.want_result, mastered, 0.0, preview.encodings[1])):
                    piece = dev.preview_cut(src, n, begin, size, fade, limit) if want else None
                    pieces.append(piece)
                    host = (None if piece is None else dev.download(piece, (size, 2), wait=False) if fmt is None
                            else dev.download_pcm(piece, size, 2, PCM_BITS[fmt], wait=False))
                    if src is t_dev:
                        preview.target_piece = host
                    else:
                        preview.result_piece = host
            results = tuple(None if not need
                            else dev.download(b, (n, 2), wait=False) if fmt is None
                            else dev.download_pcm(b, n, 2, PCM_BITS[fmt], wait=False)
                            for b, fmt, need in zip(outs, formats, returned))
            dev.synchronize()
            for piece in pieces:
                if piece is not None:
                    piece.release()
        finally:
            for b in (uploaded, fixed, r_dev, *outs):
                if b is not None:
                    b.release()
    return results
