// What the host does about the error words the kernels raise (wave_util.h): report, recover, queue the call again.
#pragma once

#include "handle.h"

// one stages.main: every launch queued on the handle's stream (master_call.h; check_device_error may queue the last
// call again)
static int queue_master(mgx_handle* h, const mgx_handle::MasterCall& c, const MasterPlan& plan);

// A bounded device-side wait expired (never seen in normal operation; the spins are bounded so that a lost word
// cannot hang the GPU, and the audio behind such a wait is wrong).  Called by every entry point that has just
// waited for the stream -- with or without a report -- so that the failure cannot pass silently; the flag is host
// memory, reading it costs nothing.  The counters a timed-out kernel may have left half-counted are put back, so
// the handle is good for the next call.
//   * DEVICE_ERROR_TAIL: k_correction_tail's workgroups (<= 129, spinning on each other's flag words) were not
//     resident together -- something else held the compute units.  Not a lost word: the last mgx_master call is
//     queued again with rounds 1..K-1 as one launch each (they wait for nobody), the handle stays that way, and the
//     call succeeds; mgx_last_error() carries a note.
//   * anything else (a limiter look-back word that never came): MGX_ERR_HIP.
// `may_requeue`: the caller has not yet handed anything of the failed run to the host (master_impl before its report
// is read, mgx_synchronize / mgx_stage_times with no download queued behind the call, the blocking copy that re-issues
// itself).  Everywhere else -- and whenever MORE than one mgx_master call is outstanding since the last
// synchronisation, or a download of its outputs is already queued behind it (only the last call could be run again,
// and a copy would have taken the failed run's frames) -- an expired tail fails like any other expired wait; the handle
// still switches to one launch per round, so the caller's retry succeeds.
// `whose`: what the caller handed in, for the report of a NaN or an infinity ("the frames to measure"); null: a pair.
static int check_device_error(mgx_handle* h, bool may_requeue = false, const char* whose = nullptr) {
    h->requeued = false;
    const int outstanding = h->masters_outstanding;
    const int copies = h->downloads_outstanding;
    const bool by_number = h->limiter_ran_by_number;
    h->masters_outstanding = 0;
    h->downloads_outstanding = 0;
    h->limiter_ran_by_number = false;
    if (!h->error_host) return 0;
    volatile int* e = (volatile int*)h->error_host;
    const int what = (e[DEVICE_ERROR_SLOT_LOOKBACK] ? DEVICE_ERROR_LOOKBACK : 0) | (e[DEVICE_ERROR_SLOT_TAIL] ? DEVICE_ERROR_TAIL : 0) |
                     (e[DEVICE_ERROR_SLOT_INPUT] ? DEVICE_ERROR_INPUT : 0) | (e[DEVICE_ERROR_SLOT_PROFILE] ? DEVICE_ERROR_PROFILE : 0);
    if (what == 0) return 0;
    const int profile_field = e[DEVICE_ERROR_SLOT_PROFILE];
    for (int i = 0; i < DEVICE_ERROR_SLOTS; ++i) e[i] = 0;
    if (h->round_ctr.p) HIP_TRY(hipMemsetAsync(h->round_ctr.p, 0, h->round_ctr.bytes, h->stream));
    if (h->lim_ctrl.p) HIP_TRY(hipMemsetAsync(h->lim_ctrl.p, 0, 64, h->stream));
    if (h->conv_queue.p) HIP_TRY(hipMemsetAsync(h->conv_queue.p, 0, 64, h->stream));
    MGX_TRY(sync_main(h));
    if (what & DEVICE_ERROR_PROFILE) {
        // (before the input report: a profile that was not read makes no statement about anybody's samples)
        // (k_profile_merge: the verdict in the low byte, the refused source's position + 1 above it)
        static const char* const FIELDS[] = {"", "magic", "version", "internal_sample_rate", "fft_size", "max_piece_size",
                                             "threshold", "min_value", "loud_count"};
        const int verdict = profile_field & 0xff, source = profile_field >> 8;
        const char* field = verdict > 0 && verdict < 9 ? FIELDS[verdict] : "header";
        const std::string whose = source > 0 ? "the reference profile, source " + std::to_string(source - 1) + " of the merge,"
                                             : "the reference profile";
        return fail(MGX_ERR_ARGUMENT, whose + " does not fit this call: its " + field +
                                      (verdict <= PROFILE_BAD_VERSION
                                           ? " is not that of a profile this library writes (mgx_profile_header)"
                                       : verdict == PROFILE_BAD_COUNT
                                           ? " is not positive or exceeds its divisions, or the merged counts do not fit 32 bits"
                                           : " differs from the Config's; a profile is used with the Config it was made with") +
                                      "; the outputs of the calls since the last synchronisation are not valid");
    }
    if ((what & DEVICE_ERROR_INPUT) && whose)
        return fail(MGX_ERR_ARGUMENT, std::string(whose) + " hold samples that are not finite numbers (NaN or infinity)");
    if (what & DEVICE_ERROR_INPUT)
        return fail(MGX_ERR_ARGUMENT, "the target or the reference holds samples that are not finite numbers (NaN or infinity): "
                                      "the reference fails on such input too (match_frequencies.py:42)");
    // What a handle can recover from, once each: an expired tail (its workgroups were not resident together -> one launch
    // per round from now on) and an expired limiter look-back while chunks were dealt by workgroup number (-> tickets from
    // now on).  Anything else, or the same again in the safer mode, is a lost word.
    const bool tail_new = (what & DEVICE_ERROR_TAIL) && !h->avoid_tail;
    // (by the mode the failed launches REALLY ran in: under MGX_LIMIT_TICKETS=1 the handle's own switch may still be
    // off while every launch drew tickets -- an expired wait is then a lost word, not something to run again)
    const bool lookback_new = (what & DEVICE_ERROR_LOOKBACK) && !h->limiter_tickets && by_number;
    const bool recoverable = (!(what & DEVICE_ERROR_TAIL) || tail_new) && (!(what & DEVICE_ERROR_LOOKBACK) || lookback_new);
    if (recoverable) {
        if (tail_new) h->avoid_tail = true;                      // whatever happens next, this handle stops using the tail
        if (lookback_new) h->limiter_tickets = true;
        if (may_requeue && h->last_call.valid && outstanding == 1 && copies == 0) {
            const mgx_handle::MasterCall again = h->last_call;
            MGX_TRY(drain(h));                                  // (serial replay: both streams idle, then main alone)
            MGX_TRY(queue_master(h, again, h->pipe.replay()));
            MGX_TRY(sync_main(h));
            h->masters_outstanding = 0;
            bool clean = true;
            for (int i = 0; i < DEVICE_ERROR_SLOTS; ++i) clean = clean && e[i] == 0;
            if (clean) {
                h->requeued = true;
                g_error = tail_new ? "note: the level-correction tail kernel's workgroups were not resident together (the GPU is shared); "
                                     "the call was run again with one launch per correction round, and this handle keeps doing so"
                                   : "note: a limiter look-back wait expired with chunks dealt by workgroup number; the call was run again "
                                     "with chunks drawn from an atomic ticket, and this handle keeps doing so";
                return 0;
            }
            for (int i = 0; i < DEVICE_ERROR_SLOTS; ++i) e[i] = 0;
        } else {
            return fail(MGX_ERR_RETRY, tail_new
                ? "the level-correction tail kernel's workgroups were not resident together (the GPU is shared) and "
                  "the results of the mgx_master calls since the last synchronisation are not valid; this handle now "
                  "runs one launch per correction round: call again"
                : "a limiter look-back wait expired with chunks dealt by workgroup number and the results of the calls since the "
                  "last synchronisation are not valid; this handle now draws chunks from an atomic ticket: call again");
        }
    }
    return fail(MGX_ERR_HIP, "a bounded device-side wait expired (limiter look-back or level-correction round): "
                             "the results of the calls since the last synchronisation are not valid");
}
