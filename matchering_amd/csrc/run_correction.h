// Stage 3 on the host side: the level correction's rounds (correction_kernels.h).
#pragma once

#include "handle.h"
#include "run_limiter.h"               // limiter_state: round 0 presets the limiter's look-back words

static const char* const TOO_MANY_PIECES ="too many analysis pieces for the level-correction kernel's LDS";

// Stage 3 (stages.py:138-170), every round queued on the handle's stream: one launch per round, the last round also
// derives the peak / early-out / normalisation scalars.  `nblocks`: the per-pair peaks the convolution left in
// h->block_peak.  `lp`: the limiter's parameters when a limited result follows, else null; round 0's grid then presets
// the limiter's look-back words (`*limiter_preset`).  `reference_match_rms`, `reference_amplitude_c`: device addresses
// of the reference's two scalars (the reference's TrackStats, or a profile's header).
// The first launch here (round 0, or k_finalize_scalars where there are no rounds) is the last of the call that touches
// its context `cx`: it starts from cx.cstate, as the front half reset it, and fills the handle's BackState, where every
// later launch of the back half reads and writes.  `released` (or null) is recorded right behind it.
static int run_correction(mgx_handle* h, const mgx_config* cfg, const CallContext& cx, const double* reference_match_rms,
                          const double* reference_amplitude_c, long long n_target, long long nblocks,
                          const LimiterParams* lp, bool* limiter_preset, hipEvent_t released) {
    const TrackWork& tw = cx.track[0];
    MGX_TRY(ensure(h, h->back, sizeof(BackState)));
    BackState* back = (BackState*)h->back.p;
    CorrectionState* cs = &back->cs;
    RoundArgs ra;
    ra.mid = (const float*)h->mid.p;
    ra.piece = tw.piece;
    ra.divisions = tw.divisions;
    ra.chunks = std::max(1, 1024 / tw.divisions);     // ~1000 workgroups: each pays one publish + ticket
    // (round 0's partial sums, and behind them the peak words of k_correction_tail's workgroups)
    MGX_TRY(ensure(h, h->partial, (size_t)2 * ra.divisions * ra.chunks * sizeof(double)));
    ra.partial = (double*)h->partial.p;
    // arrival counters [1 + divisions], zero between launches; the 16 gain words of k_correction_tail
    // live in their own buffer (a layout that moved with `divisions` would leave one call's preset
    // gain words where the next call counts arrivals)
    const size_t ctr_bytes = (size_t)(1 + ra.divisions) * sizeof(unsigned);
    // at most ~128 workgroups in k_correction_tail, at most 64 chunks (the lanes of a wave) per workgroup
    const int tail_groups = std::max((ra.chunks + 63) / 64, std::max(1, std::min(ra.chunks, 128 / ra.divisions)));
    const bool use_tail = cfg->rms_correction_steps > 1 && !h->avoid_tail;
    const int tail_total = use_tail ? ra.divisions * tail_groups : 0;
    const int tail_rounds = use_tail ? cfg->rms_correction_steps - 1 : 0;
    MGX_TRY(ensure(h, h->tail_gains, ((size_t)tail_rounds + 1 + (size_t)tail_rounds * tail_total) * sizeof(unsigned long long)));
    ra.tail_total = tail_total;
    ra.tail_rounds = tail_rounds;
    if (h->round_ctr.bytes < ctr_bytes) {                 // zeroed when (re)allocated, reset by each launch
        MGX_TRY(ensure(h, h->round_ctr, std::max(ctr_bytes, (size_t)4096)));
        HIP_TRY(hipMemsetAsync(h->round_ctr.p, 0, h->round_ctr.bytes, h->stream));
    }
    ra.arrivals = (unsigned*)h->round_ctr.p;
    const size_t wgs = (size_t)ra.divisions * ra.chunks;
    MGX_TRY(ensure(h, h->band, ((size_t)n_target + wgs * BAND_SLACK) * sizeof(float)));
    MGX_TRY(ensure(h, h->band_info, wgs * sizeof(BandInfo)));
    ra.band = (float*)h->band.p;
    ra.info = (BandInfo*)h->band_info.p;
    ra.reference_match_rms = &back->reference_match_rms;
    ra.front_cs = nullptr;
    ra.front_amplitude_c = nullptr;
    ra.back_refs = nullptr;
    ra.eps = cfg->min_value;
    ra.threshold = cfg->threshold;
    ra.cs = cs;
    ra.npeaks = nblocks;
    MGX_TRY(ensure_ctrl(h));
    ra.error = h->error_dev;
    const size_t lds_step = (size_t)(64 + tw.divisions + (size_t)ra.divisions * ra.chunks) * sizeof(double);
    if (lds_step > LDS_PER_WORKGROUP_MAX) return fail(MGX_ERR_UNSUPPORTED, TOO_MANY_PIECES);
    MGX_TRY(allow_lds(k_correction_round, lds_step));
    const int rounds = cfg->rms_correction_steps;
    ra.lim_published = nullptr;
    ra.lim_words = 0;
    ra.lim_ticket = nullptr;
    ra.tail_gains = use_tail ? (unsigned long long*)h->tail_gains.p : nullptr;
    if (rounds >= 1) {                                    // round 0 streams the mid plane and builds the band lists
        RoundArgs r0 = ra;
        r0.final_peaks = rounds == 1 ? (const float*)h->block_peak.p : nullptr;    // (the launch of the last round)
        r0.build_band = 1;
        r0.step = 0;
        r0.reference_match_rms = reference_match_rms;
        r0.front_cs = (const CorrectionState*)cx.cstate.p;
        r0.front_amplitude_c = reference_amplitude_c;
        r0.back_refs = &back->reference_match_rms;
        if (lp) {     // the limiter's look-back words are preset by this grid: a thousand workgroups, two words a thread
            MGX_TRY(limiter_state(h, n_target, *lp, &r0.lim_published, &r0.lim_words, &r0.lim_ticket));
            *limiter_preset = true;
        }
        hipLaunchKernelGGL(k_correction_round, dim3(ra.divisions * ra.chunks), dim3(256), lds_step, h->stream, r0);
        if (released) HIP_TRY(hipEventRecord(released, h->stream));
    }
    if (rounds > 1 && !use_tail) {
        // one launch per round, the last arriver of each decides (k_correction_round without a tail): what a handle
        // falls back to after its tail kernel found the GPU shared (check_device_error), and MGX_NO_TAIL=1
        for (int r = 1; r < rounds; ++r) {
            RoundArgs rr = ra;
            rr.build_band = 0;
            rr.step = r;
            rr.final_peaks = r == rounds - 1 ? (const float*)h->block_peak.p : nullptr;
            hipLaunchKernelGGL(k_correction_round, dim3(ra.divisions * ra.chunks), dim3(256), lds_step, h->stream, rr);
        }
    }
    if (use_tail) {                                       // every further round inside one small resident grid
        RoundArgs rt = ra;
        rt.build_band = 0;
        rt.step = 1;
        rt.final_peaks = (const float*)h->block_peak.p;
        const int groups = tail_groups;
        const size_t lds_tail = correction_tail_lds_bytes(ra.divisions, groups, ra.chunks);
        if (lds_tail > LDS_PER_WORKGROUP_MAX) return fail(MGX_ERR_UNSUPPORTED, TOO_MANY_PIECES);
        MGX_TRY(allow_lds(k_correction_tail, lds_tail));
        // (+ 1: the deciding workgroup)
        hipLaunchKernelGGL(k_correction_tail, dim3(ra.divisions * groups + 1), dim3(256), lds_tail, h->stream, rt, groups,
                           rounds - 1);
    }
    if (rounds == 0) {
        hipLaunchKernelGGL(k_finalize_scalars, dim3(1), dim3(256), 0, h->stream, (const float*)h->block_peak.p,
                           nblocks, cfg->threshold, cfg->min_value, cs, (const CorrectionState*)cx.cstate.p,
                           reference_match_rms, reference_amplitude_c, &back->reference_match_rms);
        if (released) HIP_TRY(hipEventRecord(released, h->stream));
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
