// The boundary, stages.main: the executor of the call pipeline's plans (call_pipeline.h) -- every launch of a master
// call, and the entry point's work around them.
#pragma once

#include <cstring>

#include "device_errors.h"
#include "handle.h"
#include "run_analysis.h"
#include "run_conv.h"
#include "run_correction.h"
#include "run_fir.h"
#include "run_limiter.h"

// every launch of one stages.main (no host round trip): the front half on main or, for a pipelined call, on the
// front stream behind the waits `plan` asks for; the back half on main
static int queue_master(mgx_handle* h, const mgx_handle::MasterCall& c, const MasterPlan& plan) {
    // (c.out: result, result_no_limiter, result_no_limiter_normalized; null: not wanted)
    // stage 1 (stages.py:38-104): both tracks analysed in one pass each -- or the target alone, against a profile
    CallContext& cx = h->ctx[plan.context];
    TrackWork& tw = cx.track[0];
    TrackWork& rw = cx.track[1];
    // the front half's stream for the length of this call; whatever way out, the stage-level entry points find main
    struct FrontQueue {
        mgx_handle* h;
        ~FrontQueue() { h->fq = h->stream; }
    } front_queue{h};
    if (plan.pipelined) {
        h->fq = h->front;
        // (a) the context's previous user, call k - 2, has let go of it: round 0 of its level correction has finished.
        // Its tail, scale kernel and limiter may still be running or waiting: they touch the BackState only.
        if (plan.wait_context) HIP_TRY(hipStreamWaitEvent(h->front, h->ctx_released[plan.context], 0));
        if (plan.wait_main) {                                                                                // (b)
            HIP_TRY(hipEventRecord(h->main_now, h->stream));
            HIP_TRY(hipStreamWaitEvent(h->front, h->main_now, 0));
        }
    }
    // where stages 3 and 4 read the reference's two scalars: its TrackStats, or the profile's header
    const double* reference_match_rms = c.profile ? &c.profile->match_rms : nullptr;
    const double* reference_amplitude_c = c.profile ? &c.profile->amplitude_coefficient : nullptr;
    // (analysing the reference first, so that the target is the fresher track in the Infinity Cache when
    // the convolution reads it, was measured: no difference)
    {
        StageScope scope(h, MGX_STAGE_ANALYZE);
        tw.is_reference = 0;
        if (c.profile) {
            MGX_TRY(run_analysis(h, &c.cfg, c.target, c.n_target, tw));
        } else {
            rw.is_reference = 1;
            MGX_TRY(run_analysis(h, &c.cfg, c.target, c.n_target, tw, c.reference, c.n_reference, &rw));
            reference_match_rms = &((const TrackStats*)rw.stats.p)->match_rms;      // (allocated by the line above)
            reference_amplitude_c = &((const TrackStats*)rw.stats.p)->amplitude_c;
        }
    }
    // stage 2 (stages.py:107-135): FIR design on the device, then the overlap-save convolution with
    // the level gain of stages.py:80-88 (a device scalar) folded into the filter spectra
    {
        StageScope scope(h, MGX_STAGE_DESIGN_FIR);
        MGX_TRY(run_fir_design(h, &c.cfg, tw, rw, c.fir_given, c.profile, c.shaped ? &c.shape : nullptr,
                               c.toned ? &c.tone : nullptr));
    }
    MGX_TRY(ensure(h, h->y, (size_t)c.n_target * sizeof(float2)));
    MGX_TRY(ensure(h, h->mid, (size_t)c.n_target * sizeof(float)));
    long long nblocks = 0;
    MGX_TRY(run_conv(h, c.target, c.n_target, c.cfg.fft_size, (const float*)cx.taps.p, 1.0, (float*)h->y.p,
                     (float*)h->mid.p, &nblocks, (const double*)cx.scalars.p, CONV_SPECTRA));
    if (plan.pipelined) {       // (c) the front half ends here, (d) the back half follows it on main
        HIP_TRY(hipEventRecord(h->front_done[plan.context], h->front));
        HIP_TRY(hipStreamWaitEvent(h->stream, h->front_done[plan.context], 0));
        h->fq = h->stream;
    }
    MGX_TRY(run_conv(h, c.target, c.n_target, c.cfg.fft_size, (const float*)cx.taps.p, 1.0, (float*)h->y.p,
                     (float*)h->mid.p, &nblocks, (const double*)cx.scalars.p, CONV_MAIN));
    // stage 3 (stages.py:138-170): scalar feedback stays on the device (the state was reset by k_fir_raw).  Its first
    // launch is the last that touches `cx`; the context is released behind it, and from here on the call works in the
    // handle's BackState.
    bool limiter_preset = false;
    {
        StageScope scope(h, MGX_STAGE_CORRECT_LEVELS);
        MGX_TRY(run_correction(h, &c.cfg, cx, reference_match_rms, reference_amplitude_c, c.n_target, nblocks,
                               c.out[0] ? &c.lp : nullptr, &limiter_preset,
                               plan.record_back && h->front ? h->ctx_released[plan.context] : nullptr));
    }
    const BackState* back = (const BackState*)h->back.p;
    const CorrectionState* cs = &back->cs;
    // stage 4 (stages.py:173-207)
    if (c.out[1] || c.out[2]) {
        StageScope scope(h, MGX_STAGE_SCALE_OUTPUTS);
        const unsigned grid = (unsigned)std::min<long long>((c.n_target + 255) / 256, 8192);
        hipLaunchKernelGGL(k_scale_outputs, dim3(grid), dim3(256), 0, h->stream, (const float2*)h->y.p,
                           (long long)c.n_target, (const double*)&cs->gain, 1.0, (const double*)&cs->normalize_c,
                           (float2*)c.out[1], (float2*)c.out[2]);
        HIP_TRY(hipGetLastError());
    }
    if (c.out[0]) {
        StageScope scope(h, MGX_STAGE_LIMIT);
        MGX_TRY(run_limiter(h, (const float*)h->y.p, c.n_target, c.lp, c.cfg.threshold, &cs->gain,
                            &back->reference_amplitude_c, &cs->limiter_active, c.out[0], limiter_preset));
    }
    return 0;
}

// the reference: `reference_dev` (n_reference frames), or `profile` with reference_dev null
static int master_impl(mgx_handle* h, const float* target_dev, int64_t n_target, const float* reference_dev,
                       int64_t n_reference, const mgx_profile_header* profile, const mgx_config* cfg,
                       const float* fir_given, float* result_dev, float* result_no_limiter_dev,
                       float* result_no_limiter_normalized_dev, mgx_report* report, const mgx_eq_shape* shape = nullptr,
                       const mgx_eq_tone* tone = nullptr) {
    if (!h || !target_dev || (!reference_dev && !profile)) return fail(MGX_ERR_ARGUMENT, "null argument");
    MGX_TRY(check_config(cfg));
    if (tone) MGX_TRY(mgx_eq_tone_check(cfg, shape, tone));   // (refused by name before anything is queued)
    else if (shape) MGX_TRY(mgx_eq_shape_check(cfg, shape));
    if (eq_tone_neutral(tone)) tone = nullptr;                  // the call without a tone: today's route
    const mgx_eq_shape tone_alone{1.0, std::nan(""), std::nan(""), 0, 0};
    if (tone && !shape) shape = &tone_alone;                    // (a NULL shape with a tone: amount 1, no caps, linear phase)
    HIP_TRY(hipSetDevice(h->device));
    LimiterParams lp{};
    if (result_dev) {               // derived (and validated) once, before any work is queued
        const std::string err = limiter_params(*cfg, lp);
        if (!err.empty()) return fail(MGX_ERR_UNSUPPORTED, err);
    }
    mgx_handle::MasterCall& call = h->last_call;
    call.valid = false;
    call.lp = std::move(lp);
    call.target = target_dev;
    call.reference = reference_dev;
    call.fir_given = fir_given;
    call.profile = profile;
    call.n_target = n_target;
    call.n_reference = n_reference;
    call.cfg = *cfg;
    call.shaped = shape != nullptr;
    if (shape) call.shape = *shape;                             // (the call's own copy: the caller's may change behind it)
    call.toned = tone != nullptr;
    if (tone) call.tone = *tone;
    call.out[0] = result_dev;
    call.out[1] = result_no_limiter_dev;
    call.out[2] = result_no_limiter_normalized_dev;
    MasterRanges ranges;
    const size_t fir_bytes = (size_t)2 * cfg->fft_size * sizeof(float);
    size_t profile_bytes = 0;
    if (profile) MGX_TRY(mgx_profile_bytes(cfg, &profile_bytes));
    ranges.in[0] = byte_range(target_dev, (size_t)n_target * sizeof(float2));
    ranges.in[1] = byte_range(reference_dev, (size_t)n_reference * sizeof(float2));
    ranges.in[2] = byte_range(profile, profile_bytes);
    ranges.in[3] = byte_range(fir_given, fir_bytes);
    for (int i = 0; i < 3; ++i) ranges.out[i] = byte_range(call.out[i], (size_t)n_target * sizeof(float2));
    for (const CallContext& other : h->ctx)
        if (overlap(ranges.in[3], byte_range(other.taps.p, other.taps.bytes))) ranges.reads_context_taps = true;
    // on main alone: stage events bracket one stream's work, and a report waits for the call's scalars before it returns.
    // So does every handle of a device that has several: the lanes of a batch fill each other's idle stretches already,
    // and with front streams beside them they were measured a fifth slower
    bool alone;
    {
        LimiterChain& chain = g_limiter_chain[h->device % MAX_DEVICES];
        std::lock_guard<std::mutex> lock(chain.mu);
        alone = chain.live == 1;
    }
    if (alone) MGX_TRY(ensure_front(h));
    const MasterPlan plan = h->pipe.master(ranges, h->stage_timing || report != nullptr || !alone || !h->front);
    const int rc = queue_master(h, call, plan);
    if (rc != 0) {              // a front half may be left without its back half: nothing stays in flight
        drain(h);
        h->pipe.drained();
        return rc;
    }
    call.valid = true;
    ++h->masters_outstanding;
    CallContext& cx = h->ctx[plan.context];
    TrackWork& tw = cx.track[0];
    TrackWork& rw = cx.track[1];
    const CorrectionState* cs = &((const BackState*)h->back.p)->cs;      // (where the call's rounds left their results)
    // (a call with a report ran on main alone and waits below before anything else is queued: its copies may still read
    // the analysis results and the level gain in the context)
    if (report) {
        MGX_TRY(ensure_pinned(h, 1 << 16));
        char* pin = (char*)h->pinned;
        TrackStats* st_t = (TrackStats*)pin;
        TrackStats* st_r = (TrackStats*)(pin + 256);
        mgx_profile_header* hd_r = (mgx_profile_header*)(pin + 2048);       // (the profile route's reference)
        CorrectionState* hc = (CorrectionState*)(pin + 512);
        double* c0 = (double*)(pin + 1024);
        for (int attempt = 0; attempt < 2; ++attempt) {      // (a second time when the check queued the call again)
            HIP_TRY(hipMemcpyAsync(st_t, tw.stats.p, sizeof(TrackStats), hipMemcpyDeviceToHost, h->stream));
            if (profile)
                HIP_TRY(hipMemcpyAsync(hd_r, profile, sizeof(mgx_profile_header), hipMemcpyDeviceToHost, h->stream));
            else
                HIP_TRY(hipMemcpyAsync(st_r, rw.stats.p, sizeof(TrackStats), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(hc, cs, sizeof(CorrectionState), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(c0, cx.scalars.p, sizeof(double), hipMemcpyDeviceToHost, h->stream));
            MGX_TRY(sync_main(h));
            MGX_TRY(check_device_error(h, true));                 // (nothing of the run has been handed out yet)
            if (!h->requeued) break;
        }
        if (profile) {
            st_r->peak = hd_r->peak;
            st_r->amplitude_c = hd_r->amplitude_coefficient;
            st_r->average_rms = hd_r->average_rms;
            st_r->match_rms = hd_r->match_rms;
            st_r->divisions = hd_r->divisions;
            st_r->loud_count = hd_r->loud_count;
            st_r->piece = hd_r->piece;
        }
        std::memset(report, 0, sizeof(*report));
        report->final_amplitude_coefficient = st_r->amplitude_c;
        report->target_match_rms = st_t->match_rms;
        report->reference_match_rms = st_r->match_rms;
        report->rms_coefficient = *c0;
        for (int i = 0; i < 16; ++i) report->correction_coefficients[i] = hc->coeffs[i];
        report->normalize_coefficient = result_no_limiter_normalized_dev ? hc->normalize_c : 0.0;
        report->result_peak = hc->result_peak;
        report->target_divisions = st_t->divisions;
        report->reference_divisions = st_r->divisions;
        report->target_piece = st_t->piece;
        report->reference_piece = st_r->piece;
        report->target_loud_count = st_t->loud_count;
        report->reference_loud_count = st_r->loud_count;
        report->limiter_active = hc->limiter_active;
    }
    return 0;
}
