// The handle of libmgx.so and what every stage runner and entry point does with it: its buffers, streams and call
// contexts, the waits, the stage brackets.  Host code of the one HIP translation unit (mgx.hip includes it once).
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mgx.h"
#include "call_pipeline.h"
#include "fir_plan.h"
#include "host_params.h"
#include "loudness_plan.h"
#include "mgx_kernels.h"
#include "mgx_policy.h"
#include "resample_plan.h"

using namespace mgx;

#if __has_include(<rocprofiler-sdk-roctx/roctx.h>) && !defined(MGX_NO_ROCTX)
#include <rocprofiler-sdk-roctx/roctx.h>         // one range per stage for rocprofv3 --marker-trace; optional
#else
static inline int roctxRangePushA(const char*) { return 0; }
static inline int roctxRangePop() { return 0; }
#endif

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(MGX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorName(e_) + " (" + \
                                         hipGetErrorString(e_) + ")");                        \
    } while (0)

// ---------------------------------------------------------------------------
// handle
// ---------------------------------------------------------------------------
// a device allocation that frees itself (the handle's buffers, and the temporaries of the FIR operator builds on every
// way out, the failing ones included)
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p) hipFree(p);
    }
};

struct TrackWork {              // per-track analysis workspace + results (device)
    DevBuf wg_sumsq, wg_peak, wg_spec, stats, rms, loud, avg;   // avg: [2][F/2+1] double
    DevBuf wg_pack;                                              // fft_size 65536: AnalysisQuad's scratch, 408 KB per workgroup
    DevBuf part;                                                 // [SPEC_SLICES][2][F/2+1] partial spectrum sums
    int divisions = 0, segs_per_piece = 0, segs_per_wg = 0, chunks = 0, nwg = 0, is_reference = 0;
    long long piece = 0;
};

struct PlanDev {
    void* blob = nullptr;       // FirPlanHost tables
    double* M = nullptr;        // [bins][bins] raw -> smooth operator
    int2* band = nullptr;       // [bins] columns [x, y) of each row that matter (k_fir_band)
    // the same operator in two packed, banded factors (fft_size >= 16384; fir_kernels.h, k_fir_apply_a / _b)
    struct Factor {
        double* packed = nullptr;       // the rows' windows, one after the other
        FactorRow* rows = nullptr;      // [rows] window of each row and where it starts in `packed`
        size_t bytes = 0;
    } A, B;
    std::shared_ptr<FirPlanHost> plan;      // keeps the host tables alive as long as the device copy
};
// One copy per (device, Config's design parameters) for the whole process, not per handle: the operator is bins^2
// doubles up to fft_size 8192 (34 MB at 4096), two packed factors of a few MB beyond, and the three device handles a
// batch runs on one GPU (batch.py) would otherwise each build and hold their own.  Entries live as long as the
// process: a handle that is destroyed may leave kernels of its siblings reading them.
static std::mutex g_plan_mu;
static std::map<std::pair<int, const FirPlanHost*>, PlanDev> g_plan_dev;

// exp(2 pi i j / N), j < N, float64: the twiddles of the minimum-phase chain (eq_shape_kernels.h), one table per
// (device, N) for the whole process, made on first use and kept like the plans above
static std::map<std::pair<int, int>, double2*> g_minphase_twiddles;

// Limiter launches of one device never run side by side.  k_limit deals its chunks by workgroup number (no atomic
// ticket): a chunk waits for words of lower-numbered chunks only, and every XCD's dispatcher hands out its share of a
// grid in order, so within ONE launch the lowest unfinished chunk is always resident.  Two limiter launches resident
// together break that: launch A's waiting workgroups can fill the XCD on which launch B's lowest chunk would start
// while B's fill the one A needs (seen with two rank PROCESSES sharing a GPU: the bounded waits expired,
// profiles/r05_u_*).  Handles of one process (the two or three lanes of a batch) therefore chain their limiter
// launches through an event per handle -- a limiter fills the chip by itself, nothing is lost -- while every other
// kernel of the lanes still overlaps freely.  Processes that share a GPU cannot see each other: they set
// MGX_LIMIT_TICKETS=1 (bench.py and batch.py do when ranks outnumber GPUs), and a handle whose wait expires all the
// same falls back to tickets by itself (check_device_error).
constexpr int MAX_DEVICES = 64;
struct LimiterChain {
    std::mutex mu;
    hipEvent_t last = nullptr;      // recorded behind the device's most recent limiter launch
    int live = 0;                   // handles alive on the device
};
static LimiterChain g_limiter_chain[MAX_DEVICES];

// What the front half of a master call (analysis, FIR design, filter spectra) writes and its back half reads.  A
// handle owns CALL_CONTEXTS of them, so that the next call's front half can run under this call's back half
// (call_pipeline.h); everything only back halves touch stays single in the handle.
// THE INVARIANT THE PIPELINE RESTS ON: once the launch of round 0 of a call's level correction has finished
// (k_correction_round with build_band; k_finalize_scalars for a call without rounds), nothing of that call reads or
// writes its CallContext.  That launch moves the last things the rest of the back half needs -- the correction state
// the front half reset and the reference's two scalars -- into the handle's BackState (mgx_handle::back); the tail,
// the later rounds, the scale kernel, the limiter and the report work there.  So the context is handed to the front
// half of the next call but one right behind that launch (ctx_released), not behind the limiter.
struct CallContext {
    TrackWork track[2];
    DevBuf fir_scratch, scalars, taps, filt, cstate;
    DevBuf fir_robust;                      // lowess_it > 0: robustness weights and residuals, [2][2][nlog]
    DevBuf eq_work;                         // a minimum-phase matching EQ: the chain's two planes and maxima (eq_shape_kernels.h)
    int last_taps = 0;
};

struct mgx_handle {
    int device = 0;
    int cus = 0;                            // compute units of the device (read at mgx_create)
    hipStream_t stream = nullptr;           // main: everything but a pipelined call's front half
    hipStream_t front = nullptr;            // the front halves of pipelined master calls (call_pipeline.h)
    hipStream_t fq = nullptr;               // where the front-half runners queue: `stream`, or `front` inside a pipelined call
    CallPipeline pipe;
    CallContext ctx[CALL_CONTEXTS];         // a pipelined call takes the other one; the stage-level entry points use the most recent call's
    // front_done[c]: behind the front half that filled context c.  ctx_released[c]: behind the last launch of the call
    // in context c that touches the context (round 0 of its level correction) -- what wait (a) of the next user's front
    // half needs, and NOT the end of that call's back half: whoever needs the whole back half (ensure / ensure_pinned
    // before freeing, mgx_free, mgx_destroy, drain, the planner's drained()) synchronises main itself.
    hipEvent_t front_done[CALL_CONTEXTS] = {}, ctx_released[CALL_CONTEXTS] = {};
    hipEvent_t main_now = nullptr;          // wait (b): recorded on main when a dirty call's front half starts
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool stage_timing = false;                                    // mgx_stage_timing
    hipEvent_t stage_ev[MGX_STAGE_COUNT][2] = {};
    bool stage_used[MGX_STAGE_COUNT] = {};
    std::map<int, float2*> twiddles;
    DevBuf y, mid, block_peak, partial, conv_queue;
    DevBuf back;                            // one BackState: filled by round 0 of each call, the rest of its back half works here
    DevBuf lim_published, lim_ctrl, lim_weights, round_ctr, tail_gains, band, band_info;
    std::vector<double> lim_weights_host;
    DevBuf peak_words;                      // mgx_peak_count: {bits of the maximum, count}
    DevBuf lim_tables;                      // general filter orders: matrix powers and look-back matrices
    std::vector<double> lim_tables_host;
    // mgx_resample: the weights of every rate pair this handle has converted, designed and uploaded once
    struct ResampleDev {
        std::shared_ptr<const ResamplePlan> plan;
        std::vector<double> host;           // the matrix as uploaded (resample_device_matrix)
        DevBuf matrix;
    };
    std::map<std::pair<int, int>, ResampleDev> resample_plans;
    long long resample_designs = 0;         // plans designed and uploaded so far (mgx_resample_plan)
    // mgx_loudness: the K-weighting plan of every sample rate this handle has metered, and its table on the device
    struct LoudnessDev {
        LoudnessPlan plan;
        DevBuf table;
    };
    std::map<int, LoudnessDev> loudness_plans;
    DevBuf loudness_out;                    // [nsub][2] sub-block energies, then [workgroups][2] peaks
    DevBuf tp_plane, tp_words;              // mgx_tp_limit: the d0 plane [tiles * T] float32; aggregates and peaks, [2][tiles] float64
    DevBuf audit_work, audit_out;           // mgx_audit: the segments' records and sub-block shares; the totals, then [count][3] sub-block sums
    DevBuf declip_work, declip_out;         // mgx_declip: the segments' counters, [segments][2][DECLIP_SLOTS] int; the track's, as long long
    bool declip_ran = false;                // declip_out holds the counters of the most recent mgx_declip call (mgx_declip_report_read)
    // mgx_spectrogram: the float32 window of every transform length this handle has drawn, built once per log2, and the
    // float64 sum of its values
    struct SpectroWindow {
        DevBuf table;
        double sum = 0.0;
    };
    std::map<int, SpectroWindow> spectro_windows;
    DevBuf visuals_work, visuals_out;       // mgx_spectrogram / mgx_overview: the workgroups' partials (then the band edges); the picture
    void* pinned = nullptr;
    size_t pinned_bytes = 0;
    // set by a kernel whose bounded wait expired (limiter look-back, level-correction round): one word of
    // page-locked host memory the kernels write through its device address, so that every blocking call
    // can look at it for free once the stream has drained
    bool limiter_ran_by_number = false;      // a limiter launch since the last error check dealt chunks by workgroup number
    int* error_host = nullptr;
    int* error_dev = nullptr;
    // the arguments of the last mgx_master call, kept so that it can be queued again when the level-correction
    // tail reports that its workgroups were not resident together (check_device_error)
    struct MasterCall {
        bool valid = false;
        const float* target = nullptr;
        const float* reference = nullptr;
        const float* fir_given = nullptr;
        const mgx_profile_header* profile = nullptr;     // mgx_master_with_profile: the reference is this, `reference` null
        int64_t n_target = 0, n_reference = 0;
        mgx_config cfg;
        LimiterParams lp;                   // derived from cfg when out[0] (the limited result) is wanted
        float* out[3] = {nullptr, nullptr, nullptr};
        bool shaped = false;                // mgx_master_shaped with a shape: `shape` is the call's own copy
        mgx_eq_shape shape = {};
        bool toned = false;                 // mgx_master_eq with a tone that is not neutral: `tone` likewise (then `shaped`)
        mgx_eq_tone tone = {};
    } last_call;
    bool avoid_tail = false;                // sticky after such a report: rounds 1..K-1 as one launch each (MGX_NO_TAIL=1: always)
    bool requeued = false;                  // the last check_device_error queued the call again
    // the limiter's chunks are its workgroups' numbers; after a look-back wait has expired once on this handle they are
    // drawn from an atomic ticket instead, which does not lean on the dispatch order (k_limit, limiter_kernels.h)
    bool limiter_tickets = false;
    hipEvent_t lim_done = nullptr;                                // behind this handle's latest limiter launch (LimiterChain)
    int masters_outstanding = 0;            // mgx_master calls queued since the last check of the error words
    int downloads_outstanding = 0;          // device-to-host copies queued behind them
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    // the paths tests compare the product against, chosen by environment switches read once at mgx_create
    bool no_conv_wide = false;              // MGX_NO_CONV_WIDE=1: 4096 taps by k_conv<13, false> on N = 2F
    bool no_conv_delay = false;             // MGX_NO_CONV_DELAY=1: two filter partitions by the partitioned k_conv<14, true>
    bool fir_round4 = false;                // MGX_FIR_ROUND4=1: the dense operator at 16384 taps, the chain itself beyond
};

static CallContext& context(mgx_handle* h) { return h->ctx[h->pipe.current()]; }

// both streams idle.  Main first: it waits for every front half that has its back half queued; then whatever front half
// is still being queued.
static int drain(mgx_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->front) HIP_TRY(hipStreamSynchronize(h->front));
    return 0;
}
// What an entry point does where it waits for its work: synchronising main drains the front stream too, because every
// front half is followed by a back half on main that waits for it (master_impl drains both where queueing failed half-way)
static int sync_main(mgx_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->pipe.drained();
    return 0;
}
// How an entry point that queues work on main opens, once its arguments are checked: the handle's device made current,
// and the call pipeline told that main holds work that may write device memory -- without that the front half of the
// next pipelined master call would not wait for it (call_pipeline.h, wait (b)).
static int open_main(mgx_handle* h) {
    HIP_TRY(hipSetDevice(h->device));
    h->pipe.other_work();
    return 0;
}

// The front stream and the events of the call pipeline, made when a handle first finds itself alone on its device: the
// lanes of a batch never pipeline (master_impl) and keep their one stream.  The lowest priority: where both streams have
// work the dispatcher takes the back half's, which the caller is waiting for, and the front half fills what that leaves
// idle (at default priority most of the gain is lost).
static int ensure_front(mgx_handle* h) {
    if (h->front) return 0;
    int least = 0, greatest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
    for (hipEvent_t* e : {&h->front_done[0], &h->front_done[1], &h->ctx_released[0], &h->ctx_released[1], &h->main_now})
        HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    HIP_TRY(hipStreamCreateWithPriority(&h->front, hipStreamNonBlocking, least));
    // (no ctx_released was recorded behind the calls so far: the first front half waits for everything main holds instead)
    h->pipe.other_work();
    return 0;
}

static int ensure(mgx_handle* h, DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return 0;
    if (b.p) {
        MGX_TRY(drain(h));
        HIP_TRY(hipFree(b.p));
        b.p = nullptr;
        b.bytes = 0;
    }
    const size_t want = std::max(bytes, (size_t)256);
    HIP_TRY(hipMalloc(&b.p, want));
    b.bytes = want;
    return 0;
}
static int ensure_pinned(mgx_handle* h, size_t bytes) {
    if (h->pinned_bytes >= bytes) return 0;
    if (h->pinned) {
        MGX_TRY(drain(h));
        HIP_TRY(hipHostFree(h->pinned));
        h->pinned = nullptr;
        h->pinned_bytes = 0;
    }
    HIP_TRY(hipHostMalloc(&h->pinned, bytes, hipHostMallocDefault));
    h->pinned_bytes = bytes;
    return 0;
}

// HIP-event brackets around the stages of mgx_master (mgx_stage_timing / mgx_stage_times): events on
// the handle's stream, so they cost no synchronisation; off by default.
static void stage_mark(mgx_handle* h, int stage, int end) {
    if (!h->stage_timing) return;
    if (!h->stage_ev[stage][0]) {
        hipEventCreate(&h->stage_ev[stage][0]);
        hipEventCreate(&h->stage_ev[stage][1]);
    }
    hipEventRecord(h->stage_ev[stage][end], h->stream);
    if (end) h->stage_used[stage] = true;
}
// (+ a roctx range per stage: `rocprofv3 --marker-trace` shows which launches belong to which stage of
// stages.py:210-272; a push/pop costs nothing when no profiler is attached)
static const char* const STAGE_NAMES[MGX_STAGE_COUNT] = {"mgx:analyze", "mgx:design_fir", "mgx:filter_spectra",
                                                         "mgx:convolve", "mgx:correct_levels", "mgx:scale_outputs",
                                                         "mgx:limit"};
struct StageScope {
    mgx_handle* h;
    int stage;
    StageScope(mgx_handle* h_, int s) : h(h_), stage(s) {
        roctxRangePushA(STAGE_NAMES[stage]);
        stage_mark(h, stage, 0);
    }
    ~StageScope() {
        stage_mark(h, stage, 1);
        roctxRangePop();
    }
};

static int get_twiddles(mgx_handle* h, int log2n, const float2** out) {
    auto it = h->twiddles.find(log2n);
    if (it != h->twiddles.end()) {
        *out = it->second;
        return 0;
    }
    const int n = 1 << log2n;
    std::vector<float2> tw(n);
    const double pi = 3.14159265358979323846;
    for (int k = 0; k < n; ++k)
        tw[k] = make_float2((float)std::cos(2.0 * pi * k / n), (float)-std::sin(2.0 * pi * k / n));
    float2* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, n * sizeof(float2)));
    HIP_TRY(hipMemcpy(d, tw.data(), n * sizeof(float2), hipMemcpyHostToDevice));
    h->twiddles[log2n] = d;
    *out = d;
    return 0;
}

template <typename K>
static int allow_lds(K kernel, size_t bytes) {
    if (bytes > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}

// control words shared by the kernels that count arrivals: [0] limiter ticket, [1] limiter error flag,
// [4] correction-round arrivals.  Zeroed when allocated; every user leaves its word at zero.
static int ensure_ctrl(mgx_handle* h) {
    if (h->lim_ctrl.p) return 0;
    MGX_TRY(ensure(h, h->lim_ctrl, 64));
    HIP_TRY(hipMemsetAsync(h->lim_ctrl.p, 0, 64, h->stream));
    return 0;
}

// The weights of a rate pair on the device: mgx_resample and mgx_convert_rate share the cache, so whichever of the two
// (`entry`) meets a pair first designs and uploads it, once for both.
static int resample_dev(mgx_handle* h, const char* entry, int rate_in, int rate_out, mgx_handle::ResampleDev** out) {
    mgx_handle::ResampleDev& dev = h->resample_plans[{rate_in, rate_out}];
    if (!dev.matrix.p) {
        dev.plan = resample_design(rate_in, rate_out);
        if (!dev.plan) return fail(MGX_ERR_UNSUPPORTED, std::string(entry) + ": no plan for these rates");
        dev.host = resample_device_matrix(*dev.plan);
        MGX_TRY(ensure(h, dev.matrix, dev.host.size() * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(dev.matrix.p, dev.host.data(), dev.host.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        ++h->resample_designs;
    }
    *out = &dev;
    return 0;
}

// an environment switch: "1" turns it on
static bool env_flag(const char* name) {
    const char* e = std::getenv(name);
    return e && e[0] == '1';
}
