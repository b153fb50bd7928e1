// libmgx.so -- C ABI (include/mgx.h) over the gfx950 kernels.  No CPU fallback:
// every entry point that needs a GPU fails with MGX_ERR_NO_DEVICE / MGX_ERR_HIP.
// The one HIP translation unit: mgx_create, mgx_destroy and the entry points that touch a device are here; the handle,
// the stage runners, the device-error recovery and the call executor are the headers included below, each once and in
// the order of the stages; the entry points that touch no device are mgx_policy.cpp.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

// (the kernel headers in this order, ahead of the host headers that name them again: it is the order of the kernels in
// the code object)
#include "../../include/mgx.h"
#include "call_pipeline.h"
#include "code_sizes.h"
#include "fir_design.h"
#include "fir_plan.h"
#include "host_params.h"
#include "loudness_kernel.h"
#include "loudness_plan.h"
#include "mgx_kernels.h"
#include "convert_rate_kernel.h"
#include "resample_kernel.h"
#include "resample_plan.h"
#include "deliver_kernel.h"            // (behind every other kernel: it moves none of them in the code object)
#include "tp_limit_kernel.h"
#include "deliver_shaped_kernel.h"
#include "audit_kernel.h"
#include "visuals_kernel.h"
#include "eq_tone_kernels.h"           // (last: only a call with a tone launches it, and it moves no other kernel)
#include "declip_kernel.h"             // (behind it: only mgx_declip launches it)

#include "mgx_policy.h"
#include "handle.h"
#include "run_analysis.h"
#include "run_fir.h"
#include "run_conv.h"
#include "run_limiter.h"               // (ahead of the correction: its round 0 presets the limiter's look-back words)
#include "run_correction.h"
#include "device_errors.h"
#include "run_visuals.h"
#include "master_call.h"

#define NCCL_TRY(expr)                                                                       \
    do {                                                                                     \
        ncclResult_t r_ = (expr);                                                            \
        if (r_ != ncclSuccess)                                                               \
            return fail(MGX_ERR_RCCL, std::string(#expr) + ": " + ncclGetErrorString(r_));   \
    } while (0)

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

int mgx_device_count(int* count) {
    if (!count) return fail(MGX_ERR_ARGUMENT, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(MGX_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorName(e));
    }
    *count = n;
    return 0;
}

int mgx_device_pci_bus_id(int device, char* out, int32_t capacity) {
    if (!out || capacity < 16) return fail(MGX_ERR_ARGUMENT, "need room for 16 characters");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(MGX_ERR_NO_DEVICE, "no HIP device (this library has no CPU fallback)");
    }
    if (device < 0 || device >= n) return fail(MGX_ERR_ARGUMENT, "no such device");
    HIP_TRY(hipDeviceGetPCIBusId(out, capacity, device));
    return 0;
}

int mgx_create(int device, mgx_handle** out) {
    if (!out) return fail(MGX_ERR_ARGUMENT, "out is null");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(MGX_ERR_NO_DEVICE, "no HIP device visible: matchering_amd has no CPU fallback");
    if (device < 0 || device >= n) return fail(MGX_ERR_ARGUMENT, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    mgx_handle* h = new mgx_handle();
    h->device = device;
    HIP_TRY(hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, device));
    // the environment switches, read once here: a host thread's setenv cannot race a running call
    h->no_conv_wide = env_flag("MGX_NO_CONV_WIDE");
    h->no_conv_delay = env_flag("MGX_NO_CONV_DELAY");
    h->fir_round4 = env_flag("MGX_FIR_ROUND4");
    h->avoid_tail = env_flag("MGX_NO_TAIL");
    HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->fq = h->stream;
    HIP_TRY(hipEventCreate(&h->ev0));
    HIP_TRY(hipEventCreate(&h->ev1));
    HIP_TRY(hipEventCreateWithFlags(&h->lim_done, hipEventDisableTiming));
    {
        // the second handle of a device: whatever limiter the first has in flight was queued without an event
        LimiterChain& chain = g_limiter_chain[device % MAX_DEVICES];
        std::lock_guard<std::mutex> lock(chain.mu);
        if (++chain.live == 2) HIP_TRY(hipDeviceSynchronize());
    }
    HIP_TRY(hipHostMalloc((void**)&h->error_host, 64, hipHostMallocMapped));
    std::memset(h->error_host, 0, 64);
    HIP_TRY(hipHostGetDevicePointer((void**)&h->error_dev, h->error_host, 0));
    {   // code sizes for warm_code, once per device
        static std::mutex mu;
        static std::map<int, bool> done;
        std::lock_guard<std::mutex> lock(mu);
        if (!done[device]) {
            int bytes[CODE_KERNELS][CODE_VARIANTS];
            code_sizes_from_library(bytes);
            HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(mgx::g_code_bytes), bytes, sizeof(bytes)));
            done[device] = true;
        }
    }
    *out = h;
    return 0;
}

int mgx_destroy(mgx_handle* h) {
    if (!h) return 0;
    hipSetDevice(h->device);
    drain(h);
    {
        LimiterChain& chain = g_limiter_chain[h->device % MAX_DEVICES];
        std::lock_guard<std::mutex> lock(chain.mu);
        if (chain.last == h->lim_done) chain.last = nullptr;       // (its limiter has finished: the stream has drained)
        --chain.live;
    }
    if (h->lim_done) hipEventDestroy(h->lim_done);
    if (h->comm) ncclCommDestroy(h->comm);
    for (auto& kv : h->twiddles) hipFree(kv.second);
    if (h->pinned) hipHostFree(h->pinned);
    if (h->error_host) hipHostFree(h->error_host);
    hipEventDestroy(h->ev0);
    hipEventDestroy(h->ev1);
    for (auto& pair : h->stage_ev)
        for (hipEvent_t e : pair)
            if (e) hipEventDestroy(e);
    for (hipEvent_t e : {h->front_done[0], h->front_done[1], h->ctx_released[0], h->ctx_released[1], h->main_now})
        if (e) hipEventDestroy(e);
    if (h->front) hipStreamDestroy(h->front);
    hipStreamDestroy(h->stream);
    delete h;                               // (and with it every DevBuf of the handle and its tracks)
    return 0;
}

int mgx_malloc(mgx_handle* h, size_t bytes, void** dev) {
    if (!h || !dev) return fail(MGX_ERR_ARGUMENT, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMalloc(dev, bytes ? bytes : 256));
    return 0;
}
int mgx_free(mgx_handle* h, void* dev) {
    if (!h) return fail(MGX_ERR_ARGUMENT, "null handle");
    if (!dev) return 0;
    MGX_TRY(drain(h));
    h->pipe.drained();
    HIP_TRY(hipFree(dev));
    h->last_call.valid = false;             // (its pointers may be the block that has just gone: never queued again)
    return 0;
}
int mgx_memcpy_h2d(mgx_handle* h, void* dev, const void* host, size_t bytes) {
    if (!h) return fail(MGX_ERR_ARGUMENT, "null handle");
    h->pipe.other_work();
    HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, h->stream));
    MGX_TRY(sync_main(h));
    return 0;
}
int mgx_memcpy_d2h(mgx_handle* h, void* host, const void* dev, size_t bytes) {
    if (!h) return fail(MGX_ERR_ARGUMENT, "null handle");
    HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, h->stream));
    MGX_TRY(sync_main(h));
    MGX_TRY(check_device_error(h, true));
    if (h->requeued) {                       // the copy above took the failed run's bytes: take them again
        HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, h->stream));
        MGX_TRY(sync_main(h));
    }
    return 0;
}
// pinned host memory + copies that do not wait: the pieces of an overlapped host <-> HBM pipeline
int mgx_host_alloc(size_t bytes, void** host) {
    if (!host) return fail(MGX_ERR_ARGUMENT, "null argument");
    HIP_TRY(hipHostMalloc(host, bytes ? bytes : 256, hipHostMallocDefault));
    return 0;
}
int mgx_host_free(void* host) {
    if (!host) return 0;
    HIP_TRY(hipHostFree(host));
    return 0;
}
int mgx_memcpy_h2d_async(mgx_handle* h, void* dev, const void* host, size_t bytes) {
    if (!h) return fail(MGX_ERR_ARGUMENT, "null handle");
    h->pipe.other_work();
    HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, h->stream));
    return 0;
}
int mgx_memcpy_d2h_async(mgx_handle* h, void* host, const void* dev, size_t bytes) {
    if (!h) return fail(MGX_ERR_ARGUMENT, "null handle");
    // (a download writes no device memory and does not hold the next front half back -- unless it reads a context's own
    // taps, mgx_last_fir's pointer, which the front half of the call after next writes)
    for (const CallContext& cx : h->ctx)
        if (overlap(byte_range(dev, bytes), byte_range(cx.taps.p, cx.taps.bytes))) h->pipe.other_work();
    HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, h->stream));
    if (h->masters_outstanding > 0) ++h->downloads_outstanding;
    return 0;
}
int mgx_synchronize(mgx_handle* h) {
    if (!h) return fail(MGX_ERR_ARGUMENT, "null handle");
    MGX_TRY(sync_main(h));
    return check_device_error(h, true);
}
int mgx_timer_start(mgx_handle* h) {
    if (!h) return fail(MGX_ERR_ARGUMENT, "null handle");
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    return 0;
}
int mgx_timer_stop(mgx_handle* h, float* ms) {
    if (!h || !ms) return fail(MGX_ERR_ARGUMENT, "null argument");
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    HIP_TRY(hipEventSynchronize(h->ev1));
    HIP_TRY(hipEventElapsedTime(ms, h->ev0, h->ev1));
    return check_device_error(h);
}

// ---- stage level -----------------------------------------------------------
int mgx_analyze(mgx_handle* h, const float* x_dev, int64_t n, const mgx_config* cfg, int is_reference,
                double* peak, double* amplitude_coefficient, double* match_rms, int32_t* divisions,
                int64_t* piece_size, double* piece_rms, int32_t* loud, double* avg_mid, double* avg_side) {
    if (!h || !x_dev) return fail(MGX_ERR_ARGUMENT, "null argument");
    MGX_TRY(check_config(cfg));
    MGX_TRY(open_main(h));
    TrackWork& w = context(h).track[is_reference ? 1 : 0];
    w.is_reference = is_reference;
    MGX_TRY(run_track_spectra(h, cfg, x_dev, n, w));
    TrackStats st;
    HIP_TRY(hipMemcpyAsync(&st, w.stats.p, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    MGX_TRY(sync_main(h));
    const int half = cfg->fft_size / 2;
    if (peak) *peak = st.peak;
    if (amplitude_coefficient) *amplitude_coefficient = st.amplitude_c;
    if (match_rms) *match_rms = st.match_rms;
    if (divisions) *divisions = w.divisions;
    if (piece_size) *piece_size = w.piece;
    if (piece_rms) HIP_TRY(hipMemcpy(piece_rms, w.rms.p, w.divisions * sizeof(double), hipMemcpyDeviceToHost));
    if (loud) HIP_TRY(hipMemcpy(loud, w.loud.p, w.divisions * sizeof(int), hipMemcpyDeviceToHost));
    if (avg_mid) HIP_TRY(hipMemcpy(avg_mid, w.avg.p, (half + 1) * sizeof(double), hipMemcpyDeviceToHost));
    if (avg_side)
        HIP_TRY(hipMemcpy(avg_side, (double*)w.avg.p + (half + 1), (half + 1) * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

static int upload_taps(mgx_handle* h, const double* fir_mid, const double* fir_side, int taps) {
    CallContext& cx = context(h);
    MGX_TRY(ensure(h, cx.taps, (size_t)2 * taps * sizeof(float)));
    MGX_TRY(ensure_pinned(h, std::max((size_t)2 * taps * sizeof(float), (size_t)1 << 16)));
    float* st = (float*)h->pinned;
    for (int i = 0; i < taps; ++i) {
        st[i] = (float)fir_mid[i];
        st[taps + i] = (float)fir_side[i];
    }
    HIP_TRY(hipMemcpyAsync(cx.taps.p, st, (size_t)2 * taps * sizeof(float), hipMemcpyHostToDevice, h->stream));
    cx.last_taps = taps;
    return 0;
}

int mgx_convolve(mgx_handle* h, const float* x_dev, int64_t n, const double* fir_mid, const double* fir_side,
                 int32_t taps, double gain, float* y_dev, float* y_mid_dev, double* peak) {
    if (!h || !x_dev || !fir_mid || !fir_side || !y_dev) return fail(MGX_ERR_ARGUMENT, "null argument");
    if (n <= 0) return fail(MGX_ERR_ARGUMENT, "empty input");
    MGX_TRY(open_main(h));
    MGX_TRY(upload_taps(h, fir_mid, fir_side, taps));
    long long nblocks = 0;
    MGX_TRY(run_conv(h, x_dev, n, taps, (const float*)context(h).taps.p, gain, y_dev, y_mid_dev, &nblocks));
    MGX_TRY(sync_main(h));
    if (peak) {
        std::vector<float> bp(nblocks);
        HIP_TRY(hipMemcpy(bp.data(), h->block_peak.p, nblocks * sizeof(float), hipMemcpyDeviceToHost));
        float m = 0.f;
        for (float v : bp) m = std::max(m, v);
        *peak = m;
    }
    return 0;
}

// out[r] = the sum of part[r][0 .. chunks), in chunk order (mgx_clipped_piece_sumsq, mgx_window_energy)
static void sum_partials(const double* part, int64_t rows, int chunks, double* out) {
    for (int64_t r = 0; r < rows; ++r) {
        double s = 0.0;
        for (int c = 0; c < chunks; ++c) s += part[(size_t)r * chunks + c];
        out[r] = s;
    }
}

int mgx_clipped_piece_sumsq(mgx_handle* h, const float* mid_dev, int64_t n, int64_t piece_size, int32_t divisions,
                            double gain, double* sumsq) {
    if (!h || !mid_dev || !sumsq) return fail(MGX_ERR_ARGUMENT, "null argument");
    if (piece_size <= 0 || divisions <= 0 || piece_size * divisions > n)
        return fail(MGX_ERR_ARGUMENT, "piece grid does not fit the array");
    MGX_TRY(open_main(h));
    int chunks = 0;
    MGX_TRY(run_clipped_sumsq(h, mid_dev, piece_size, divisions, nullptr, gain, &chunks));
    std::vector<double> part((size_t)divisions * chunks);
    HIP_TRY(hipMemcpyAsync(part.data(), h->partial.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    MGX_TRY(sync_main(h));
    sum_partials(part.data(), divisions, chunks, sumsq);
    return 0;
}

int mgx_limit(mgx_handle* h, const float* x_dev, int64_t n, const mgx_config* cfg, double gain, double post_gain,
              float* out_dev, int32_t* active) {
    if (!h || !x_dev || !out_dev) return fail(MGX_ERR_ARGUMENT, "null argument");
    MGX_TRY(check_config(cfg));
    MGX_TRY(open_main(h));
    // peak -> early-out decision, through the same kernels the pipeline uses, in the handle's BackState as a master
    // call's limiter finds them (on main, behind every back half queued so far; no call context is touched)
    MGX_TRY(ensure(h, h->back, sizeof(BackState)));
    MGX_TRY(ensure_pinned(h, 1 << 16));
    BackState* back = (BackState*)h->back.p;
    CorrectionState* cs = &back->cs;
    hipLaunchKernelGGL(k_correction_init, dim3(1), dim3(1), 0, h->stream, cs, gain);
    // per-block peaks of x via the scale kernel's sibling: reuse k_finalize on a peak pass
    const long long nb = (n + 4095) / 4096;
    MGX_TRY(ensure(h, h->block_peak, (size_t)nb * sizeof(float)));
    hipLaunchKernelGGL(k_frame_peaks, dim3((unsigned)nb), dim3(256), 0, h->stream, (const float2*)x_dev, (long long)n,
                       (float*)h->block_peak.p);
    hipLaunchKernelGGL(k_finalize_scalars, dim3(1), dim3(256), 0, h->stream, (const float*)h->block_peak.p, nb,
                       cfg->threshold, cfg->min_value, cs, (const CorrectionState*)nullptr, (const double*)nullptr,
                       (const double*)nullptr, (double*)nullptr);
    double* post = (double*)h->pinned;
    *post = post_gain;
    HIP_TRY(hipMemcpyAsync(&back->reference_amplitude_c, post, sizeof(double), hipMemcpyHostToDevice, h->stream));
    CorrectionState host_cs;
    // Error words that earlier asynchronous mgx_master calls may have left are THEIRS: looked at (and reported) before
    // this call queues anything, so that the retry below can only ever answer for this call's own limiter.
    if (h->masters_outstanding > 0) {
        MGX_TRY(sync_main(h));
        MGX_TRY(check_device_error(h));
    }
    LimiterParams lp;
    const std::string err = limiter_params(*cfg, lp);
    if (!err.empty()) return fail(MGX_ERR_UNSUPPORTED, err);
    for (int attempt = 0;; ++attempt) {
        const bool tickets_before = h->limiter_tickets;
        MGX_TRY(run_limiter(h, x_dev, n, lp, cfg->threshold, &cs->gain, &back->reference_amplitude_c, &cs->limiter_active,
                            out_dev));
        HIP_TRY(hipMemcpyAsync(&host_cs, cs, sizeof(host_cs), hipMemcpyDeviceToHost, h->stream));
        MGX_TRY(sync_main(h));
        const int rc = check_device_error(h);
        if (rc == 0) break;
        if (attempt > 0 || tickets_before || !h->limiter_tickets) return rc;       // (once more when the handle has just switched to tickets)
    }
    if (active) *active = host_cs.limiter_active;
    return 0;
}

int mgx_scale(mgx_handle* h, const float* x_dev, int64_t n, double gain, float* out_dev) {
    if (!h || !x_dev || !out_dev) return fail(MGX_ERR_ARGUMENT, "null argument");
    if (n < 0) return fail(MGX_ERR_ARGUMENT, "negative frame count");
    if (n == 0) return 0;                                       // nothing to scale: a success that launches nothing
    MGX_TRY(open_main(h));
    const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(k_scale_outputs, dim3(grid), dim3(256), 0, h->stream, (const float2*)x_dev, (long long)n,
                       (const double*)nullptr, gain, (const double*)nullptr, (float2*)out_dev, (float2*)nullptr);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mgx_peak_count(mgx_handle* h, const float* x_dev, int64_t samples, double* peak, int64_t* count) {
    if (!h || !x_dev || !peak || !count) return fail(MGX_ERR_ARGUMENT, "null argument");
    MGX_TRY(open_main(h));
    MGX_TRY(ensure(h, h->peak_words, 64));
    MGX_TRY(ensure_pinned(h, (size_t)1 << 16));
    unsigned long long* words = (unsigned long long*)h->peak_words.p;
    HIP_TRY(hipMemsetAsync(words, 0, 16, h->stream));
    if (samples > 0) {
        const unsigned grid = (unsigned)peak_grid(samples);
        hipLaunchKernelGGL(k_peak_max, dim3(grid), dim3(256), 0, h->stream, x_dev, (long long)samples, words);
        hipLaunchKernelGGL(k_peak_count, dim3(grid), dim3(256), 0, h->stream, x_dev, (long long)samples, words);
        HIP_TRY(hipGetLastError());
    }
    unsigned long long* host = (unsigned long long*)h->pinned;
    HIP_TRY(hipMemcpyAsync(host, words, 16, hipMemcpyDeviceToHost, h->stream));
    MGX_TRY(sync_main(h));
    const unsigned bits = (unsigned)host[0];
    float f;
    std::memcpy(&f, &bits, 4);
    *peak = (double)f;
    *count = (int64_t)host[1];
    return 0;
}

int mgx_loudness(mgx_handle* h, const float* x_dev, int64_t n, int32_t sample_rate, mgx_loudness_report* report,
                 double* sub_energy, int64_t capacity, int64_t* count) {
    // everything that depends on the numbers alone is settled before the handle is touched
    int S = 0;
    MGX_TRY(loudness_request(report, n, sample_rate, sub_energy, capacity, count, &S));
    if (!h || (n > 0 && !x_dev)) return fail(MGX_ERR_ARGUMENT, "null argument");
    report->true_peak = report->sample_peak = 0.0;
    if (n == 0) {
        loudness_fill(loudness_gate(nullptr, 0, S), 0, S, report);
        return 0;
    }
    MGX_TRY(open_main(h));
    mgx_handle::LoudnessDev& dev = h->loudness_plans[sample_rate];
    if (!dev.table.p) {
        dev.plan = loudness_design(sample_rate);
        MGX_TRY(ensure(h, dev.table, dev.plan.table.size() * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(dev.table.p, dev.plan.table.data(), dev.plan.table.size() * sizeof(double), hipMemcpyHostToDevice,
                               h->stream));
    }
    const LoudnessGeometry g = loudness_geometry(dev.plan, n);
    const size_t doubles = (size_t)g.nsub * 2 + (size_t)g.workgroups * 2;
    MGX_TRY(ensure(h, h->loudness_out, doubles * sizeof(double)));
    MGX_TRY(ensure_pinned(h, std::max(doubles * sizeof(double), (size_t)1 << 16)));
    LoudnessArgs a;
    loudness_launch(a, dev.plan, g, n);
    a.x = x_dev;
    a.table = (const double*)dev.table.p;
    a.e = (double*)h->loudness_out.p;
    a.peaks = a.e + (size_t)g.nsub * 2;
    a.error = h->error_dev;
    a.error_slot = DEVICE_ERROR_SLOT_INPUT;
    MGX_TRY(allow_lds(k_loudness, LOUD_LDS_BYTES));
    hipLaunchKernelGGL(k_loudness, dim3((unsigned)g.workgroups), dim3(LOUD_THREADS), LOUD_LDS_BYTES, h->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->pinned, h->loudness_out.p, doubles * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    MGX_TRY(sync_main(h));
    // (as every blocking call: this also takes whatever the calls queued before it have reported, and with it the
    // handle's count of mgx_master calls and downloads outstanding -- nothing of theirs can be queued again from here)
    MGX_TRY(check_device_error(h, false, "the frames to measure"));
    const double* e = (const double*)h->pinned;
    const double* peaks = e + (size_t)g.nsub * 2;
    for (int64_t w = 0; w < g.workgroups; ++w) {
        report->true_peak = std::max(report->true_peak, peaks[2 * w]);
        report->sample_peak = std::max(report->sample_peak, peaks[2 * w + 1]);
    }
    loudness_fill(loudness_gate(e, g.nsub, g.S), g.nsub, g.S, report);
    if (sub_energy) std::memcpy(sub_energy, e, (size_t)g.nsub * 2 * sizeof(double));
    return 0;
}

int mgx_audit(mgx_handle* h, const void* x_dev, int64_t n_frames, int32_t bits, int32_t sample_rate,
              const mgx_audit_limits* limits, mgx_audit_report* report, double* sub_sums, int64_t capacity,
              int64_t* count) {
    // everything that depends on the numbers alone is settled before the handle is touched
    static_assert(AUDIT_SUB_MIN == (LOUD_MIN_RATE + 5) / 10, "a segment meets at most AUDIT_SUBS_MAX sub-blocks at every rate audit_request accepts");
    int B = 0;
    MGX_TRY(audit_request(limits, report, n_frames, bits, sample_rate, sub_sums, capacity, count, &B));
    if (!h) return fail(MGX_ERR_ARGUMENT, "h: null handle");
    if (n_frames > 0 && !x_dev) return fail(MGX_ERR_ARGUMENT, "x_dev: null");
    if (((size_t)x_dev) & 15) return fail(MGX_ERR_ARGUMENT, "x_dev: must be 16-byte aligned");
    audit_clear(report, bits);
    const int64_t subs = audit_sub_blocks(n_frames, B);
    if (n_frames == 0) return audit_gate(nullptr, 0, 0, B, report);
    MGX_TRY(open_main(h));
    AuditArgs a;
    audit_launch(a, n_frames, B, limits->clip_level, limits->silence_level, limits->clip_run);
    const size_t result_bytes = audit_result_bytes(a);
    MGX_TRY(ensure(h, h->audit_work, audit_seg_bytes(a) + audit_part_bytes(a)));
    MGX_TRY(ensure(h, h->audit_out, result_bytes));
    MGX_TRY(ensure_pinned(h, std::max(result_bytes, (size_t)1 << 16)));
    a.x = x_dev;
    a.seg = (AuditSegment*)h->audit_work.p;
    a.part = (double*)((char*)h->audit_work.p + audit_seg_bytes(a));
    a.totals = (AuditTotals*)h->audit_out.p;
    a.sub_sums = (double*)((char*)h->audit_out.p + sizeof(AuditTotals));
    const dim3 grid((unsigned)a.segments), block(AUDIT_THREADS);
    if (bits == 0) hipLaunchKernelGGL(k_audit<0>, grid, block, 0, h->stream, a);
    else if (bits == 16) hipLaunchKernelGGL(k_audit<16>, grid, block, 0, h->stream, a);
    else if (bits == 24) hipLaunchKernelGGL(k_audit<24>, grid, block, 0, h->stream, a);
    else hipLaunchKernelGGL(k_audit<32>, grid, block, 0, h->stream, a);
    hipLaunchKernelGGL(k_audit_merge<0>, dim3(1), dim3(AUDIT_MERGE_THREADS), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->pinned, h->audit_out.p, result_bytes, hipMemcpyDeviceToHost, h->stream));
    MGX_TRY(sync_main(h));
    MGX_TRY(check_device_error(h));
    const AuditTotals* t = (const AuditTotals*)h->pinned;
    const double* sums = (const double*)((const char*)h->pinned + sizeof(AuditTotals));
    for (int c = 0; c < 2; ++c) {
        report->sum[c] = t->sum[c], report->sumsq[c] = t->sumsq[c], report->peak[c] = t->peak[c];
        report->nonfinite[c] = t->nonfinite[c];
        report->clip_events[c] = t->clip_events[c], report->clip_samples[c] = t->clip_samples[c];
        report->clip_longest[c] = t->clip_longest[c], report->clip_first[c] = t->clip_first[c];
    }
    report->sum_lr = t->sum_lr;
    report->head_silence = t->head_silence, report->tail_silence = t->tail_silence;
    report->gap_longest = t->gap_longest, report->gap_at = t->gap_at;
    if (sub_sums) std::memcpy(sub_sums, sums, (size_t)subs * 3 * sizeof(double));
    return audit_gate(sums, subs, n_frames, B, report);
}

int mgx_declip(mgx_handle* h, const float* x_dev, int64_t n_frames, const mgx_declip_params* params, float* out_dev,
               mgx_declip_report* report) {
    // everything that depends on the numbers alone is settled before the handle is touched
    static_assert(DECLIP_MAX_RUN == MGX_DECLIP_MAX_RUN, "mgx_declip_check refuses what the kernel's halo does not hold");
    MGX_TRY(mgx_declip_check(params));
    if (n_frames < 0) return fail(MGX_ERR_ARGUMENT, "n_frames: negative");
    if (n_frames > LOUD_FRAMES_MAX) return fail(MGX_ERR_UNSUPPORTED, "mgx_declip: tracks of more than 500 million frames are not repaired here");
    if (!h) return fail(MGX_ERR_ARGUMENT, "h: null handle");
    if (!x_dev) return fail(MGX_ERR_ARGUMENT, "x_dev: null");
    if (!out_dev) return fail(MGX_ERR_ARGUMENT, "out_dev: null");
    if (((size_t)x_dev) & 15) return fail(MGX_ERR_ARGUMENT, "x_dev: must be 16-byte aligned");
    if (((size_t)out_dev) & 15) return fail(MGX_ERR_ARGUMENT, "out_dev: must be 16-byte aligned");
    const char* xb = (const char*)x_dev;
    const char* ob = (const char*)out_dev;
    if (xb < ob + (size_t)n_frames * 8 && ob < xb + (size_t)n_frames * 8) return fail(MGX_ERR_ARGUMENT, "out_dev: overlaps x_dev");
    if (report) {
        std::memset(report, 0, sizeof(*report));
        report->first_repaired[0] = report->first_repaired[1] = -1;
    }
    if (n_frames == 0) {
        h->declip_ran = false;
        return 0;
    }
    MGX_TRY(open_main(h));
    DeclipArgs a;
    declip_launch(a, n_frames, params->level, params->max_rise, params->min_run, params->max_run);
    MGX_TRY(ensure(h, h->declip_work, declip_seg_bytes(a)));
    MGX_TRY(ensure(h, h->declip_out, DECLIP_TOTALS_BYTES));
    a.x = x_dev;
    a.out = out_dev;
    a.seg = (int*)h->declip_work.p;
    a.totals = (long long*)h->declip_out.p;
    hipLaunchKernelGGL(k_declip<0>, dim3((unsigned)a.segments), dim3(DECLIP_THREADS), 0, h->stream, a);
    hipLaunchKernelGGL(k_declip_fold<0>, dim3(1), dim3(DECLIP_FOLD_THREADS), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    h->declip_ran = true;
    return report ? mgx_declip_report_read(h, report) : 0;
}

int mgx_declip_report_read(mgx_handle* h, mgx_declip_report* report) {
    if (!h) return fail(MGX_ERR_ARGUMENT, "h: null handle");
    if (!report) return fail(MGX_ERR_ARGUMENT, "report: null");
    std::memset(report, 0, sizeof(*report));
    report->first_repaired[0] = report->first_repaired[1] = -1;
    if (!h->declip_ran) return 0;                               // (no call yet, or the last one had no frames)
    HIP_TRY(hipSetDevice(h->device));
    MGX_TRY(ensure_pinned(h, (size_t)1 << 16));
    HIP_TRY(hipMemcpyAsync(h->pinned, h->declip_out.p, DECLIP_TOTALS_BYTES, hipMemcpyDeviceToHost, h->stream));
    MGX_TRY(sync_main(h));
    MGX_TRY(check_device_error(h));
    const long long* t = (const long long*)h->pinned;
    for (int c = 0; c < 2; ++c) {
        const long long* v = t + c * DECLIP_SLOTS;
        report->runs_repaired[c] = v[DECLIP_RUNS_REPAIRED], report->samples_repaired[c] = v[DECLIP_SAMPLES_REPAIRED];
        report->samples_raised[c] = v[DECLIP_SAMPLES_RAISED], report->longest_repaired[c] = v[DECLIP_LONGEST];
        report->first_repaired[c] = v[DECLIP_FIRST];
        report->runs_short[c] = v[DECLIP_RUNS_SHORT], report->runs_long[c] = v[DECLIP_RUNS_LONG], report->runs_edge[c] = v[DECLIP_RUNS_EDGE];
        const unsigned before = (unsigned)v[DECLIP_PEAK_BEFORE], after = (unsigned)v[DECLIP_PEAK_AFTER];
        float f;
        std::memcpy(&f, &before, 4);
        report->peak_before[c] = (double)f;
        std::memcpy(&f, &after, 4);
        report->peak_after[c] = (double)f;
    }
    return 0;
}

int mgx_spectrogram(mgx_handle* h, const float* x_dev, int64_t n_frames, const mgx_spectrogram_spec* spec,
                    const int32_t* edges, float* power, int64_t capacity, int64_t* count) {
    // everything that depends on the numbers alone is settled before the handle is touched
    SpectroPlan plan;
    MGX_TRY(spectrogram_request(n_frames, spec, edges, &plan));
    if (!h) return fail(MGX_ERR_ARGUMENT, "h: null handle");
    if (n_frames > 0 && !x_dev) return fail(MGX_ERR_ARGUMENT, "x_dev: null");
    if (((size_t)x_dev) & 7) return fail(MGX_ERR_ARGUMENT, "x_dev: must be 8-byte aligned");
    if (count) *count = plan.columns;
    if (n_frames == 0) return 0;
    const long long values = (long long)plan.columns * 2 * spec->bands;
    if (!power) return fail(MGX_ERR_ARGUMENT, "power: null");
    if (capacity < values)
        return fail(MGX_ERR_ARGUMENT, "capacity: " + std::to_string(capacity) + " floats hold fewer than the picture's " +
                                          std::to_string(values));
    MGX_TRY(open_main(h));
    const int N = 1 << spec->log2_fft, half = N / 2;
    mgx_handle::SpectroWindow* window = nullptr;
    MGX_TRY(spectro_window(h, spec->log2_fft, &window));
    SpectroArgs a;
    a.x = reinterpret_cast<const float2*>(x_dev);
    a.n = n_frames;
    a.hop = spec->hop, a.hops = plan.hops, a.columns = plan.columns, a.parts = plan.parts;
    a.channels = spec->channels, a.bands = spec->bands;
    a.window = (const float*)window->table.p;
    MGX_TRY(get_twiddles(h, spec->log2_fft, &a.tw));
    const size_t part_bytes = (size_t)plan.columns * plan.parts * 2 * (half + 1) * sizeof(float);
    const size_t edge_bytes = (size_t)(spec->bands + 1) * sizeof(int);
    MGX_TRY(ensure(h, h->visuals_work, part_bytes + edge_bytes));
    MGX_TRY(ensure(h, h->visuals_out, (size_t)values * sizeof(float)));
    a.part = (float*)h->visuals_work.p;
    a.edges = (const int*)((char*)h->visuals_work.p + part_bytes);
    a.scale = (2.0 / window->sum) * (2.0 / window->sum) * 0.25;
    a.out = (float*)h->visuals_out.p;
    HIP_TRY(hipMemcpyAsync((void*)a.edges, edges, edge_bytes, hipMemcpyHostToDevice, h->stream));
    switch (spec->log2_fft) {
#define CASE(L) case L: MGX_TRY(launch_spectrogram<L>(h, a)); break;
        CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14)
#undef CASE
        default: return fail(MGX_ERR_ARGUMENT, "log2_fft: outside 8 .. 14");
    }
    hipLaunchKernelGGL(k_spectro_pool<0>, dim3((unsigned)((values + 255) / 256)), dim3(256), 0, h->stream, a, half);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(power, a.out, (size_t)values * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    MGX_TRY(sync_main(h));
    MGX_TRY(check_device_error(h));
    return 0;
}

int mgx_overview(mgx_handle* h, const float* x_dev, int64_t n_frames, int32_t columns, float* minmax, double* sumsq) {
    int parts = 0;
    MGX_TRY(overview_request(n_frames, columns, &parts));
    if (!h) return fail(MGX_ERR_ARGUMENT, "h: null handle");
    if (n_frames > 0 && !x_dev) return fail(MGX_ERR_ARGUMENT, "x_dev: null");
    if (((size_t)x_dev) & 7) return fail(MGX_ERR_ARGUMENT, "x_dev: must be 8-byte aligned");
    if (n_frames == 0) return 0;
    if (!minmax) return fail(MGX_ERR_ARGUMENT, "minmax: null");
    if (!sumsq) return fail(MGX_ERR_ARGUMENT, "sumsq: null");
    MGX_TRY(open_main(h));
    OverviewArgs a;
    a.x = reinterpret_cast<const float2*>(x_dev);
    a.n = n_frames, a.columns = columns, a.parts = parts;
    // per (column, share) and channel: a double and two floats; the result the same per (column, channel)
    const size_t groups = (size_t)columns * parts;
    MGX_TRY(ensure(h, h->visuals_work, groups * 2 * (sizeof(double) + 2 * sizeof(float))));
    MGX_TRY(ensure(h, h->visuals_out, (size_t)columns * 2 * (sizeof(double) + 2 * sizeof(float))));
    MGX_TRY(ensure_pinned(h, std::max((size_t)columns * 2 * (sizeof(double) + 2 * sizeof(float)), (size_t)1 << 16)));
    a.part_sumsq = (double*)h->visuals_work.p;
    a.part_minmax = (float*)(a.part_sumsq + groups * 2);
    a.sumsq = (double*)h->visuals_out.p;
    a.minmax = (float*)(a.sumsq + (size_t)columns * 2);
    hipLaunchKernelGGL(k_overview<0>, dim3((unsigned)groups), dim3(OVERVIEW_THREADS), 0, h->stream, a);
    hipLaunchKernelGGL(k_overview_fold<0>, dim3((unsigned)((columns * 2 + 255) / 256)), dim3(256), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    const size_t result_bytes = (size_t)columns * 2 * (sizeof(double) + 2 * sizeof(float));
    HIP_TRY(hipMemcpyAsync(h->pinned, h->visuals_out.p, result_bytes, hipMemcpyDeviceToHost, h->stream));
    MGX_TRY(sync_main(h));
    MGX_TRY(check_device_error(h));
    std::memcpy(sumsq, h->pinned, (size_t)columns * 2 * sizeof(double));
    std::memcpy(minmax, (const char*)h->pinned + (size_t)columns * 2 * sizeof(double), (size_t)columns * 4 * sizeof(float));
    return 0;
}

int mgx_window_energy(mgx_handle* h, const float* x_dev, int64_t n, int64_t size, int64_t step, double* energy,
                      int64_t capacity, int64_t* count) {
    if (!h || !x_dev || !energy || !count || n < 1 || size < 1 || step < 1)
        return fail(MGX_ERR_ARGUMENT, "bad window energy arguments");
    MGX_TRY(open_main(h));
    if (size > n) size = n;                                   // dsp.py:131-132: the whole array is the only window
    const int64_t windows = (n - size) / step + 1;
    *count = windows;
    if (windows > capacity) return fail(MGX_ERR_ARGUMENT, "energy array too small for the number of windows");
    const int chunks = window_energy_chunks(size);
    const size_t bytes = (size_t)windows * chunks * sizeof(double);
    MGX_TRY(ensure(h, h->partial, bytes));
    MGX_TRY(ensure_pinned(h, std::max(bytes, (size_t)1 << 16)));
    for (int64_t w0 = 0; w0 < windows; w0 += WINDOW_ENERGY_ROWS_MAX) {      // (the reference has no limit)
        const unsigned rows = (unsigned)std::min<int64_t>(WINDOW_ENERGY_ROWS_MAX, windows - w0);
        hipLaunchKernelGGL(k_window_energy, dim3(chunks, rows), dim3(256), 0, h->stream, (const float2*)x_dev,
                           (long long)size, (long long)step, chunks, (double*)h->partial.p, (long long)w0);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->pinned, h->partial.p, bytes, hipMemcpyDeviceToHost, h->stream));
    MGX_TRY(sync_main(h));
    MGX_TRY(check_device_error(h));
    sum_partials((const double*)h->pinned, windows, chunks, energy);
    return 0;
}

int mgx_preview_cut(mgx_handle* h, const float* x_dev, int64_t n, int64_t begin, int64_t size, int64_t fade,
                    double clip_limit, float* out_dev) {
    if (!h || !x_dev || !out_dev || begin < 0 || size < 1 || begin + size > n || fade < 0 || fade > size)
        return fail(MGX_ERR_ARGUMENT, "bad preview cut arguments");
    MGX_TRY(open_main(h));
    const unsigned grid = (unsigned)preview_cut_grid(size);
    hipLaunchKernelGGL(k_preview_cut, dim3(grid), dim3(256), 0, h->stream, (const float2*)x_dev, (long long)begin,
                       (long long)size, (long long)fade, clip_limit, (float2*)out_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mgx_pcm_decode(mgx_handle* h, const void* pcm_dev, int64_t samples, int32_t bits, float* out_dev) {
    if (!h || !pcm_dev || !out_dev) return fail(MGX_ERR_ARGUMENT, "null argument");
    if (bits != 16 && bits != 24 && bits != 32) return fail(MGX_ERR_ARGUMENT, "PCM width must be 16, 24 or 32 bits");
    if (samples <= 0) return 0;
    MGX_TRY(open_main(h));
    const unsigned grid = (unsigned)pcm_grid(samples);
    hipLaunchKernelGGL(k_pcm_decode, dim3(grid), dim3(256), 0, h->stream, pcm_dev, (long long)samples, bits, out_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mgx_pcm_encode(mgx_handle* h, const float* x_dev, int64_t samples, int32_t bits, void* pcm_dev) {
    if (!h || !pcm_dev || !x_dev) return fail(MGX_ERR_ARGUMENT, "null argument");
    if (bits != 16 && bits != 24 && bits != 32) return fail(MGX_ERR_ARGUMENT, "PCM width must be 16, 24 or 32 bits");
    if (samples <= 0) return 0;
    MGX_TRY(open_main(h));
    const unsigned grid = (unsigned)pcm_grid(samples);
    hipLaunchKernelGGL(k_pcm_encode, dim3(grid), dim3(256), 0, h->stream, x_dev, (long long)samples, bits, pcm_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mgx_deliver(mgx_handle* h, const float* x_dev, int64_t samples, double gain, int32_t bits, int32_t dither,
                uint64_t seed, void* out_dev) {
    if (!h || !x_dev || !out_dev) return fail(MGX_ERR_ARGUMENT, "null argument");
    MGX_TRY(deliver_check(samples, gain, bits, dither));
    if ((((size_t)x_dev) | ((size_t)out_dev)) & 15) return fail(MGX_ERR_ARGUMENT, "x_dev / out_dev: must be 16-byte aligned");
    if (samples == 0) return 0;
    MGX_TRY(open_main(h));
    DeliverArgs a;
    deliver_launch(a, samples, gain, bits, dither, seed);
    a.x = x_dev;
    a.out = out_dev;
    hipLaunchKernelGGL(k_deliver, dim3((unsigned)deliver_grid(samples)), dim3(DELIVER_THREADS), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mgx_deliver_shaped(mgx_handle* h, const float* x_dev, int64_t n_frames, double gain, int32_t bits,
                       const mgx_noise_shaper* shaper, uint64_t seed, void* out_dev) {
    static_assert(SHAPED_TAPS_MAX == MGX_SHAPER_TAPS_MAX && MGX_SHAPER_SEGMENT % SHAPED_STEP == 0 &&
                      MGX_SHAPER_WARMUP % SHAPED_STEP == 0 && SHAPED_STEP % 2 == 0,
                  "a step of k_deliver_shaped is whole frame pairs and divides the segment and the warm-up");
    MGX_TRY(deliver_shaped_check(n_frames, gain, bits, shaper));
    if (!h) return fail(MGX_ERR_ARGUMENT, "h: null handle");
    if (!x_dev) return fail(MGX_ERR_ARGUMENT, "x_dev: null");
    if (!out_dev) return fail(MGX_ERR_ARGUMENT, "out_dev: null");
    if (((size_t)x_dev) & 15) return fail(MGX_ERR_ARGUMENT, "x_dev: must be 16-byte aligned");
    if (((size_t)out_dev) & 15) return fail(MGX_ERR_ARGUMENT, "out_dev: must be 16-byte aligned");
    if (n_frames == 0) return 0;
    MGX_TRY(open_main(h));
    DeliverShapedArgs a;
    deliver_shaped_launch(a, n_frames, gain, bits, shaper->taps, shaper->c, MGX_SHAPER_SEGMENT, MGX_SHAPER_WARMUP, seed);
    a.x = x_dev;
    a.out = out_dev;
    hipLaunchKernelGGL(k_deliver_shaped, dim3((unsigned)shaped_grid(n_frames, MGX_SHAPER_SEGMENT)), dim3(SHAPED_THREADS), 0,
                       h->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mgx_tp_limit(mgx_handle* h, const float* x_dev, int64_t n, double pre_gain, double ceiling, int32_t lookahead,
                 double release, float* out_dev, double* max_reduction) {
    // everything that depends on the numbers alone is settled before the handle is touched
    static_assert(TPL_LOOKAHEAD_MAX == TP_LIMIT_LOOKAHEAD_MAX && TPL_RELEASE_MAX == TP_LIMIT_RELEASE_MAX,
                  "tp_limit_check refuses what the kernels' LDS and decay tables do not hold");
    MGX_TRY(tp_limit_check(n, pre_gain, ceiling, lookahead, release));
    if (!h) return fail(MGX_ERR_ARGUMENT, "null handle");
    if (!x_dev) return fail(MGX_ERR_ARGUMENT, "x_dev: null");
    if (!out_dev) return fail(MGX_ERR_ARGUMENT, "out_dev: null");
    if ((((size_t)x_dev) | ((size_t)out_dev)) & 7) return fail(MGX_ERR_ARGUMENT, "x_dev / out_dev: must be 8-byte aligned");
    const char* xb = (const char*)x_dev;
    const char* ob = (const char*)out_dev;
    if (xb < ob + (size_t)n * 8 && ob < xb + (size_t)n * 8) return fail(MGX_ERR_ARGUMENT, "out_dev: overlaps x_dev");
    if (max_reduction) *max_reduction = 0.0;
    if (n == 0) return 0;
    MGX_TRY(open_main(h));
    TpLimitArgs a;
    double taps[49];
    loudness_true_peak_taps(taps);
    tpl_plan(a, n, pre_gain, ceiling, lookahead, release, taps);
    MGX_TRY(ensure(h, h->tp_plane, (size_t)a.tiles * TPL_TILE * sizeof(float)));
    MGX_TRY(ensure(h, h->tp_words, (size_t)a.tiles * 2 * sizeof(double)));
    if (max_reduction) MGX_TRY(ensure_pinned(h, std::max((size_t)a.tiles * sizeof(double), (size_t)1 << 16)));
    a.x = x_dev;
    a.out = out_dev;
    a.d0 = (float*)h->tp_plane.p;
    a.agg = (double*)h->tp_words.p;
    a.peak = a.agg + a.tiles;
    const size_t region_a = tpl_region_a(lookahead), region_b = tpl_region_b(lookahead), lds = tpl_apply_lds_bytes(lookahead);
    if (lds > LDS_PER_WORKGROUP_MAX) return fail(MGX_ERR_UNSUPPORTED, "mgx_tp_limit: the look-ahead's window does not fit the LDS");
    MGX_TRY(allow_lds(k_tp_apply, lds));
    hipLaunchKernelGGL(k_tp_envelope, dim3((unsigned)a.tiles), dim3(TPL_THREADS), TPL_ENVELOPE_LDS_BYTES, h->stream, a);
    if (a.tiles > 1)
        hipLaunchKernelGGL(k_tp_aggregate, dim3((unsigned)(a.tiles - 1)), dim3(TPL_THREADS), TPL_AGGREGATE_LDS_BYTES, h->stream, a);
    hipLaunchKernelGGL(k_tp_apply, dim3((unsigned)a.tiles), dim3(TPL_THREADS), lds, h->stream, a, (unsigned)region_a,
                       (unsigned)region_b);
    HIP_TRY(hipGetLastError());
    if (!max_reduction) return 0;
    HIP_TRY(hipMemcpyAsync(h->pinned, a.peak, (size_t)a.tiles * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    MGX_TRY(sync_main(h));
    MGX_TRY(check_device_error(h));
    const double* peaks = (const double*)h->pinned;
    for (long long t = 0; t < a.tiles; ++t) *max_reduction = std::max(*max_reduction, peaks[t]);
    return 0;
}

int mgx_resample(mgx_handle* h, const float* x_dev, int64_t n, int32_t channels, int32_t rate_in, int32_t rate_out,
                 float* out_dev, int64_t out_capacity_frames, int64_t* n_out) {
    // everything that depends on the numbers alone is settled before the handle is touched
    ResampleGeometry g;
    MGX_TRY(resample_request("mgx_resample", "the track is", &channels, n, rate_in, rate_out, &g, n_out));
    if (!out_dev) return 0;                                     // the caller asked for the length only
    if (!h || !x_dev) return fail(MGX_ERR_ARGUMENT, "null argument");
    const int64_t frames = *n_out;
    if (out_capacity_frames < frames) return fail(MGX_ERR_ARGUMENT, "the output holds fewer frames than the conversion gives");
    if (frames == 0) return 0;
    MGX_TRY(open_main(h));
    mgx_handle::ResampleDev* dev = nullptr;
    MGX_TRY(resample_dev(h, "mgx_resample", rate_in, rate_out, &dev));
    ResampleArgs a;
    const ResampleLaunch launch = resample_launch(a, g, n, frames, channels);
    a.x = x_dev;
    a.w = (const double*)dev->matrix.p;
    a.out = out_dev;
    if (channels == 2)
        hipLaunchKernelGGL(k_resample<2>, dim3(launch.grid), dim3(RESAMPLE_BLOCK), launch.lds, h->stream, a);
    else
        hipLaunchKernelGGL(k_resample<1>, dim3(launch.grid), dim3(RESAMPLE_BLOCK), launch.lds, h->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mgx_convert_rate(mgx_handle* h, const float* x_dev, int64_t n, int32_t rate_in, int32_t rate_out, float* out_dev,
                     int64_t out_capacity_frames, int64_t* n_out) {
    // everything that depends on the numbers alone is settled before the handle is touched (mgx_resample's contract)
    ResampleGeometry g;
    MGX_TRY(resample_request("mgx_convert_rate", "the frames are", nullptr, n, rate_in, rate_out, &g, n_out));
    if (!out_dev) return 0;                                     // the caller asked for the length only
    if (!h || !x_dev) return fail(MGX_ERR_ARGUMENT, "null argument");
    const int64_t frames = *n_out;
    if (out_capacity_frames < frames) return fail(MGX_ERR_ARGUMENT, "the output holds fewer frames than the conversion gives");
    if (frames == 0) return 0;
    MGX_TRY(open_main(h));
    mgx_handle::ResampleDev* dev = nullptr;
    MGX_TRY(resample_dev(h, "mgx_convert_rate", rate_in, rate_out, &dev));
    ConvertRateArgs a;
    const ConvertRateLaunch launch = convert_rate_launch(a, g, n, frames);
    a.x = x_dev;
    a.w = (const double*)dev->matrix.p;
    a.out = out_dev;
    const dim3 grid(launch.grid), block(CONVERT_RATE_BLOCK);
    switch (launch.P) {
        case 8: hipLaunchKernelGGL(k_convert_rate<8>, grid, block, launch.lds, h->stream, a); break;
        case 4: hipLaunchKernelGGL(k_convert_rate<4>, grid, block, launch.lds, h->stream, a); break;
        case 2: hipLaunchKernelGGL(k_convert_rate<2>, grid, block, launch.lds, h->stream, a); break;
        default: hipLaunchKernelGGL(k_convert_rate<1>, grid, block, launch.lds, h->stream, a); break;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int mgx_resample_plan(mgx_handle* h, int32_t rate_in, int32_t rate_out, void** weights_dev, int32_t* phases,
                      int32_t* row_entries, int64_t* designed) {
    if (!h || !weights_dev || !phases || !row_entries || !designed) return fail(MGX_ERR_ARGUMENT, "null argument");
    const auto it = h->resample_plans.find({rate_in, rate_out});
    if (it == h->resample_plans.end() || !it->second.matrix.p)
        return fail(MGX_ERR_ARGUMENT, "no track has been converted between these rates on this handle yet");
    *weights_dev = it->second.matrix.p;
    *phases = it->second.plan->g.L;
    *row_entries = it->second.plan->g.W;
    *designed = h->resample_designs;
    return 0;
}

// ---- the boundary: stages.main (master_call.h) --------------------------------
int mgx_master(mgx_handle* h, const float* target_dev, int64_t n_target, const float* reference_dev,
               int64_t n_reference, const mgx_config* cfg, float* result_dev, float* result_no_limiter_dev,
               float* result_no_limiter_normalized_dev, mgx_report* report) {
    return master_impl(h, target_dev, n_target, reference_dev, n_reference, nullptr, cfg, nullptr, result_dev,
                       result_no_limiter_dev, result_no_limiter_normalized_dev, report);
}
int mgx_master_with_fir(mgx_handle* h, const float* target_dev, int64_t n_target, const float* reference_dev,
                        int64_t n_reference, const mgx_config* cfg, const float* fir_dev, float* result_dev,
                        float* result_no_limiter_dev, float* result_no_limiter_normalized_dev, mgx_report* report) {
    if (!fir_dev) return fail(MGX_ERR_ARGUMENT, "null FIR");
    return master_impl(h, target_dev, n_target, reference_dev, n_reference, nullptr, cfg, fir_dev, result_dev,
                       result_no_limiter_dev, result_no_limiter_normalized_dev, report);
}

// the matching EQ's controls (mgx_eq_shape_check, mgx_shape_fir: mgx_policy.cpp)
int mgx_master_shaped(mgx_handle* h, const float* target_dev, int64_t n_target, const float* reference_dev,
                      int64_t n_reference, const void* profile_dev, const mgx_config* cfg, const mgx_eq_shape* shape,
                      float* result_dev, float* result_no_limiter_dev, float* result_no_limiter_normalized_dev,
                      mgx_report* report) {
    if ((reference_dev != nullptr) == (profile_dev != nullptr))
        return fail(MGX_ERR_ARGUMENT, "mgx_master_shaped takes a reference track or a reference profile, exactly one of them");
    return master_impl(h, target_dev, n_target, reference_dev, profile_dev ? 0 : n_reference,
                       (const mgx_profile_header*)profile_dev, cfg, nullptr, result_dev, result_no_limiter_dev,
                       result_no_limiter_normalized_dev, report, shape);
}

// ... and its tone controls (mgx_eq_tone_check, mgx_eq_tone_curve, mgx_tone_fir: mgx_policy.cpp)
int mgx_master_eq(mgx_handle* h, const float* target_dev, int64_t n_target, const float* reference_dev,
                  int64_t n_reference, const void* profile_dev, const mgx_config* cfg, const mgx_eq_shape* shape,
                  const mgx_eq_tone* tone, float* result_dev, float* result_no_limiter_dev,
                  float* result_no_limiter_normalized_dev, mgx_report* report) {
    if ((reference_dev != nullptr) == (profile_dev != nullptr))
        return fail(MGX_ERR_ARGUMENT, "mgx_master_eq takes a reference track or a reference profile, exactly one of them");
    return master_impl(h, target_dev, n_target, reference_dev, profile_dev ? 0 : n_reference,
                       (const mgx_profile_header*)profile_dev, cfg, nullptr, result_dev, result_no_limiter_dev,
                       result_no_limiter_normalized_dev, report, shape, tone);
}

// ---- reference profiles (mgx_profile_bytes: mgx_policy.cpp) --------------------
int mgx_reference_profile(mgx_handle* h, const float* reference_dev, int64_t n_reference, const mgx_config* cfg,
                          void* profile_dev) {
    if (!h || !reference_dev || !profile_dev) return fail(MGX_ERR_ARGUMENT, "null argument");
    MGX_TRY(check_config(cfg));
    MGX_TRY(open_main(h));
    // mgx_analyze(is_reference = 1)'s chain, then the pack
    TrackWork& w = context(h).track[1];
    w.is_reference = 1;
    MGX_TRY(run_track_spectra(h, cfg, reference_dev, n_reference, w));
    const int bins = cfg->fft_size / 2 + 1;
    hipLaunchKernelGGL(k_profile_pack, dim3((2 * bins + 255) / 256), dim3(256), 0, h->stream, (const TrackStats*)w.stats.p,
                       (const double*)w.avg.p, profile_want(cfg), (long long)n_reference, bins,
                       (mgx_profile_header*)profile_dev, h->error_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mgx_master_with_profile(mgx_handle* h, const float* target_dev, int64_t n_target, const void* profile_dev,
                            const mgx_config* cfg, const float* fir_dev, float* result_dev,
                            float* result_no_limiter_dev, float* result_no_limiter_normalized_dev,
                            mgx_report* report) {
    if (!profile_dev) return fail(MGX_ERR_ARGUMENT, "null profile");
    return master_impl(h, target_dev, n_target, nullptr, 0, (const mgx_profile_header*)profile_dev, cfg, fir_dev,
                       result_dev, result_no_limiter_dev, result_no_limiter_normalized_dev, report);
}

int mgx_profile_merge(mgx_handle* h, const void* const* profiles_dev, const int32_t* weights, int32_t count,
                      const mgx_config* cfg, void* profile_dev) {
    if (!h || !profiles_dev || !cfg || !profile_dev) return fail(MGX_ERR_ARGUMENT, "null argument");
    MGX_TRY(profile_merge_check(profiles_dev, weights, count, cfg, profile_dev));
    ProfileMergeArgs a = {};
    a.count = count;
    for (int i = 0; i < count; ++i) {
        a.src[i] = (const mgx_profile_header*)profiles_dev[i];
        a.weight[i] = weights ? weights[i] : 1;
    }
    MGX_TRY(open_main(h));
    const int bins = cfg->fft_size / 2 + 1;
    hipLaunchKernelGGL(k_profile_merge, dim3((2 * bins + 255) / 256), dim3(256), 0, h->stream, a, profile_want(cfg), bins,
                       (mgx_profile_header*)profile_dev, h->error_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mgx_stage_timing(mgx_handle* h, int32_t enable) {
    if (!h) return fail(MGX_ERR_ARGUMENT, "null handle");
    h->stage_timing = enable != 0;
    for (bool& u : h->stage_used) u = false;
    return 0;
}
#ifdef MGX_DEV_CONV_PHASES           // development builds only (tools/conv_delay_phases.py)
int mgx_dev_conv_ticks_read(unsigned* out, int blocks) {        // out: [blocks][8]
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(mgx::mgx_dev_conv_ticks), (size_t)blocks * 8 * sizeof(unsigned)) != hipSuccess;
}
#endif
#ifdef MGX_DEV_LIMITER_PHASES        // development builds only (tools/limiter_phases.py)
int mgx_dev_chunk_life_read(long long* out, int chunks) {       // out: [chunks][8]
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(mgx::mgx_dev_chunk_life), (size_t)chunks * 8 * sizeof(long long)) != hipSuccess;
}
int mgx_dev_phase_ticks_read(unsigned* out, int chunks) {       // out: [chunks][16]
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(mgx::mgx_dev_phase_ticks), (size_t)chunks * 16 * sizeof(unsigned)) != hipSuccess;
}
#endif
int mgx_stage_times(mgx_handle* h, float* ms) {
    if (!h || !ms) return fail(MGX_ERR_ARGUMENT, "null argument");
    MGX_TRY(sync_main(h));
    for (int s = 0; s < MGX_STAGE_COUNT; ++s) {
        ms[s] = -1.f;
        if (!h->stage_used[s]) continue;
        HIP_TRY(hipEventElapsedTime(&ms[s], h->stage_ev[s][0], h->stage_ev[s][1]));
        h->stage_used[s] = false;
    }
    return check_device_error(h);
}

int mgx_code_bytes(int32_t* bytes, int32_t capacity) {
    if (!bytes || capacity < CODE_KERNELS * CODE_VARIANTS) return fail(MGX_ERR_ARGUMENT, "need room for 7 x 16 sizes");
    int found[CODE_KERNELS][CODE_VARIANTS];
    code_sizes_from_library(found);
    for (int c = 0; c < CODE_KERNELS; ++c)
        for (int v = 0; v < CODE_VARIANTS; ++v) bytes[c * CODE_VARIANTS + v] = found[c][v];
    return CODE_KERNELS;
}

int mgx_last_fir(mgx_handle* h, void** taps_dev, int32_t* taps) {
    if (!h || !taps_dev || !taps) return fail(MGX_ERR_ARGUMENT, "null argument");
    CallContext& cx = context(h);
    if (!cx.taps.p || cx.last_taps <= 0) return fail(MGX_ERR_ARGUMENT, "no FIR has been designed on this handle yet");
    *taps_dev = cx.taps.p;
    *taps = cx.last_taps;
    return 0;
}

// ---- RCCL ----------------------------------------------------------------------
// The ranks of a job are the GPUs of ONE node, the data path between them is xGMI and the bootstrap needs nothing but
// loop-back -- but telling RCCL so (NCCL_SOCKET_IFNAME=lo, NCCL_IB_DISABLE=1) changes the environment of the HOST
// process, which is the host's decision and not thread-safe against a running library's reads of it: the Python
// front end does it where a job sets itself up (matchering_amd/ranks.py single_node_rccl_defaults), a C / C++ host sets
// the two variables itself before its first mgx_comm_* call.  Nothing here calls setenv.
int mgx_comm_unique_id(void* id128) {
    if (!id128) return fail(MGX_ERR_ARGUMENT, "null argument");
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    NCCL_TRY(ncclGetUniqueId(&id));
    std::memcpy(id128, &id, sizeof(id));
    return 0;
}
int mgx_comm_init(mgx_handle* h, const void* id128, int rank, int world) {
    if (!h || !id128) return fail(MGX_ERR_ARGUMENT, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    NCCL_TRY(ncclCommInitRank(&h->comm, world, id, rank));
    h->comm_rank = rank;
    h->comm_world = world;
    return 0;
}
int mgx_comm_count(mgx_handle* h, int32_t* ranks) {
    if (!h || !ranks) return fail(MGX_ERR_ARGUMENT, "null argument");
    if (!h->comm) return fail(MGX_ERR_ARGUMENT, "communicator not initialised");
    int n = 0;
    NCCL_TRY(ncclCommCount(h->comm, &n));
    *ranks = n;
    return 0;
}
int mgx_comm_broadcast_f32(mgx_handle* h, float* dev, int64_t count, int root) {
    if (!h || !h->comm) return fail(MGX_ERR_ARGUMENT, "communicator not initialised");
    h->pipe.other_work();
    NCCL_TRY(ncclBroadcast(dev, dev, (size_t)count, ncclFloat, root, h->comm, h->stream));
    return 0;
}
int mgx_comm_allgather_f32(mgx_handle* h, const float* send_dev, float* recv_dev, int64_t count) {
    if (!h || !h->comm) return fail(MGX_ERR_ARGUMENT, "communicator not initialised");
    h->pipe.other_work();
    NCCL_TRY(ncclAllGather(send_dev, recv_dev, (size_t)count, ncclFloat, h->comm, h->stream));
    return 0;
}
int mgx_comm_destroy(mgx_handle* h) {
    if (!h || !h->comm) return 0;
    NCCL_TRY(ncclCommDestroy(h->comm));
    h->comm = nullptr;
    return 0;
}

}  // extern "C"


#ifdef MGX_TAIL_TRACE
// experiments only (tools/tail_trace.py): the 100 MHz phase stamps of the last k_correction_round / k_correction_tail
extern "C" int mgx_debug_tail_trace(unsigned long long* tail /* [160*32] */, unsigned long long* round /* [8] */) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(tail, HIP_SYMBOL(mgx::g_tail_trace), sizeof(unsigned long long) * 160 * 32));
    HIP_TRY(hipMemcpyFromSymbol(round, HIP_SYMBOL(mgx::g_round_trace), sizeof(unsigned long long) * 8));
    return 0;
}
#endif
