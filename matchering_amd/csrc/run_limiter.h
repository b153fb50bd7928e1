// Stage 4's limiter on the host side: the state a launch needs, its arguments and the launch itself (limiter_kernels.h,
// limiter_general.h).
#pragma once

#include "handle.h"

// look-back words and control block of a limiter launch over n frames (allocated, not initialised)
// (blocks per limiter chunk: the rule of host_params.h.  Chunks of 512 blocks were built and measured in round 6 for
// 96 kHz, where the halos eat a quarter of a 256-block chunk: 221 us against 204 (and 306 for 1024 blocks), 84 B of
// scratch at the 128 registers two workgroups per CU leave -- profiles/r06_b_*; removed.)
static int limiter_state(mgx_handle* h, long long n, const LimiterParams& lp, unsigned long long** published,
                         long long* words, int** ticket) {
    const long long nchunks = (n + lp.geo.chunk - 1) / lp.geo.chunk;
    MGX_TRY(ensure(h, h->lim_published, (size_t)limiter_words(lp, nchunks) * sizeof(unsigned long long)));
    MGX_TRY(ensure_ctrl(h));
    *published = (unsigned long long*)h->lim_published.p;
    *words = limiter_words(lp, nchunks);
    *ticket = (int*)h->lim_ctrl.p;
    return 0;
}

// A table the limiter kernels read (the look-back weights, the general orders' matrices): uploaded when `want` differs
// from the host copy of what the device holds, that is when the parameters have changed.  A blocking copy behind
// whatever main still runs with the old table.
static int upload_if_changed(mgx_handle* h, DevBuf& dev, std::vector<double>& host, const std::vector<double>& want) {
    if (host == want) return 0;
    MGX_TRY(ensure(h, dev, want.size() * sizeof(double)));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(dev.p, want.data(), want.size() * sizeof(double), hipMemcpyHostToDevice));
    host = want;
    return 0;
}

// hold / release filters of order 2 or 3: k_limit_general<K>, its tables uploaded when the parameters change
template <int K>
static int launch_limiter_general(mgx_handle* h, const LimiterArgs& a, const LimiterParams& lp) {
    MGX_TRY(upload_if_changed(h, h->lim_tables, h->lim_tables_host, general_tables(lp)));
    const GeneralArgs<K> g = general_fill<K>(lp, (const double*)h->lim_tables.p, a.published, a.nchunks);
    const size_t lds = LimiterGeneral<K>::LDS_BYTES;
    MGX_TRY((allow_lds(k_limit_general<K>, lds)));
    hipLaunchKernelGGL((k_limit_general<K>), dim3((unsigned)a.nchunks), dim3(256), lds, h->stream, a, g);
    HIP_TRY(hipGetLastError());
    return 0;
}

// 256-block chunks (four workgroups per CU) unless the configured attack / hold times need 1024
// (a persistent grid that fetches a workgroup's next chunk under its current one was built and measured in round 4:
// 187 against 171 us, profiles/r04_c_persistent_limiter.txt)
// the 256-block kernel: the instantiation for the configuration's window geometry when there is one (k_limit in
// limiter_kernels.h)
static void launch_limiter_256(const LimiterArgs& a, dim3 grid, hipStream_t stream) {
    const size_t lds = LimiterBlock<256>::LDS_BYTES;
#ifdef MGX_TEST_LIMIT_GENERAL
    // test build (tests/test_gpu_stage_sweeps.py): every geometry takes the general instantiation, which the
    // specialised ones must equal bit for bit
    constexpr bool specialised = false;
#else
    constexpr bool specialised = true;
#endif
    if (specialised && a.hw == 44 && a.hb == 43 && a.gr == 26 && a.gl == 6 && a.gw == 3)                 // 44.1 kHz, 1 ms / 1 ms
        hipLaunchKernelGGL((k_limit<256, 4, 44, 43, 26>), grid, dim3(256), lds, stream, a);
    else if (specialised && a.hw == 48 && a.hb == 47 && a.gr == 28 && a.gl == 6 && a.gw == 3)            // 48 kHz
        hipLaunchKernelGGL((k_limit<256, 4, 48, 47, 28>), grid, dim3(256), lds, stream, a);
    else if (specialised && a.hw == 96 && a.hb == 95 && a.gr == 55 && a.gl == 12 && a.gw == 6)           // 96 kHz (BASELINE config #5)
        hipLaunchKernelGGL((k_limit<256, 4, 96, 95, 55>), grid, dim3(256), lds, stream, a);
    else
        hipLaunchKernelGGL((k_limit<256, 4>), grid, dim3(256), lds, stream, a);
}
static int launch_limiter(mgx_handle* h, const LimiterArgs& a, int threads) {
    const dim3 grid((unsigned)a.nchunks);
    if (threads == 1024) {
        const size_t lds = LimiterBlock<1024>::LDS_BYTES;
        MGX_TRY((allow_lds(k_limit<1024, 1>, lds)));
        hipLaunchKernelGGL((k_limit<1024, 1>), grid, dim3(1024), lds, h->stream, a);
    } else {
        launch_limiter_256(a, grid, h->stream);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// everything of a limiter launch but the look-back words, ticket and error flag
static int limiter_args(mgx_handle* h, const float* y, long long n, const LimiterParams& lp, double threshold,
                        const double* gain_dev, const double* post_dev, const int* active_dev, float* out, LimiterArgs& a) {
    if (n < 8) return fail(MGX_ERR_ARGUMENT, "limiter input too short");
    limiter_fill(lp, (float)threshold, a);
    a.y = reinterpret_cast<const float2*>(y);
    a.n = n;
    a.out = reinterpret_cast<float2*>(out);
    a.gain = gain_dev;
    a.post_gain = post_dev;
    a.active = active_dev;
    a.nchunks = (n + lp.geo.chunk - 1) / lp.geo.chunk;
    // look-back weights: uploaded when the parameters change
    std::vector<double> w(lp.w_hold);
    w.insert(w.end(), lp.w_rel.begin(), lp.w_rel.end());
    w.insert(w.end(), lp.w_att.begin(), lp.w_att.end());
    MGX_TRY(upload_if_changed(h, h->lim_weights, h->lim_weights_host, w));
    a.w_hold = (const double*)h->lim_weights.p;
    a.w_rel = a.w_hold + lp.w_hold.size();
    a.w_att = a.w_rel + lp.w_rel.size();
    return 0;
}

// preset_done: the caller's previous kernel has already preset the look-back words and the ticket
static int run_limiter(mgx_handle* h, const float* y, long long n, const LimiterParams& lp, double threshold,
                       const double* gain_dev, const double* post_dev, const int* active_dev, float* out,
                       bool preset_done = false) {
    LimiterArgs a;
    MGX_TRY(limiter_args(h, y, n, lp, threshold, gain_dev, post_dev, active_dev, out, a));
    // published words preset to "unpublished", ticket and error zeroed, every launch
    const size_t pub_bytes = (size_t)limiter_words(lp, a.nchunks) * sizeof(unsigned long long);
    MGX_TRY(ensure(h, h->lim_published, pub_bytes));
    MGX_TRY(ensure_ctrl(h));
    a.published = (unsigned long long*)h->lim_published.p;
    // "1" = always tickets.  Read here at every launch, not at mgx_create: bench.py and the batch lanes set it at run
    // time, possibly after the handle exists.
    a.ticket = (h->limiter_tickets || env_flag("MGX_LIMIT_TICKETS")) ? (int*)h->lim_ctrl.p : nullptr;
    h->limiter_ran_by_number = h->limiter_ran_by_number || a.ticket == nullptr;     // (since the last error check)
    a.error = h->error_dev;
    a.gave_up = (int*)h->lim_ctrl.p + 2;                      // ([0] the ticket, [2] "a waiter has given up")
    if (!preset_done) {
        HIP_TRY(hipMemsetAsync(h->lim_published.p, 0xff, pub_bytes, h->stream));
        HIP_TRY(hipMemsetAsync(h->lim_ctrl.p, 0, 16, h->stream));
    }
    // behind the device's previous limiter launch if another handle queued it (LimiterChain); a handle that is alone
    // on its device records nothing: its launches are ordered by its one stream
    LimiterChain& chain = g_limiter_chain[h->device % MAX_DEVICES];
    std::unique_lock<std::mutex> lock(chain.mu);
    const bool shared = chain.live > 1;
    if (shared && chain.last && chain.last != h->lim_done) HIP_TRY(hipStreamWaitEvent(h->stream, chain.last, 0));
    int rc = 0;
    switch (lp.general) {
        case 0: rc = launch_limiter(h, a, lp.threads); break;
        case 2: rc = launch_limiter_general<2>(h, a, lp); break;
        default: rc = launch_limiter_general<3>(h, a, lp); break;
    }
    if (rc == 0 && shared) {
        HIP_TRY(hipEventRecord(h->lim_done, h->stream));
        chain.last = h->lim_done;
    }
    return rc;
}
