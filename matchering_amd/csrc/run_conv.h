// Stage 2's second half on the host side: the convolution's launches (conv2_kernel.h, conv_delay_kernel.h,
// conv_wide_kernel.h, small_fft_kernels.h) and the clipped piece sums.
#pragma once

#include "handle.h"

// The FFT convolution (run_conv) comes in three forms.  They share one launch path: the filter spectra under
// MGX_STAGE_FILTER_SPECTRA, a peak per block in h->block_peak, a grid sized by the workgroups the chip holds at once,
// and the main kernel under MGX_STAGE_CONVOLVE.  They differ in their filter-spectra kernel, block hop and grid:
//   CONV_QUEUE: k_conv<LOG2N, MULTI> on blocks of N frames; a persistent grid, a multiple of 8, that draws its blocks
//               from the queue counters
//   CONV_DELAY: k_conv_delay<LOG2N>, taps = N in two partitions (config #5: 16384 taps on N = 16384 blocks), the
//               frequency-domain delay line of conv_delay_kernel.h; blocks of N/2 frames, a run of consecutive blocks
//               per workgroup (every run costs one extra forward transform, so runs are as long as the chip allows)
//   CONV_WIDE:  k_conv_wide<LOG2N>, F taps on N = 4F (conv_wide_kernel.h; F = 4096 on N = 16384); blocks of 3N/4
//               frames, one per workgroup, dealt round-robin
enum ConvForm { CONV_QUEUE, CONV_DELAY, CONV_WIDE };
// The two launches of a convolution can be queued apart: the filter spectra belong to a master call's front half (on
// h->fq), the main kernel to its back half (on h->stream).
enum ConvPhases { CONV_SPECTRA = 1, CONV_MAIN = 2, CONV_BOTH = 3 };

// *blocks: the number of blocks, one peak each in h->block_peak
template <int LOG2N, ConvForm FORM, bool MULTI = false>
static int launch_conv(mgx_handle* h, Conv2Args a, const float* taps_dev, double gain, const double* gain_ptr,
                       long long* blocks, int phases) {
    using F = Fft2<LOG2N>;
    CallContext& cx = context(h);
    const size_t lds = conv_lds_bytes<LOG2N>();
    void (*kernel)(Conv2Args);
    long long hop;                                              // input frames from one block to the next
    if constexpr (FORM == CONV_QUEUE) {
        kernel = k_conv<LOG2N, MULTI>;
        hop = F::N;
    } else if constexpr (FORM == CONV_DELAY) {
        kernel = k_conv_delay<LOG2N>;
        hop = ConvDelay<LOG2N>::HOP;
    } else {
        kernel = k_conv_wide<LOG2N>;
        hop = ConvWide<LOG2N>::HOP;
    }
    if (phases & CONV_SPECTRA) {
        if constexpr (FORM == CONV_WIDE) {
            MGX_TRY(allow_lds(k_conv_wide_prep<LOG2N>, lds));
        } else {
            MGX_TRY(allow_lds(k_conv_prep<LOG2N>, lds));
        }
        StageScope scope(h, MGX_STAGE_FILTER_SPECTRA);
        if constexpr (FORM == CONV_WIDE) {
            hipLaunchKernelGGL(k_conv_wide_prep<LOG2N>, dim3(2), dim3(F::T), lds, h->fq, taps_dev, a.tw,
                               (float2*)cx.filt.p, gain_ptr, gain);
        } else {
            hipLaunchKernelGGL(k_conv_prep<LOG2N>, dim3(2 * a.parts), dim3(F::T), lds, h->fq, taps_dev, a.tw,
                               (float2*)cx.filt.p, a.parts, gain_ptr, gain);
        }
    }
    HIP_TRY(hipGetLastError());
    if (!(phases & CONV_MAIN)) return 0;
    MGX_TRY(allow_lds(kernel, lds));
    a.npairs = (a.n + hop - 1) / hop;
    MGX_TRY(ensure(h, h->block_peak, (size_t)a.npairs * sizeof(float)));
    a.pair_peak = (float*)h->block_peak.p;
    const long long fit = (long long)h->cus * workgroups_per_cu(F::T, lds);
    unsigned grid;
    if constexpr (FORM == CONV_QUEUE) {
        if (!h->conv_queue.p) {                  // zero once: every launch leaves the counters at zero
            MGX_TRY(ensure(h, h->conv_queue, 64));
            HIP_TRY(hipMemsetAsync(h->conv_queue.p, 0, 64, h->stream));
        }
        a.queue = (unsigned*)h->conv_queue.p;
        grid = (unsigned)(((std::min(a.npairs, fit) + 7) / 8) * 8);
    } else if constexpr (FORM == CONV_DELAY) {
        a.run = (int)std::max<long long>(1, (a.npairs + fit - 1) / fit);
        grid = (unsigned)((a.npairs + a.run - 1) / a.run);
    } else {
        grid = (unsigned)std::min(a.npairs, fit);
    }
    {
        StageScope scope(h, MGX_STAGE_CONVOLVE);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(F::T), lds, h->stream, a);
    }
    HIP_TRY(hipGetLastError());
    *blocks = a.npairs;
    return 0;
}

// taps_dev: [2][F] float (mid then side) already on the device.  F <= 8192: one overlap-save block of
// N = 2F per filter; longer filters (config #5: 16 k taps at 96 kHz) are cut into K = F/8192
// partitions on N = 16384 blocks (uniformly partitioned overlap-save), because N = 2F no longer fits
// a CU's LDS.  (Round 2 used K = F/4096 partitions on N = 8192 blocks: K + 1 transforms of 8192 points
// per channel and 8192 output frames, 325 flop per frame and channel; K/2 + 1 of 16384 points per 16384
// frames are 210.)
constexpr int LONG_FIR_LOG2N = 14;
constexpr int WIDE_LOG2N = 14;                                  // CONV_WIDE: 4096 taps on 16384-point blocks
static int run_conv(mgx_handle* h, const float* x, long long n, int taps, const float* taps_dev, double gain,
                    float* y, float* ymid, long long* npairs_out, const double* gain_ptr = nullptr,
                    int phases = CONV_BOTH) {
    CallContext& cx = context(h);
    const int l = ilog2_exact(taps);
    if (l < 0) return fail(MGX_ERR_ARGUMENT, "FIR length must be a power of two");
    MGX_TRY(check_length(n));
    if (taps <= CONV_DIRECT_MAX_TAPS) {                          // 2 .. 32 taps: in the time domain (small_fft_kernels.h)
        if (!(phases & CONV_MAIN)) return 0;                     // (no filter spectra)
        const long long tiles = (n + CONV_DIRECT_TILE - 1) / CONV_DIRECT_TILE;
        MGX_TRY(ensure(h, h->block_peak, (size_t)tiles * sizeof(float)));
        if (npairs_out) *npairs_out = tiles;
        StageScope scope(h, MGX_STAGE_CONVOLVE);
        hipLaunchKernelGGL(k_conv_direct, dim3((unsigned)tiles), dim3(256), 0, h->stream, reinterpret_cast<const float2*>(x),
                           (long long)n, taps_dev, taps, gain_ptr, gain, reinterpret_cast<float2*>(y), ymid,
                           (float*)h->block_peak.p);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // 4096 taps (the reference's default fft_size) on 16384-point blocks, three quarters of a block fresh output
    const bool wide = taps == 4096 && !h->no_conv_wide;
    // (N = 4F -- 4096 taps on 16384-point blocks, 187 instead of 260 flop per frame -- was retried in round 4 with the
    // register diet the kernel has had since round 1: 264 against 148 us, profiles/r04_g_conv_n4f.txt)
    const int log2b = wide ? WIDE_LOG2N : std::min(l + 1, LONG_FIR_LOG2N);
    const size_t nb = (size_t)1 << log2b;
    const int parts = wide ? 1 : (int)((size_t)2 * taps / nb);
    MGX_TRY(ensure(h, cx.filt, 2 * (size_t)parts * nb * sizeof(float2)));
    Conv2Args a;
    a.x = reinterpret_cast<const float2*>(x);
    a.n = n;
    a.y = reinterpret_cast<float2*>(y);
    a.ymid = ymid;
    a.h_mid = (const float2*)cx.filt.p;
    a.h_side = (const float2*)cx.filt.p + (size_t)parts * nb;
    a.parts = parts;
    a.queue = nullptr;
    a.run = 0;
    MGX_TRY(get_twiddles(h, log2b, &a.tw));
    long long blocks = 0;
    if (wide) {
        MGX_TRY((launch_conv<WIDE_LOG2N, CONV_WIDE>(h, a, taps_dev, gain, gain_ptr, &blocks, phases)));
    } else if (parts == 2 && !h->no_conv_delay) {
        MGX_TRY((launch_conv<LONG_FIR_LOG2N, CONV_DELAY>(h, a, taps_dev, gain, gain_ptr, &blocks, phases)));
    } else if (parts > 1) {
        MGX_TRY((launch_conv<LONG_FIR_LOG2N, CONV_QUEUE, true>(h, a, taps_dev, gain, gain_ptr, &blocks, phases)));
    } else {
        switch (log2b) {
#define CASE(L) case L: MGX_TRY((launch_conv<L, CONV_QUEUE>(h, a, taps_dev, gain, gain_ptr, &blocks, phases))); break;
            CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14)
#undef CASE
            default: return fail(MGX_ERR_UNSUPPORTED, "FIR length not supported by the convolution kernel");
        }
    }
    if (npairs_out) *npairs_out = blocks;
    return 0;
}

static int clipped_chunks(int divisions) { return std::max(1, std::min(1024, (2048 + divisions - 1) / divisions)); }

static int run_clipped_sumsq(mgx_handle* h, const float* mid, long long piece, int divisions,
                             const double* gain_ptr, double gain_mul, int* chunks_out) {
    const int chunks = clipped_chunks(divisions);
    MGX_TRY(ensure(h, h->partial, (size_t)divisions * chunks * sizeof(double)));
    hipLaunchKernelGGL(k_clipped_sumsq, dim3(divisions * chunks), dim3(256), 0, h->stream, mid, piece, chunks,
                       gain_ptr, gain_mul, (double*)h->partial.p);
    HIP_TRY(hipGetLastError());
    if (chunks_out) *chunks_out = chunks;
    return 0;
}
