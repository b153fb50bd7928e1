// Visuals: the spectrogram and the waveform overview of frames that are in HBM (include/mgx.h, "Visuals"; DESIGN.md
// section 3.18).  No counterpart in the reference: a new surface like the meter and the audit.
//
// k_spectrogram<LOG2N>: one workgroup of Fft2<LOG2N>::T threads takes a run of at most SPECTRO_RUN_CAP consecutive hops
// of ONE output column.  Per hop: the N frames centred on frame t * hop are loaded through a buffer view (frames past
// the end of the track read zero by the range check; frames before frame 0 are selected to zero explicitly, no offset is
// ever formed from a negative frame), multiplied by the float32 window from global memory, and the two real channels
// (left / right, or mid / side as Analysis2Block::to_ms forms them) go through ONE complex transform, z = a + j b.  The
// last pass leaves every thread one row of bins; with the mirror row's upper half (analysis2_kernel.h: phase_row) the
// thread separates |2 A_k|^2 = |Z_k + conj Z_{N-k}|^2 and |2 B_k|^2 = |Z_k - conj Z_{N-k}|^2 for the lower half of its
// row -- no square root -- and adds them to float32 accumulators in registers, in hop order.  At the end the
// accumulators go out as the workgroup's partial spectrum [2][N/2+1].
// k_spectro_pool: one thread per output value (column, channel, band) adds the column's partials in workgroup order and
// the band's bins in bin order, all in float64, and scales: the mean over hops and bins times (2 / sum w)^2.
// k_overview: one workgroup per (column, share of OVERVIEW_SHARE frames): per channel the least and the largest sample
// (fminf / fmaxf: a NaN is skipped) and the float64 sum of squares, reduced over lanes by a fixed butterfly and over
// waves in wave order.  k_overview_fold: one thread per column folds its shares in order.
// Two launches each, no workgroup waits for another, no atomics: two calls give the same bits.
#pragma once

#include "analysis2_kernel.h"
#include "visuals_plan.h"

namespace mgx {

struct SpectroArgs {
    const float2* x;            // (n, 2) interleaved
    long long n;
    int hop;
    long long hops;             // T
    int columns;                // W
    int parts;                  // workgroups per column
    int channels;               // 0: left / right, 1: mid / side
    int bands;                  // B
    const float* window;        // [N] float32
    const float2* tw;           // the transform's twiddles
    float* part;                // [columns * parts][2][N/2+1]: sums of |2 A_k|^2, |2 B_k|^2 over the workgroup's hops
    const int* edges;           // [B + 1]
    double scale;               // (2 / sum w)^2 / 4
    float* out;                 // [columns][2][B]
};

struct OverviewArgs {
    const float2* x;
    long long n;
    int columns;
    int parts;                  // workgroups per column
    float* part_minmax;         // [columns * parts][2][2]: channel, {least, largest}
    double* part_sumsq;         // [columns * parts][2]
    float* minmax;              // [columns][2][2]
    double* sumsq;              // [columns][2]
};

template <int LOG2N>
struct SpectroBlock {
    using AB = Analysis2Block<LOG2N>;
    using F = Fft2<LOG2N>;
    static constexpr int N = F::N;
    static constexpr int T = F::T;
    static constexpr int R0 = F::R0;
    static constexpr int RL = F::RL;
    static constexpr int S0 = F::S(0);
    static constexpr int CNT0 = F::CNT(0);
    using Persist = typename AB::Persist;
    using Row = typename AB::Row;

    struct Thread {
        float acc[2][RL / 2 + 1];      // bins (row, q < RL/2) of both channels; [RL/2]: bin N/2 on thread 0
    };
    static MGX_HD void init(Thread& t) {
        MGX_UNROLL
        for (int c = 0; c < 2; ++c) {
            MGX_UNROLL
            for (int q = 0; q <= RL / 2; ++q) t.acc[c][q] = 0.f;
        }
    }
    // first frame of hop t: may be negative (the first hops) and may leave less than N frames before the end
    static MGX_HD long long hop_start(long long t, int hop) { return t * (long long)hop - N / 2; }

    // the hop's frames times the window, as two channels -> pass 0 -> LDS
    static MGX_HD void phase_load(int tid, long long start, const SpectroArgs& a, const Persist& ps, float2* lds) {
        if (!AB::active0(tid)) return;
        // one butterfly per thread (4096 and 16384 points at 128 registers among them): the twiddles are built as they
        // are used, behind the loads, so that the full set never lives beside the hop's frames
        constexpr bool LEAN = CNT0 == 1;
        typename F::Tw0Full tw;
        if (!LEAN) F::expand_tw0(ps.tw0, tw);
        const MemView src = mem_view(a.x, a.n * 8), win = mem_view(a.window, (long long)N * 4);
        MGX_UNROLL
        for (int c = 0; c < CNT0; ++c) {
            const int i0 = tid + c * T;                          // position in the hop of the butterfly's element 0
            float2 v[R0];
            if (start >= 0) {                                    // (uniform) past the end the range check answers zeros
                const unsigned lane = (unsigned)(start + i0) * 8u;
                MGX_UNROLL
                for (int j = 0; j < R0; ++j) v[j] = ld_f2(src, lane, (unsigned)(j * S0 * 8));
            } else {                                             // a hop that hangs over the START of the track
                MGX_UNROLL
                for (int j = 0; j < R0; ++j) {
                    const long long f = start + i0 + j * S0;
                    const bool before = f < 0;
                    const float2 got = ld_f2(src, before ? 0u : (unsigned)f * 8u, 0u);
                    v[j] = make_float2(before ? 0.f : got.x, before ? 0.f : got.y);
                }
            }
            MGX_UNROLL
            for (int j = 0; j < R0; ++j) {
                const float w = ld_f1(win, (unsigned)i0 * 4u, (unsigned)(j * S0 * 4));
                float p = v[j].x, q = v[j].y;
                if (a.channels != 0) AB::to_ms(v[j], p, q);
                v[j] = make_float2(p * w, q * w);
            }
            if constexpr (LEAN) {
                MGX_SCHED_FENCE();
                F::fwd0_store_lean(v, tid, ps.tw0, lds);
            } else {
                F::fwd0_store(v, tid, c, tw, lds);
            }
        }
    }
    // own lower half + mirror row's upper half -> |2A|^2, |2B|^2 (Analysis2Block::phase_magnitudes without the root)
    static MGX_HD void phase_power(int tid, const Row& own, Thread& t, const float2* lds) {
        if (!F::has_row(tid)) return;
        float2 m[RL / 2];
        F::template load_row_part<RL / 2, RL / 2>(m, F::mirror_row(tid), lds);
        const float2 (&z)[RL / 2 + 1] = own.z;
        const bool r0 = tid == 0;
        MGX_UNROLL
        for (int q = 0; q < RL / 2; ++q) {
            const float2 a = m[RL / 2 - 1 - q];
            const float2 b = q == 0 ? z[0] : m[RL / 2 - q];
            const float2 zm = make_float2(r0 ? b.x : a.x, r0 ? b.y : a.y);
            const float ax = z[q].x + zm.x, ay = z[q].y - zm.y;
            const float bx = z[q].x - zm.x, by = z[q].y + zm.y;
            t.acc[0][q] += fmaf(ax, ax, ay * ay);
            t.acc[1][q] += fmaf(bx, bx, by * by);
        }
        // bin N/2 mirrors into itself: 2A = 2 Re Z, 2B = 2 Im Z (meaningful on thread 0 only)
        const float hx = z[RL / 2].x + z[RL / 2].x, hy = z[RL / 2].y + z[RL / 2].y;
        t.acc[0][RL / 2] += hx * hx;
        t.acc[1][RL / 2] += hy * hy;
    }
    // the accumulators -> the workgroup's partial spectrum; the pair {k, N-k} of bin (row, q) goes to min(k, N-k)
    static MGX_HD void phase_write(int tid, long long wg, const SpectroArgs& a, const Thread& t) {
        if (!F::has_row(tid)) return;
        const int half = N / 2;
        float* c0 = a.part + (size_t)wg * 2 * (half + 1);
        float* c1 = c0 + (half + 1);
        const int k0 = F::frequency_at(tid * RL);
        MGX_UNROLL
        for (int q = 0; q < RL / 2; ++q) {
            const int k = k0 + q * F::L;
            const int kk = k <= half ? k : N - k;
            c0[kk] = t.acc[0][q];
            c1[kk] = t.acc[1][q];
        }
        if (tid == 0) { c0[half] = t.acc[0][RL / 2]; c1[half] = t.acc[1][RL / 2]; }
    }
};

// output value `idx` of [columns][2][bands]: partials in workgroup order, bins in bin order, float64
MGX_HD float spectro_pool_value(const SpectroArgs& a, long long idx, int half) {
    const int b = (int)(idx % a.bands), ch = (int)((idx / a.bands) & 1), c = (int)(idx / (2 * (long long)a.bands));
    long long t0, t1;
    visuals_column(a.hops, a.columns, c, t0, t1);
    const int e0 = a.edges[b], e1 = a.edges[b + 1];
    double acc = 0.0;
    for (int p = 0; p < a.parts; ++p) {
        const float* row = a.part + (((size_t)c * a.parts + p) * 2 + ch) * (half + 1);
        for (int k = e0; k < e1; ++k) acc += (double)row[k];
    }
    return (float)(acc * a.scale / ((double)(t1 - t0) * (double)(e1 - e0)));
}

// one frame into a thread's overview record
struct OverviewThread {
    float lo[2], hi[2];
    double sq[2];
};
MGX_HD void overview_init(OverviewThread& t) {
    t.lo[0] = t.lo[1] = INFINITY;
    t.hi[0] = t.hi[1] = -INFINITY;
    t.sq[0] = t.sq[1] = 0.0;
}
MGX_HD void overview_push(OverviewThread& t, float2 v) {
    t.lo[0] = fminf(t.lo[0], v.x), t.hi[0] = fmaxf(t.hi[0], v.x);
    t.lo[1] = fminf(t.lo[1], v.y), t.hi[1] = fmaxf(t.hi[1], v.y);
    t.sq[0] += (double)v.x * (double)v.x;
    t.sq[1] += (double)v.y * (double)v.y;
}

}  // namespace mgx

#if defined(__HIPCC__) && !defined(MGX_HOST_EMU)
#include "mgx_kernels.h"

namespace mgx {

template <int LOG2N>
__global__ __launch_bounds__(Fft2<LOG2N>::T, analysis_waves_per_simd<LOG2N>()) void k_spectrogram(SpectroArgs a) {
    using SB = SpectroBlock<LOG2N>;
    using AB = Analysis2Block<LOG2N>;
    using F = Fft2<LOG2N>;
    MGX_LDS;
    float2* lds = reinterpret_cast<float2*>(mgx_smem);
    float2* mid_table = lds + F::LDS_ELEMS;
    const int tid = threadIdx.x;
    const long long wg = blockIdx.x;
    const int c = (int)(wg / a.parts), p = (int)(wg % a.parts);
    long long t0, t1, h0, h1;
    visuals_column(a.hops, a.columns, c, t0, t1);
    visuals_part(t0, t1, p, SPECTRO_RUN_CAP, h0, h1);
    typename SB::Thread th;
    SB::init(th);
    typename AB::Persist ps;
    AB::load_persist(tid, a.tw, mid_table, ps);
    __syncthreads();
    for (long long t = h0; t < h1; ++t) {
        SB::phase_load(tid, SB::hop_start(t, a.hop), a, ps, lds);
        lds_barrier();
        fwd_middle_passes<F>(tid, lds, mid_table);
        typename AB::Row own;
        AB::phase_row(tid, own, lds);
        lds_barrier();
        SB::phase_power(tid, own, th, lds);
        lds_barrier();
    }
    SB::phase_write(tid, wg, a, th);
}

template <int UNUSED>
__global__ __launch_bounds__(256) void k_spectro_pool(SpectroArgs a, int half) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.columns * 2 * a.bands) return;
    a.out[idx] = spectro_pool_value(a, idx, half);
}

template <int UNUSED>
__global__ __launch_bounds__(OVERVIEW_THREADS) void k_overview(OverviewArgs a) {
    constexpr int NW = OVERVIEW_THREADS / 64;
    __shared__ float wave_lo[NW][2], wave_hi[NW][2];
    __shared__ double wave_sq[NW][2];
    const int tid = threadIdx.x;
    const long long wg = blockIdx.x;
    const int c = (int)(wg / a.parts), p = (int)(wg % a.parts);
    long long f0, f1, begin, end;
    visuals_column(a.n, a.columns, c, f0, f1);
    visuals_part(f0, f1, p, OVERVIEW_SHARE, begin, end);
    OverviewThread t;
    overview_init(t);
    for (long long f = begin + tid; f < end; f += OVERVIEW_THREADS) overview_push(t, a.x[f]);
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            t.lo[ch] = fminf(t.lo[ch], __shfl_xor(t.lo[ch], o, 64));
            t.hi[ch] = fmaxf(t.hi[ch], __shfl_xor(t.hi[ch], o, 64));
            t.sq[ch] += __shfl_xor(t.sq[ch], o, 64);
        }
    }
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        wave_lo[w][0] = t.lo[0], wave_lo[w][1] = t.lo[1];
        wave_hi[w][0] = t.hi[0], wave_hi[w][1] = t.hi[1];
        wave_sq[w][0] = t.sq[0], wave_sq[w][1] = t.sq[1];
    }
    __syncthreads();
    if (tid < 2) {
        float lo = wave_lo[0][tid], hi = wave_hi[0][tid];
        double sq = wave_sq[0][tid];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            lo = fminf(lo, wave_lo[w][tid]), hi = fmaxf(hi, wave_hi[w][tid]);
            sq += wave_sq[w][tid];
        }
        a.part_minmax[(wg * 2 + tid) * 2] = lo;
        a.part_minmax[(wg * 2 + tid) * 2 + 1] = hi;
        a.part_sumsq[wg * 2 + tid] = sq;
    }
}

template <int UNUSED>
__global__ __launch_bounds__(256) void k_overview_fold(OverviewArgs a) {
    const int idx = blockIdx.x * 256 + threadIdx.x;             // (column, channel)
    if (idx >= a.columns * 2) return;
    const int c = idx >> 1, ch = idx & 1;
    float lo = INFINITY, hi = -INFINITY;
    double sq = 0.0;
    for (int p = 0; p < a.parts; ++p) {
        const size_t at = ((size_t)c * a.parts + p) * 2 + ch;
        lo = fminf(lo, a.part_minmax[at * 2]), hi = fmaxf(hi, a.part_minmax[at * 2 + 1]);
        sq += a.part_sumsq[at];
    }
    a.minmax[idx * 2] = lo, a.minmax[idx * 2 + 1] = hi;
    a.sumsq[idx] = sq;
}

}  // namespace mgx
#endif
