// Sample-rate conversion of resident stereo frames for the deliveries (mgx_convert_rate): the polyphase sum of
// resample_plan.h with each weight loaded once for several outputs.
//
// k_resample (resample_kernel.h) has every thread stream all W weights of its column for ONE output.  Outputs t and
// t + S meet the same phase whenever S is a multiple of L, and their input positions then differ by exactly
// (S / L) M frames.  So a workgroup of 256 threads takes a tile of P S consecutive outputs, S = L ceil(256 / L),
// starting at T0 = tile P S (a multiple of L: phase 0, column 0), stages the tile's input span -- at most
// P (S / L) M + W frames -- into LDS through the buffer range check, and each thread, for every column
// i = tid, tid + 256, ... < S, sums the P outputs T0 + i + q S together: one weight load, then 2 P FMAs against P
// float2 LDS reads at newest_0 + q (S / L) M - k.  The matrix in output order (resample_device_matrix) serves as it is,
// column (T0 + i) % L.  Each output's own sum is k_resample's: float64 samples and weights, explicit fma in tap order
// k = 0 .. W - 1, one rounding to float32 at the store -- the same bits.
//
// P is chosen on the host (convert_rate_tiling): the largest of 8, 4, 2 whose span leaves room for four workgroups on
// a CU (CONVERT_RATE_SPAN_MAX = 5120 frames, 40 KB of the 160: measured, DESIGN.md section 3.14 -- with three the
// kernel loses more to its idle SIMDs than the wider reuse gains), else P = 1 where one period fits RESAMPLE_SPAN_MAX.
// With P = 1 nothing is shared between periods, so a pair whose single period does not fit either (L >= 256 and M + W
// frames too many) falls back to S = 256, k_resample's own tile: no pair mgx_resample accepts is refused here for its
// span.  What the host decides of a launch -- the arguments but the pointers, P, the grid and the LDS bytes -- is
// convert_rate_launch, for mgx_convert_rate and tests/emu/emu_convert_rate.cpp alike.
#pragma once

#include "mgx_hd.h"
#include "resample_kernel.h"
#include "resample_plan.h"

namespace mgx {

constexpr int CONVERT_RATE_BLOCK = 256;                         // threads of a workgroup
constexpr int CONVERT_RATE_P_MAX = 8;                           // outputs a thread sums per weight load, at most
constexpr int CONVERT_RATE_SPAN_MAX = (int)(LDS_PER_CU / 4 / sizeof(float2));   // input frames a tile of P > 1 may stage

struct ConvertRateTiling {
    int P = 0;                  // 8, 4, 2 or 1
    int S = 0;                  // columns of a tile: L ceil(256 / L), or 256 for the fallback at P = 1
    int span = 0;               // input frames a tile stages, at most
};

// `forced` > 0: that P or nothing (P == 0 comes back when its span does not fit the launch's LDS at all) -- the tests
// run every P the kernel could be launched with, not only the rule's choice
inline ConvertRateTiling convert_rate_tiling(const ResampleGeometry& g, int forced = 0) {
    ConvertRateTiling t;
    const int S = g.L * ((CONVERT_RATE_BLOCK + g.L - 1) / g.L);
    for (int P = CONVERT_RATE_P_MAX; P >= 1; P >>= 1) {
        if (forced > 0 && P != forced) continue;
        const long long span = (long long)P * (S / g.L) * g.M + g.W;
        if (span <= (forced > 0 || P == 1 ? RESAMPLE_SPAN_MAX : CONVERT_RATE_SPAN_MAX)) {
            t.P = P, t.S = S, t.span = (int)span;
            return t;
        }
    }
    if (forced <= 1) t.P = 1, t.S = RESAMPLE_BLOCK, t.span = g.span;        // (resample_geometry has checked this one)
    return t;
}

struct ConvertRateArgs {
    const float* x;             // [n][2] float32
    long long n;
    const double* w;            // [W][L], columns in output order
    int L, M, W;
    float* out;                 // [n_out][2]
    long long n_out;
    int S;                      // columns of a tile
    int hop;                    // (S / L) M: input frames between outputs t and t + S (used when P > 1 only)
};

// ---- what the host decides (mgx_convert_rate and the emulation alike) --------------------------------------------------
struct ConvertRateLaunch {
    int P;                      // the instantiation, as convert_rate_tiling gives it (0: `forced` does not fit, nothing is filled)
    unsigned grid;              // tiles of P S outputs
    size_t lds;                 // dynamic LDS: the tiling's span as float2 frames
};
// everything of the arguments but the pointers
inline ConvertRateLaunch convert_rate_launch(ConvertRateArgs& a, const ResampleGeometry& g, long long n, long long n_out,
                                             int forced = 0) {
    const ConvertRateTiling t = convert_rate_tiling(g, forced);
    if (t.P == 0) return {};
    a.n = n, a.n_out = n_out;
    a.L = g.L, a.M = g.M, a.W = g.W;
    a.S = t.S, a.hop = t.S / g.L * g.M;
    const long long tile = (long long)t.P * t.S;
    return {t.P, (unsigned)((n_out + tile - 1) / tile), (size_t)t.span * sizeof(float2)};
}

// what is the same for every thread of a workgroup
struct ConvertRateTile {
    long long t0;               // first output
    long long first;            // input frame held at LDS slot 0
    unsigned r0;                // (t0 M) % L -- 0 whenever S is a multiple of L
    unsigned j0;                // t0 % L, likewise
    int count;                  // outputs of this tile that exist
    int span;                   // frames staged
};

MGX_HD ConvertRateTile convert_rate_tile(const ConvertRateArgs& a, int P, long long index) {
    ConvertRateTile tile;
    const long long size = (long long)P * a.S;
    tile.t0 = index * size;
    const long long at = tile.t0 * a.M, left = a.n_out - tile.t0;
    tile.count = (int)(left < size ? left : size);
    tile.r0 = (unsigned)(at % a.L);
    tile.j0 = (unsigned)(tile.t0 % a.L);
    tile.first = at / a.L - (a.W / 2 - 1);
    tile.span = (int)((tile.r0 + (long long)(tile.count - 1) * a.M) / a.L) + a.W;
    return tile;
}

// phase 1: the tile's input span -> LDS as float2 frames (resample_stage<2> over this tile's span)
MGX_D void convert_rate_stage(const ConvertRateArgs& a, const ConvertRateTile& tile, float* lds, int tid) {
    const MemView xv = mem_view(a.x, a.n * (long long)sizeof(float2));
    for (int s = tid; s < tile.span; s += CONVERT_RATE_BLOCK) {
        // (a frame before the track wraps to an offset near 4 G, one behind it lies past the view: both read zero)
        const unsigned off = (unsigned)((tile.first + s) * (long long)sizeof(float2));
        reinterpret_cast<float2*>(lds)[s] = ld_f2_or_zero(xv, off);
    }
}

// phase 2: outputs t0 + i + q S, q < P, of column i before their rounding to float32.  Returns how many of them
// exist; the sums of the others are not stored, and they are taken from the slots of q = 0 so that no slot the stage
// did not write is read.
template <int P>
MGX_D int convert_rate_sum(const ConvertRateArgs& a, const ConvertRateTile& tile, const float* lds, int i, double2* acc) {
    MGX_UNROLL
    for (int q = 0; q < P; ++q) acc[q].x = acc[q].y = 0.0;
    if (i >= tile.count) return 0;
    const int live = (tile.count - 1 - i) / a.S + 1;
    const MemView wv = mem_view(a.w, (long long)a.W * a.L * (long long)sizeof(double));
    const unsigned column = (tile.j0 + (unsigned)i) % (unsigned)a.L;
    const unsigned woff = column * (unsigned)sizeof(double), wrow = (unsigned)a.L * (unsigned)sizeof(double);
    // tap k multiplies slot newest - k (resample_sum), and output q sits q hops further on
    const int newest = (int)((tile.r0 + (unsigned)i * (unsigned)a.M) / (unsigned)a.L) + a.W - 1;
    int slot[P];
    MGX_UNROLL
    for (int q = 0; q < P; ++q) slot[q] = newest + (q < live ? q * a.hop : 0);
    const float2* frames = reinterpret_cast<const float2*>(lds);
    // (four taps' weights in flight per thread: each sum stays in tap order)
    _Pragma("unroll 4")
    for (int k = 0; k < a.W; ++k) {
        const double w = ld_f64(wv, woff, (unsigned)k * wrow);
        MGX_UNROLL
        for (int q = 0; q < P; ++q) {
            const float2 v = frames[slot[q] - k];
            acc[q].x = fma(w, (double)v.x, acc[q].x);
            acc[q].y = fma(w, (double)v.y, acc[q].y);
        }
    }
    return live;
}

template <int P>
MGX_D void convert_rate_store(const ConvertRateArgs& a, const ConvertRateTile& tile, int i, int live, const double2* acc) {
    const MemView ov = mem_view(a.out, a.n_out * (long long)sizeof(float2));
    MGX_UNROLL
    for (int q = 0; q < P; ++q) {
        const long long t = tile.t0 + i + (long long)q * a.S;
        if (q < live) st_f2_in_range(ov, (unsigned)(t * (long long)sizeof(float2)), make_float2((float)acc[q].x, (float)acc[q].y));
    }
}

#if defined(__HIPCC__) && !defined(MGX_HOST_EMU)
template <int P>
__global__ __launch_bounds__(CONVERT_RATE_BLOCK) void k_convert_rate(ConvertRateArgs a) {
    extern __shared__ __attribute__((aligned(16))) float convert_rate_lds[];
    const ConvertRateTile tile = convert_rate_tile(a, P, (long long)blockIdx.x);
    convert_rate_stage(a, tile, convert_rate_lds, threadIdx.x);
    __syncthreads();
    for (int i = threadIdx.x; i < a.S; i += CONVERT_RATE_BLOCK) {
        double2 acc[P];
        const int live = convert_rate_sum<P>(a, tile, convert_rate_lds, i, acc);
        convert_rate_store<P>(a, tile, i, live, acc);
    }
}
#endif

}  // namespace mgx
