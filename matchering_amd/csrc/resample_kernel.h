// Sample-rate conversion on the device (matchering/checker.py:30-45): the polyphase sum of resample_plan.h, one
// output frame per thread.
//
// A workgroup takes RESAMPLE_BLOCK consecutive outputs t0 .. t0 + 255.  Their input frames form one span of
// (255 M + r0) / L + W frames, which phase 1 copies into LDS (frames outside the track read as zero through the buffer
// range check, as resampy cuts its wings short there); phase 2 is each thread's dot product over the W taps.  The
// weights come from the matrix in OUTPUT order (resample_device_matrix): lane i of a wave reads column (j0 + i) % L
// of tap row k, so a wave's load is 512 contiguous bytes, where a row-per-phase matrix would have every lane on a cache
// line of its own.  Samples are promoted to float64, the sum runs in float64 with explicit fma in tap order, and the
// store rounds once to float32: float32(host result) up to a flip of the last bit where the two orders of summation
// straddle a rounding boundary.  A mono input is summed once and written to both columns (dsp.py:45-46).  What the host
// decides of a launch -- the arguments but the pointers, the grid and the LDS bytes -- is resample_launch, for
// mgx_resample and tests/emu/emu_resample.cpp alike.
#pragma once

#include <cstring>

#include "mgx_hd.h"
#include "resample_plan.h"

namespace mgx {

struct ResampleArgs {
    const float* x;             // [n][channels] float32
    long long n;
    const double* w;            // [W][L], columns in output order
    int L, M, W;
    float* out;                 // [n_out][2]
    long long n_out;
};

// ---- what the host decides (mgx_resample and the emulation alike) ------------------------------------------------------
struct ResampleLaunch {
    unsigned grid;              // workgroups of RESAMPLE_BLOCK outputs
    size_t lds;                 // dynamic LDS: the longest span a workgroup stages, `channels` floats a frame
};
// everything of the arguments but the pointers
inline ResampleLaunch resample_launch(ResampleArgs& a, const ResampleGeometry& g, long long n, long long n_out, int channels) {
    a.n = n, a.n_out = n_out;
    a.L = g.L, a.M = g.M, a.W = g.W;
    return {(unsigned)((n_out + RESAMPLE_BLOCK - 1) / RESAMPLE_BLOCK), (size_t)g.span * channels * sizeof(float)};
}

// what is the same for every thread of a workgroup
struct ResampleTile {
    long long t0;               // first output
    long long first;            // input frame held at LDS slot 0
    unsigned r0;                // (t0 * M) % L: output t0 + i sits at input first + taps - 1 + (r0 + i M) / L
    unsigned j0;                // t0 % L: its column of the matrix
    int span;                   // frames staged
};

MGX_HD ResampleTile resample_tile(const ResampleArgs& a, long long t0) {
    ResampleTile tile;
    const long long at = t0 * a.M;
    const long long left = a.n_out - t0;
    const int count = left < RESAMPLE_BLOCK ? (int)left : RESAMPLE_BLOCK;
    tile.t0 = t0;
    tile.r0 = (unsigned)(at % a.L);
    tile.j0 = (unsigned)(t0 % a.L);
    tile.first = at / a.L - (a.W / 2 - 1);
    tile.span = (int)((tile.r0 + (unsigned)(count - 1) * (unsigned)a.M) / (unsigned)a.L) + a.W;
    return tile;
}

MGX_D double ld_f64(MemView m, unsigned voff, unsigned soff) {
#if defined(__HIPCC__) && !defined(MGX_HOST_EMU)
    typedef unsigned u2_t __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(m.r, voff, soff, 0));
#else
    const float2 bits = ld_f2(m, voff, soff);
    double v;
    memcpy(&v, &bits, sizeof v);
    return v;
#endif
}

// phase 1: the tile's input span -> LDS, `CH` floats per frame
template <int CH>
MGX_D void resample_stage(const ResampleArgs& a, const ResampleTile& tile, float* lds, int tid) {
    const MemView xv = mem_view(a.x, a.n * CH * (long long)sizeof(float));
    for (int s = tid; s < tile.span; s += RESAMPLE_BLOCK) {
        // (a frame before the track wraps to an offset near 4 G, one behind it lies past the view: both read zero)
        const unsigned off = (unsigned)((tile.first + s) * (long long)(CH * sizeof(float)));
        if (CH == 2)
            reinterpret_cast<float2*>(lds)[s] = ld_f2_or_zero(xv, off);
        else
            lds[s] = ld_f1_or_zero(xv, off);
    }
}

// phase 2: output t0 + tid before its rounding to float32 (zero for threads behind the last output)
template <int CH>
MGX_D double2 resample_sum(const ResampleArgs& a, const ResampleTile& tile, const float* lds, int tid) {
    double2 acc;
    acc.x = acc.y = 0.0;
    if (tile.t0 + tid >= a.n_out) return acc;
    const MemView wv = mem_view(a.w, (long long)a.W * a.L * (long long)sizeof(double));
    const unsigned column = (tile.j0 + (unsigned)tid) % (unsigned)a.L;
    const unsigned woff = column * (unsigned)sizeof(double), wrow = (unsigned)a.L * (unsigned)sizeof(double);
    // tap k multiplies x[n - (k - taps)] = slot (n - first) + taps - k = newest - k
    const int newest = (int)((tile.r0 + (unsigned)tid * (unsigned)a.M) / (unsigned)a.L) + a.W - 1;
    // (eight taps' loads in flight per thread: the sum itself stays in tap order)
    _Pragma("unroll 8")
    for (int k = 0; k < a.W; ++k) {
        const double w = ld_f64(wv, woff, (unsigned)k * wrow);
        if (CH == 2) {
            const float2 v = reinterpret_cast<const float2*>(lds)[newest - k];
            acc.x = fma(w, (double)v.x, acc.x);
            acc.y = fma(w, (double)v.y, acc.y);
        } else {
            acc.x = fma(w, (double)lds[newest - k], acc.x);
        }
    }
    if (CH == 1) acc.y = acc.x;
    return acc;
}

MGX_D void resample_store(const ResampleArgs& a, long long t, double2 acc) {
    const MemView ov = mem_view(a.out, a.n_out * (long long)sizeof(float2));
    if (t < a.n_out) st_f2_in_range(ov, (unsigned)(t * (long long)sizeof(float2)), make_float2((float)acc.x, (float)acc.y));
}

#if defined(__HIPCC__) && !defined(MGX_HOST_EMU)
template <int CH>
__global__ __launch_bounds__(RESAMPLE_BLOCK) void k_resample(ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float resample_lds[];
    const ResampleTile tile = resample_tile(a, (long long)blockIdx.x * RESAMPLE_BLOCK);
    resample_stage<CH>(a, tile, resample_lds, threadIdx.x);
    __syncthreads();
    resample_store(a, tile.t0 + threadIdx.x, resample_sum<CH>(a, tile, resample_lds, threadIdx.x));
}
#endif

}  // namespace mgx
