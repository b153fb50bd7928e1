// Loudness levels and loud-piece spectra on the device (match_levels.py:62-71,93-103; match_frequencies.py:30-42):
// the piece sums of the analysis workgroups' partials, the loud-piece decision by a workgroup (decide_loud) and by a
// single wave (wave_decide: k_match_curve in fir_kernels.h and the correction kernels use it), and the stage-level
// kernels k_levels, k_average_spectra and k_finish_spectra.  Device only.
#pragma once

#include "analysis2_kernel.h"
#include "wave_util.h"

namespace mgx {

// ---- piece statistics -> decisions (match_levels.py:62-71,93-103), one 1024-thread workgroup ----
// Step 1: wave w sums the chunk partials of pieces w, w+16, ... (lanes = chunks) into LDS.
// Step 2: thread d owns piece d: rms, mean of squares, rms >= average, RMS of the loud ones.
// All reductions are fixed trees, so results are run-to-run identical.
__device__ __forceinline__ void piece_sums_to_lds(const double* partial, int chunks, int divisions, double* sums) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    for (int d = wave; d < divisions; d += nwaves) {
        double s = 0.0;
        for (int ch = lane; ch < chunks; ch += 64) s += partial[(size_t)d * chunks + ch];
        s = wave_sum(s);
        if (lane == 0) sums[d] = s;
    }
    __syncthreads();
}
// The same sums with L lanes side by side on a piece (L a power of two, as many as the workgroup has for
// `divisions` pieces, at most 64) and a butterfly over them: a fixed order too, and no wave walks alone
// through its pieces.
__device__ __forceinline__ void piece_sums_by_groups(const double* partial, int chunks, int divisions, double* sums) {
    int l = 64;
    while (l > 1 && l * divisions > (int)blockDim.x) l >>= 1;
    const int part = threadIdx.x & (l - 1), per_pass = blockDim.x / l;
    for (int d0 = 0; d0 < divisions; d0 += per_pass) {
        const int d = d0 + threadIdx.x / l;
        double s = 0.0;
        if (d < divisions)
            for (int ch = part; ch < chunks; ch += l) s += partial[(size_t)d * chunks + ch];
        for (int o = l >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (d < divisions && part == 0) sums[d] = s;
    }
    __syncthreads();
}
// returns (on every thread) average rms, match rms and the loud count; optionally stores rms/loud
template <int THREADS>
__device__ __forceinline__ void decide_loud(const double* sums, int divisions, long long piece, double inv_c,
                                            double* red, double* rms_out, int* loud_out, double& avg,
                                            double& match, int& count) {
    double acc = 0.0;
    for (int d = threadIdx.x; d < divisions; d += blockDim.x) {
        const double r = sqrt(sums[d] / (double)piece) * inv_c;
        acc += r * r;
    }
    double tot = block_sum<THREADS>(acc, red);
    if (threadIdx.x == 0) red[16] = sqrt(tot / divisions);
    __syncthreads();
    avg = red[16];
    double lacc = 0.0, lcnt = 0.0;
    for (int d = threadIdx.x; d < divisions; d += blockDim.x) {
        const double r = sqrt(sums[d] / (double)piece) * inv_c;
        const bool l = r >= avg;
        if (l) { lacc += r * r; lcnt += 1.0; }
        if (rms_out) rms_out[d] = r;
        if (loud_out) loud_out[d] = l ? 1 : 0;
    }
    __syncthreads();
    tot = block_sum<THREADS>(lacc, red);
    if (threadIdx.x == 0) red[17] = tot;
    __syncthreads();
    const double cnt = block_sum<THREADS>(lcnt, red + 18);
    if (threadIdx.x == 0) red[40] = cnt;
    __syncthreads();
    count = (int)red[40];
    match = sqrt(red[17] / red[40]);
}
// The piece decisions of match_levels.py:62-71,93-103 by ONE wave, without a barrier: sums[d] = sum of
// mid^2 of piece d (LDS); every lane returns the same average rms, match rms and loud count, and the loud
// flags go to `loud_out` (LDS).  Lane-strided loops and butterfly sums: a fixed order.
__device__ __forceinline__ void wave_decide(const double* sums, int divisions, long long piece, double inv_c,
                                            double* rms_out, int* loud_out, double& avg, double& match, int& count) {
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int d = lane; d < divisions; d += 64) {
        const double r = sqrt(sums[d] / (double)piece) * inv_c;
        acc += r * r;
    }
    avg = sqrt(wave_sum(acc) / divisions);
    double lacc = 0.0, lcnt = 0.0;
    for (int d = lane; d < divisions; d += 64) {
        const double r = sqrt(sums[d] / (double)piece) * inv_c;
        const bool l = r >= avg;
        if (l) { lacc += r * r; lcnt += 1.0; }
        if (rms_out) rms_out[d] = r;
        if (loud_out) loud_out[d] = l ? 1 : 0;
    }
    const double cnt = wave_sum(lcnt);
    count = (int)cnt;
    match = sqrt(wave_sum(lacc) / cnt);
}

struct LevelsArgs {
    const double* wg_sumsq;
    const float* wg_peak;
    int chunks_per_piece, divisions;
    long long piece;
    int is_reference;
    TrackStats* st;
    double* rms;
    int* loud;
};
__device__ __forceinline__ void levels_body(const LevelsArgs& t, double threshold, double eps) {
    MGX_LDS;
    double* red = reinterpret_cast<double*>(mgx_smem);          // 64 doubles of reduction scratch
    double* sums = red + 64;                                     // [divisions]
    float* fred = reinterpret_cast<float*>(red + 52);
    float m = 0.f;
    for (int w = threadIdx.x; w < t.divisions * t.chunks_per_piece; w += blockDim.x) m = fmaxf(m, t.wg_peak[w]);
    const float pk = block_max<1024>(m, fred);
    if (threadIdx.x == 0) red[41] = (double)pk;
    __syncthreads();
    const double peak = red[41];
    double c = 1.0;
    if (t.is_reference && peak < threshold) c = fmax(eps, peak / threshold);     // dsp.py:98-99
    piece_sums_to_lds(t.wg_sumsq, t.chunks_per_piece, t.divisions, sums);
    double avg, match;
    int count;
    decide_loud<1024>(sums, t.divisions, t.piece, 1.0 / c, red, t.rms, t.loud, avg, match, count);
    if (threadIdx.x == 0) {
        TrackStats s;
        s.peak = peak;
        s.amplitude_c = c;
        s.average_rms = avg;
        s.match_rms = match;
        s.divisions = t.divisions;
        s.loud_count = count;
        s.piece = t.piece;
        *t.st = s;
    }
}
// one workgroup per track: grid = 1 (a single track) or 2 (target, reference)
__global__ __launch_bounds__(1024) void k_levels(LevelsArgs t0, LevelsArgs t1, double threshold, double eps) {
    levels_body(blockIdx.x == 0 ? t0 : t1, threshold, eps);
}

// mean over loud pieces and segments of |rfft|/F (match_frequencies.py:42), float64
// Stage 1 of a fixed-order two-stage sum: grid (bin tiles of 64, 2 planes, SPEC_SLICES); a
// workgroup = 64 bins x 16 lanes over its slice of the analysis workgroups.  Output
// part[z][plane][bins] (unscaled sums over the LOUD pieces' workgroups); the consumer adds
// the SPEC_SLICES slices and applies spectrum_scale().
constexpr int SPEC_SLICES = 8;
struct SpectraArgs {
    const float* wg_spec;
    const int* loud;
    int chunks_per_piece, nwg;
    double* part;
};
// grid (bin tiles of 64, 2 planes, SPEC_SLICES * tracks)
__global__ __launch_bounds__(1024) void k_average_spectra(SpectraArgs t0, SpectraArgs t1, int bins) {
    __shared__ double red[1024];
    const SpectraArgs& t = blockIdx.z < SPEC_SLICES ? t0 : t1;
    const int bin = blockIdx.x * 64 + (threadIdx.x & 63), lane = threadIdx.x >> 6;
    const int plane = blockIdx.y, z = blockIdx.z % SPEC_SLICES;
    const int per = (t.nwg + SPEC_SLICES - 1) / SPEC_SLICES;
    const int w0 = z * per, w1 = min(t.nwg, w0 + per);
    double s = 0.0;
    if (bin < bins) {
        for (int w = w0 + lane; w < w1; w += 16)
            if (t.loud[w / t.chunks_per_piece]) s += (double)t.wg_spec[((size_t)w * 2 + plane) * bins + bin];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (lane == 0 && bin < bins) {
        double acc = 0.0;
#pragma unroll
        for (int l = 0; l < 16; ++l) acc += red[l * 64 + (threadIdx.x & 63)];
        t.part[((size_t)z * 2 + plane) * bins + bin] = acc;
    }
}
__device__ __forceinline__ double spectrum_scale(const TrackStats* st, int segs_per_piece, int fft) {
    return 1.0 / ((double)st->loud_count * (double)segs_per_piece * (double)fft * st->amplitude_c);
}
__device__ __forceinline__ double spectrum_at(const double* part, int plane, int bins, int k) {
    double t = 0.0;
#pragma unroll
    for (int z = 0; z < SPEC_SLICES; ++z) t += part[((size_t)z * 2 + plane) * bins + k];
    return t;
}
// mean |rfft|/F over the loud pieces (match_frequencies.py:42) for the stage-level API
__global__ void k_finish_spectra(const double* part, const TrackStats* st, int segs_per_piece, int fft,
                                 double* avg /* [2][bins] */) {
    const int bins = fft / 2 + 1;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * bins) return;
    avg[i] = spectrum_at(part, i / bins, bins, i % bins) * spectrum_scale(st, segs_per_piece, fft);
}

}  // namespace mgx
