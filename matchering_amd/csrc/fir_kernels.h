// The FIR design on the device (fir_plan.h holds the phase functions and the plan; match_frequencies.py:45-99).
// Device only:
//   * the spline / LOWESS operator kernels (k_fir_unit_a ... k_fir_gather) and the raw curve (k_fir_raw),
//   * k_match_curve: levels + loud-piece spectra + raw matching curve in one launch,
//   * the dense operator (k_fir_band, k_fir_matvec) and its two packed factors (k_fir_unit_fit ... k_fir_apply_b),
//   * tap synthesis: direct (k_fir_taps_direct), by cosine sum (k_fir_taps) and by float64 transform
//     (k_fir_taps_sub, k_fir_taps_combine).
#pragma once

#include "fir_plan.h"
#include "levels_kernels.h"
#include "wave_util.h"

namespace mgx {

// ---------------------------------------------------------------------------
// FIR design on the device (fir_plan.h): four small kernels, no host round trip
// ---------------------------------------------------------------------------
struct FirInputs {
    const double* part_t;        // target spectra partial sums   [SPEC_SLICES][2][bins]
    const double* part_r;        // reference
    const TrackStats* st_t;
    const TrackStats* st_r;
    int segs_t, segs_r;
    double eps;
};
__device__ __forceinline__ FirScratch fir_scratch(double* base, const FirPlanView& pl, int plane) {
    const size_t per = (size_t)3 * pl.bins + (size_t)3 * pl.nlog + pl.lw.anchors;
    double* p = base + (size_t)plane * per;
    FirScratch s;
    s.raw = p;
    s.m1 = s.raw + pl.bins;
    s.smooth = s.m1 + pl.bins;
    s.on_log = s.smooth + pl.bins;
    s.log_s = s.on_log + pl.nlog;
    s.m2 = s.log_s + pl.nlog;
    s.fit = s.m2 + pl.nlog;
    return s;
}
__device__ __forceinline__ void fir_solve(const SplineTables& sp, const double* y, double* m, Affine* sc) {
    using FD = FirDesign;
    const int tid = threadIdx.x;
    FD::phase_fwd_local(tid, sp, y, sc);
    __syncthreads();
    FD::Scan::scan_groups(sc, tid);
    __syncthreads();
    FD::Scan::scan_top(sc, tid);
    __syncthreads();
    FD::phase_fwd_apply(tid, sp, y, sc, m);
    __syncthreads();
    FD::phase_bwd_local(tid, sp, m, sc);
    __syncthreads();
    FD::Scan::scan_groups(sc, tid);
    __syncthreads();
    FD::Scan::scan_top(sc, tid);
    __syncthreads();
    FD::phase_bwd_apply(tid, sp, sc, m);
    __syncthreads();
    FD::phase_closure(tid, sp, m);
    __syncthreads();
}
// ---- the chain raw -> smooth as ONE dense operator ---------------------------------------------
// For a given Config, smooth = M * raw with a fixed (bins x bins) float64 matrix: splines and
// LOWESS (it = 0) are linear in their input and the pinned bins are rows of M.  M is built once
// per plan ON THE DEVICE by pushing unit vectors through the very kernels above/below
// (k_fir_unit_a, k_fir_lowess, k_fir_b, k_fir_gather); per pair the design is then k_fir_raw +
// one 34 MB matrix-vector product for both channels (k_fir_matvec) instead of ~90 us of serial
// single-workgroup scans.
__global__ __launch_bounds__(1024) void k_fir_unit_a(FirPlanView pl, double* scratch, int col0) {
    MGX_LDS;
    Affine* sc = reinterpret_cast<Affine*>(mgx_smem);
    const int tid = threadIdx.x, plane = blockIdx.x;
    FirScratch s = fir_scratch(scratch, pl, plane);
    for (int k = tid; k < pl.bins; k += 1024) s.raw[k] = k == col0 + plane ? 1.0 : 0.0;
    __syncthreads();
    fir_solve(pl.s1, s.raw, s.m1, sc);
    FirDesign::phase_eval(tid, pl.s1, s.raw, s.m1, s.on_log);
}
// ---- lowess_it > 0: LOWESS is no longer linear in the data, so the chain runs on the curve itself ----
// raw curve -> spline onto the log grid.  grid = 2 (mid, side)
__global__ __launch_bounds__(1024) void k_fir_direct_a(FirPlanView pl, double* scratch, const double* raw /* [2][bins] */) {
    MGX_LDS;
    Affine* sc = reinterpret_cast<Affine*>(mgx_smem);
    const int tid = threadIdx.x, plane = blockIdx.x;
    FirScratch s = fir_scratch(scratch, pl, plane);
    for (int k = tid; k < pl.bins; k += 1024) s.raw[k] = raw[(size_t)plane * pl.bins + k];
    __syncthreads();
    fir_solve(pl.s1, s.raw, s.m1, sc);
    FirDesign::phase_eval(tid, pl.s1, s.raw, s.m1, s.on_log);
}
// the k-th smallest (k from 0) of n non-negative doubles, by bisection on the bit pattern (which orders
// them): 63 counting passes, every thread of the 1024 gets the result.  red: 17 ints of LDS
__device__ __forceinline__ double block_select(const double* v, int n, int k, int* red) {
    const int tid = threadIdx.x;
    unsigned long long lo = 0ull, hi = 0x7ff0000000000000ull;
    while (lo < hi) {
        const unsigned long long mid = lo + ((hi - lo) >> 1);
        int c = 0;
        for (int q = tid; q < n; q += 1024) c += double_bits(v[q]) <= mid ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if ((tid & 63) == 0) red[tid >> 6] = c;
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int w = 0; w < 16; ++w) t += red[w];
            red[16] = t;
        }
        __syncthreads();
        if (red[16] >= k + 1) hi = mid;
        else lo = mid + 1;
        __syncthreads();                      // red[16] is rewritten in the next pass
    }
    return bits_double(lo);
}
// LOWESS with robustness iterations (fir_plan.h: phase_lowess_fit_robust ...), one workgroup per channel;
// work: [2][2][nlog] doubles (robustness weights, residuals).  Leaves the anchors' fits of the last pass
// in s.fit, where k_fir_b picks them up.
__global__ __launch_bounds__(1024) void k_fir_lowess_robust(FirPlanView pl, double* scratch, double* work, int it) {
    __shared__ int red[17];
    const int tid = threadIdx.x, plane = blockIdx.x, n = pl.nlog;
    FirScratch s = fir_scratch(scratch, pl, plane);
    double* robust = work + (size_t)plane * 2 * n;
    double* resid = robust + n;
    FirDesign::phase_robust_init(tid, n, robust);
    __syncthreads();
    for (int pass = 0; pass <= it; ++pass) {
        FirDesign::phase_lowess_fit_robust(tid, pl.lw, s.on_log, robust, s.fit);
        __syncthreads();
        if (pass == it) break;
        FirDesign::phase_lowess_fill(tid, pl.lw, s.fit, s.log_s);
        __syncthreads();
        FirDesign::phase_residuals(tid, n, s.on_log, s.log_s, resid);
        __syncthreads();
        double median = block_select(resid, n, n / 2, red);                       // numpy.median
        if (!(n & 1)) median = 0.5 * (block_select(resid, n, n / 2 - 1, red) + median);
        FirDesign::phase_robust_weights(tid, n, resid, median, robust);
        __syncthreads();
    }
}
// M[i][col0 + c] = smooth of unit vector col0 + c, bin i
__global__ __launch_bounds__(256) void k_fir_gather(FirPlanView pl, double* scratch, int col0, int ncols, double* M) {
    const int c = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (c >= ncols) return;
    const FirScratch s = fir_scratch(scratch, pl, c);
    M[(size_t)i * pl.bins + col0 + c] = s.smooth[i];
}
// raw matching curves of both channels (match_frequencies.py:93-94) + the level gain c0
struct CorrectionState;       // (correction_kernels.h, the stage after this one)
__device__ void correction_reset(CorrectionState* cs, double gain);
__global__ __launch_bounds__(256) void k_fir_raw(FirPlanView pl, FirInputs in, double* raw /* [2][bins] */,
                                                 double* c0_out, CorrectionState* cs_init) {
    const int k = blockIdx.x * 256 + threadIdx.x, plane = blockIdx.y;
    const double c0 = in.st_r->match_rms / fmax(in.eps, in.st_t->match_rms);      // match_levels.py:106-111
    if (plane == 0 && k == 0) {
        *c0_out = c0;
        if (cs_init) correction_reset(cs_init, 1.0);       // stages.py:138-170 starts from gain 1
    }
    if (k >= pl.bins) return;
    const double sc_t = spectrum_scale(in.st_t, in.segs_t, pl.fft) * c0;          // stages.py:90-91
    const double sc_r = spectrum_scale(in.st_r, in.segs_r, pl.fft);
    const double at = spectrum_at(in.part_t, plane, pl.bins, k) * sc_t;
    const double ar = spectrum_at(in.part_r, plane, pl.bins, k) * sc_r;
    raw[(size_t)plane * pl.bins + k] = ar / fmax(pl.min_value, at);
}

// ---- levels + loud-piece spectra + raw matching curve in ONE launch --------------------------------
// k_levels -> k_average_spectra -> k_fir_raw are three dependent launches of a few microseconds of
// work each; here every workgroup re-derives the (tiny) piece decisions of both tracks in its own LDS
// (one batch of loads, the two tracks decided side by side by one wave each), sums its tile of bins
// over the loud workgroup rows of both tracks and writes the raw curve (match_frequencies.py:93-94)
// directly.  Grid (bin tiles of 32, 2 planes) x 1024 threads = 32 bins x 32 row lanes; every sum runs in
// a fixed order.  Workgroup (0, 0) also leaves the TrackStats, the piece tables, the level gain c0
// (stages.py:80-88) and the reset correction state.
struct CurveTrack {
    LevelsArgs lv;
    const float* wg_spec;        // [nwg][2][bins]
    int nwg, segs_per_piece;
};
// LDS carve, in doubles: acc[1024] | scal[16] | sums[2][max_div] | ss[nwg_t + nwg_r] ; then ints loud[2][max_div]
// and floats pk[nwg_t + nwg_r]
__host__ __device__ inline size_t match_curve_lds_bytes(int max_div, int rows) {
    return ((size_t)1024 + 16 + 2 * (size_t)max_div + rows) * 8 + (2 * (size_t)max_div + rows + 4) * 4;
}
// TILE bins x ROWL = 1024 / TILE row lanes per workgroup.  32 x 32 unless 33 x 31 (one idle thread) saves a round of
// workgroups: the spectrum has 2^k + 1 bins, so tiles of 32 leave ONE bin for a last tile per channel, and at
// fft_size 16384 those two workgroups are numbers 513 and 514 on a chip that holds 256 at a time (29 -> 20 us).
template <int TILE>
__global__ __launch_bounds__(1024) void k_match_curve(CurveTrack tt, CurveTrack tr, int bins, int fft, int max_div,
                                                      double threshold, double eps, double curve_floor,
                                                      double* raw /* [2][bins] */, double* c0_out,
                                                      CorrectionState* cs_init, int* error) {
    warm_code(CODE_MATCH_CURVE);
    MGX_LDS;
    const int rows = tt.nwg + tr.nwg;
    double* acc = reinterpret_cast<double*>(mgx_smem);
    double* scal = acc + 1024;                                  // [k*4 + {amplitude_c, match, count, -}]
    double* sums = scal + 16;                                   // [2][max_div]
    double* ss = sums + 2 * max_div;                            // [rows] piece-chunk sums of mid^2, target rows first
    int* loud = reinterpret_cast<int*>(ss + rows);              // [2][max_div]
    float* pk = reinterpret_cast<float*>(loud + 2 * max_div);   // [rows]
    const bool writer = blockIdx.x == 0 && blockIdx.y == 0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // The spectra of the first 16 ROWL workgroup rows of EACH track are asked for before anything else: what is summed
    // depends on the level decisions below, what is loaded does not, so the decisions (two LDS round trips and a
    // wave's worth of arithmetic) run while the loads are in flight.  Buffer views: ONE lane offset per track, the row
    // step is a scalar displacement, and rows past the end of a track read as zero through the range check.
    constexpr int ROWL = 1024 / TILE;
    const int b = threadIdx.x % TILE, row_lane = threadIdx.x / TILE, plane = blockIdx.y;      // (row_lane == ROWL: the idle thread)
    const int bin = row_lane < ROWL ? blockIdx.x * TILE + b : bins;
    const MemView vt = mem_view(tt.wg_spec, (long long)tt.nwg * 2 * bins * 4);
    const MemView vr = mem_view(tr.wg_spec, (long long)tr.nwg * 2 * bins * 4);
    // (a bin past the end reads from past the end of the view: zeros)
    const unsigned lane_off = bin < bins ? (unsigned)((((size_t)row_lane * 2 + plane) * bins + bin) * 4) : 0xfffffff0u;
    const unsigned row_step = (unsigned)((size_t)ROWL * 2 * bins * 4);
    double ssv[2] = {0.0, 0.0};
    float pkv[2] = {0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 2; ++u) {                                // (rows <= 2048: host_params / run_fir_design)
        const int w = threadIdx.x + 1024 * u;
        if (w < rows) {
            const bool second = w >= tt.nwg;
            const LevelsArgs& t = second ? tr.lv : tt.lv;
            const int i = second ? w - tt.nwg : w;
            ssv[u] = t.wg_sumsq[i];
            pkv[u] = t.wg_peak[i];
        }
    }
    float v0[2][16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const unsigned disp = (unsigned)u * row_step;
        v0[0][u] = ld_f1(vt, lane_off, disp);
        v0[1][u] = ld_f1(vr, lane_off, disp);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int w = threadIdx.x + 1024 * u;
        if (w < rows) {
            ss[w] = ssv[u];
            pk[w] = pkv[u];
        }
    }
    for (int w = threadIdx.x + 2048; w < rows; w += 1024) {       // (more rows than that: the plain way)
        const bool second = w >= tt.nwg;
        const LevelsArgs& t = second ? tr.lv : tt.lv;
        const int i = second ? w - tt.nwg : w;
        ss[w] = t.wg_sumsq[i];
        pk[w] = t.wg_peak[i];
    }
    lds_barrier();
    for (int p = threadIdx.x; p < tt.lv.divisions + tr.lv.divisions; p += 1024) {
        const bool second = p >= tt.lv.divisions;
        const LevelsArgs& t = second ? tr.lv : tt.lv;
        const int d = second ? p - tt.lv.divisions : p;
        const double* src = ss + (second ? tt.nwg : 0) + (size_t)d * t.chunks_per_piece;
        double sum = 0.0;
        for (int ch = 0; ch < t.chunks_per_piece; ++ch) sum += src[ch];
        sums[(second ? max_div : 0) + d] = sum;
    }
    lds_barrier();
    if (wave < 2) {                                             // wave 0: target, wave 1: reference
        const int k = wave;
        const LevelsArgs& t = k == 0 ? tt.lv : tr.lv;
        const float* p = pk + (k == 0 ? 0 : tt.nwg);
        float m = 0.f;
        for (int w = lane; w < (k == 0 ? tt.nwg : tr.nwg); w += 64) m = fmaxf(m, p[w]);
        const double peak = (double)wave_max(m);
        double c = 1.0;
        if (t.is_reference && peak < threshold) c = fmax(eps, peak / threshold);     // dsp.py:98-99
        double avg, match;
        int count;
        wave_decide(sums + k * max_div, t.divisions, t.piece, 1.0 / c, writer ? t.rms : nullptr, loud + k * max_div, avg,
                    match, count);
        if (lane == 0) {
            scal[k * 4 + 0] = c;
            scal[k * 4 + 1] = match;
            scal[k * 4 + 2] = (double)count;
        }
        if (writer) {
            for (int d = lane; d < t.divisions; d += 64) t.loud[d] = loud[k * max_div + d];
            if (lane == 0) {
                TrackStats st;
                st.peak = peak;
                st.amplitude_c = c;
                st.average_rms = avg;
                st.match_rms = match;
                st.divisions = t.divisions;
                st.loud_count = count;
                st.piece = t.piece;
                *t.st = st;
                // A NaN or an infinity among the samples: no piece is "loud" (every comparison with NaN fails) or
                // the loud pieces' RMS is not a number.  The reference stops there (match_frequencies.py:42 is
                // handed an empty selection); here the handle's error word makes the next blocking call fail.
                if (error && (count == 0 || !(fabs(match) < 1.0e300))) error[DEVICE_ERROR_SLOT_INPUT] = 1;
            }
        }
    }
    lds_barrier();
    const double c0 = scal[4 + 1] / fmax(eps, scal[1]);         // match_levels.py:106-111
    if (writer && threadIdx.x == 0) {
        *c0_out = c0;
        if (cs_init) correction_reset(cs_init, 1.0);            // stages.py:138-170 starts from gain 1
    }
    // sixteen rows of EACH track per thread and batch: one round trip for a pair of 8-minute tracks
    double sacc[2] = {0.0, 0.0};
    {
        const int longest = max(tt.nwg, tr.nwg);
        // workgroup row -> piece without a division per row: floor(w * ceil(2^32 / d) / 2^32) = w / d for w, d < 2^16
        const unsigned magic[2] = {(unsigned)((0x100000000ull + tt.lv.chunks_per_piece - 1) / tt.lv.chunks_per_piece),
                                   (unsigned)((0x100000000ull + tr.lv.chunks_per_piece - 1) / tr.lv.chunks_per_piece)};
#pragma unroll 1
        for (int w0 = 0; w0 < longest; w0 += ROWL * 16) {
            if (opaque(w0) > 0) {                               // (the first batch is in flight since the top; opaque: one copy of the sums)
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const unsigned disp = (unsigned)(w0 / ROWL + u) * row_step;
                    v0[0][u] = ld_f1(vt, lane_off, disp);
                    v0[1][u] = ld_f1(vr, lane_off, disp);
                }
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const CurveTrack& t = k == 0 ? tt : tr;
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int w = w0 + row_lane + ROWL * u;
                    const int piece = t.lv.chunks_per_piece == 1 ? w : (int)__umulhi((unsigned)w, magic[k]);
                    const bool on = w < t.nwg && loud[k * max_div + (w < t.nwg ? piece : 0)] != 0;
                    sacc[k] += on ? (double)v0[k][u] : 0.0;
                }
            }
        }
    }
    double level[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const CurveTrack& t = k == 0 ? tt : tr;
        acc[threadIdx.x] = sacc[k];
        __syncthreads();
        double total = 0.0;
        if (row_lane == 0) {
#pragma unroll 8
            for (int l = 0; l < ROWL; ++l) total += acc[l * TILE + b];
        }
        // mean over loud pieces and segments of |rfft|/F of the normalised track (match_frequencies.py:42)
        level[k] = total / (scal[k * 4 + 2] * (double)t.segs_per_piece * (double)fft * scal[k * 4 + 0]);
        __syncthreads();
    }
    if (row_lane == 0 && bin < bins)
        raw[(size_t)plane * bins + bin] = level[1] / fmax(curve_floor, level[0] * c0);   // stages.py:90-91 on the target
}

// The operator is numerically banded: LOWESS looks at 3.75 % of the log-frequency grid and the
// splines' influence decays geometrically, so outside a window around the diagonal (about a third of
// the bin index wide) every entry is below 1e-18 of the row's largest.  k_fir_band records that
// window per row once per plan; the product then reads only it (a sixth of the matrix).
constexpr double BAND_EPS = 1e-18;
__global__ __launch_bounds__(256) void k_fir_band(const double* M, int bins, int2* band) {
    __shared__ double dred[4];
    __shared__ int ired[2][4];
    const int row = blockIdx.x, tid = threadIdx.x;
    const double* m = M + (size_t)row * bins;
    double mx = 0.0;
    for (int j = tid; j < bins; j += 256) mx = fmax(mx, fabs(m[j]));
    mx = wave_max_f64(mx);
    if ((tid & 63) == 0) dred[tid >> 6] = mx;
    __syncthreads();
    const double cut = fmax(fmax(dred[0], dred[1]), fmax(dred[2], dred[3])) * BAND_EPS;
    int lo = bins, hi = 0;
    for (int j = tid; j < bins; j += 256)
        if (fabs(m[j]) > cut) { lo = min(lo, j); hi = max(hi, j + 1); }
    for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
    if ((tid & 63) == 0) { ired[0][tid >> 6] = lo; ired[1][tid >> 6] = hi; }
    __syncthreads();
    if (tid == 0) {
        lo = min(min(ired[0][0], ired[0][1]), min(ired[0][2], ired[0][3]));
        hi = max(max(ired[1][0], ired[1][1]), max(ired[1][2], ired[1][3]));
        band[row] = lo < hi ? make_int2(lo, hi) : make_int2(0, 0);
    }
}
// smooth[plane][i] = sum_j M[i][j] raw[plane][j] over the row's window: one 256-thread workgroup per
// row, both channels per pass, ten loads per thread in flight
__global__ __launch_bounds__(256) void k_fir_matvec(FirPlanView pl, const double* M, const int2* band,
                                                    const double* raw, double* scratch) {
    __shared__ double red[2][4];
    const int row = blockIdx.x, tid = threadIdx.x;
    const double* m = M + (size_t)row * pl.bins;
    const double* r0 = raw;
    const double* r1 = raw + pl.bins;
    const int first = band[row].x, last = band[row].y;
    double a0 = 0.0, a1 = 0.0;
    for (int j0 = first + tid; j0 < last; j0 += 256 * 10) {
        double v[10];
#pragma unroll
        for (int u = 0; u < 10; ++u) {
            const int j = j0 + 256 * u;
            v[u] = j < last ? m[j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 10; ++u) {
            const int j = j0 + 256 * u;
            if (j < last) {
                a0 = fma(v[u], r0[j], a0);
                a1 = fma(v[u], r1[j], a1);
            }
        }
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    if ((tid & 63) == 0) { red[0][tid >> 6] = a0; red[1][tid >> 6] = a1; }
    __syncthreads();
    if (tid == 0) {
        fir_scratch(scratch, pl, 0).smooth[row] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        fir_scratch(scratch, pl, 1).smooth[row] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

// ---- the same chain in TWO factors, for fft_size >= 16384 ----------------------------------------------
// raw -> smooth passes through the LOWESS fits at the anchors (match_frequencies.py:62-64 with lowess_delta: only
// ~1/delta = 1000 points of the log grid get a regression, the rest is interpolated between them), so
//     smooth = B * (A * raw),   A = [anchors x bins]: spline onto the log grid + the anchors' regressions,
//                               B = [bins x anchors]: fill between anchors + spline back + pinned bins.
// Both are banded like M (A's row of anchor a covers the linear bins under its 3.75 % neighbourhood, B's row of bin
// i the handful of anchors around it) and stored PACKED, row after row, only the window k_fir_band found:
// 3.4 MB at fft_size 16384 where M is 537 MB (of which the product read 83 MB per pair, 28 us), a few MB more at
// 65536 where M would be 8.6 GB.  Built like M, by pushing unit vectors through the chain's own kernels.
// One 16-byte descriptor per row: its window [first, last) and where it starts in the packed array (one load, not a
// chain of two, in front of a row's data).
struct FactorRow {
    int first, last;
    long long off;
};
// unit anchor `col0 + plane` as the fits, nothing on the raw side (phase_pin reads raw[1])
__global__ __launch_bounds__(256) void k_fir_unit_fit(FirPlanView pl, double* scratch, int col0) {
    const int plane = blockIdx.x;
    FirScratch s = fir_scratch(scratch, pl, plane);
    for (int a = threadIdx.x; a < pl.lw.anchors; a += 256) s.fit[a] = a == col0 + plane ? 1.0 : 0.0;
    if (threadIdx.x == 0) s.raw[1] = 0.0;
}
// dense[i][col0 + c] = (fits | smooth curve) of plane c at i; grid = (ceil(ncols / 256), rows)
__global__ __launch_bounds__(256) void k_fir_gather_plane(FirPlanView pl, double* scratch, int col0, int ncols, int stride,
                                                          int from_fit, double* dense) {
    const int c = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (c >= ncols) return;
    const FirScratch s = fir_scratch(scratch, pl, c);
    dense[(size_t)i * stride + col0 + c] = from_fit ? s.fit[i] : s.smooth[i];
}
// packed[off[row] + j - band[row].x] = dense[row][j] over the row's window; grid = rows
__global__ __launch_bounds__(256) void k_fir_pack(const double* dense, int stride, const FactorRow* rows, double* packed) {
    const int row = blockIdx.x;
    const int first = rows[row].first, last = rows[row].last;
    const double* src = dense + (size_t)row * stride;
    double* dst = packed + rows[row].off - first;
    for (int j = first + threadIdx.x; j < last; j += 256) dst[j] = src[j];
}
// fit[plane][a] = sum_j A[a][j] raw[plane][j]: one 256-thread workgroup per anchor, both channels per pass, the whole
// window in flight at once (the widest is 0.31 * bins + 62 columns: eleven loads per thread at fft_size 16384);
// grid = anchors.  (One WAVE per anchor, the first version, walked the wide windows in five dependent batches:
// 20 us for the two factors against the dense product's 28, profiles/r05_p_fir_factored_first_version.txt.)
__global__ __launch_bounds__(256) void k_fir_apply_a(FirPlanView pl, const double* A, const FactorRow* rows, const double* raw,
                                                     double* scratch) {
    __shared__ double red[2][4];
    const int a = blockIdx.x, tid = threadIdx.x;
    const FactorRow row = rows[a];
    const int first = row.first, last = row.last;
    const double* m = A + row.off - first;
    const double* r0 = raw;
    const double* r1 = raw + pl.bins;
    double a0 = 0.0, a1 = 0.0;
    for (int j0 = first + tid; j0 < last; j0 += 256 * 12) {
        double v[12], x0[12], x1[12];
#pragma unroll
        for (int u = 0; u < 12; ++u) {
            const int j = j0 + 256 * u;
            const bool in = j < last;
            v[u] = in ? m[j] : 0.0;
            x0[u] = in ? r0[j] : 0.0;
            x1[u] = in ? r1[j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 12; ++u) {
            a0 = fma(v[u], x0[u], a0);
            a1 = fma(v[u], x1[u], a1);
        }
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    if ((tid & 63) == 0) { red[0][tid >> 6] = a0; red[1][tid >> 6] = a1; }
    __syncthreads();
    if (tid == 0) {
        fir_scratch(scratch, pl, 0).fit[a] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        fir_scratch(scratch, pl, 1).fit[a] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}
// smooth[plane][i] = sum_a B[i][a] fit[plane][a] (a handful of terms: one thread per bin), bins 0 and 1 pinned
// (match_frequencies.py:72-73); grid = ceil(bins / 256)
__global__ __launch_bounds__(256) void k_fir_apply_b(FirPlanView pl, const double* B, const FactorRow* rows, const double* raw,
                                                     double* scratch) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pl.bins) return;
    const FirScratch s0 = fir_scratch(scratch, pl, 0), s1 = fir_scratch(scratch, pl, 1);
    const FactorRow row = rows[i];
    const int first = row.first, last = row.last;
    const double* m = B + row.off - first;
    double a0 = 0.0, a1 = 0.0;
    for (int a = first; a < last; a += 8) {                      // (windows are 4 - 10 anchors wide: one batch, two at most)
        double v[8], f0[8], f1[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool in = a + u < last;
            v[u] = in ? m[a + u] : 0.0;
            f0[u] = in ? s0.fit[a + u] : 0.0;
            f1[u] = in ? s1.fit[a + u] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            a0 = fma(v[u], f0[u], a0);
            a1 = fma(v[u], f1[u], a1);
        }
    }
    if (i == 0) a0 = a1 = 0.0;
    if (i == 1) { a0 = raw[1]; a1 = raw[pl.bins + 1]; }
    s0.smooth[i] = a0;
    s1.smooth[i] = a1;
}

// fft_size 8 .. 32 (small_fft_kernels.h): taps[i] = hann[i] * irfft(smooth)[(i + F/2) mod F] by the plain cosine sum (fir_plan.h, phase_taps); grid = 2
__global__ __launch_bounds__(1024) void k_fir_taps_direct(FirPlanView pl, const double* scratch, float* taps /* [2][F] */) {
    const int plane = blockIdx.x;
    const FirScratch s = fir_scratch(const_cast<double*>(scratch), pl, plane);
    FirDesign::phase_taps(threadIdx.x, pl, s.smooth, taps + (size_t)plane * pl.fft, nullptr);
}

// LOWESS regressions: one wave per anchor.  grid = (ceil(anchors/16), 2)
__global__ __launch_bounds__(1024) void k_fir_lowess(FirPlanView pl, double* scratch) {
    const int plane = blockIdx.y;
    const FirScratch s = fir_scratch(scratch, pl, plane);
    const int a = blockIdx.x * 16 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (a >= pl.lw.anchors) return;
    const double* p = pl.lw.p + (size_t)a * pl.lw.k;
    const double* y = s.on_log + pl.lw.lo[a];
    double acc = 0.0;
    for (int j = lane; j < pl.lw.k; j += 64) acc = fma(p[j], y[j], acc);
    acc = wave_sum(acc);
    if (lane == 0) s.fit[a] = acc;
}
// skipped points -> spline back onto the linear grid -> pinned bins.  grid = 2
__global__ __launch_bounds__(1024) void k_fir_b(FirPlanView pl, double* scratch) {
    MGX_LDS;
    Affine* sc = reinterpret_cast<Affine*>(mgx_smem);
    const int tid = threadIdx.x, plane = blockIdx.x;
    FirScratch s = fir_scratch(scratch, pl, plane);
    FirDesign::phase_lowess_fill(tid, pl.lw, s.fit, s.log_s);
    __syncthreads();
    fir_solve(pl.s2, s.log_s, s.m2, sc);
    FirDesign::phase_eval(tid, pl.s2, s.log_s, s.m2, s.smooth);
    __syncthreads();
    FirDesign::phase_pin(tid, s);
}
// irfft + ifftshift + Hann (match_frequencies.py:98-99) as a cosine sum in float64.  The spectrum is real
// and even, so h0[m] = (H[0] + (-1)^m H[F/2] + 2 S(m)) / F with S(m) = sum_{k=1}^{F/2-1} H[k] cos(2 pi k m / F),
// and S has two symmetries: S(F - m) = S(m), and with the even-k and odd-k halves E(m), O(m) of the sum,
// S(m) = E + O while S(F/2 - m) = E - O.  One pair (E, O) for m in [0, F/4] therefore gives four taps:
// a quarter of the F^2 / 2 terms of the plain sum (at 16 k taps 100 us of this kernel).
// grid = (ceil((F/4 + 1) / TAP_ROWS), 2); a workgroup takes TAP_ROWS values of m, its TAP_SLICES = 1024 /
// TAP_ROWS groups of lanes each sum a slice of the bins.  cos(2 pi k m / F) for the consecutive k of a
// slice comes from a rotation: start and step are exact table values, the steps in between cost four
// float64 operations each and add ~1e-14 of error over a slice -- no cosine table in LDS (filling 32 KB of
// it per workgroup was most of this kernel's time) and no gather through the L2.
constexpr int TAP_ROWS = 8, TAP_SLICES = 1024 / TAP_ROWS;
__global__ __launch_bounds__(1024) void k_fir_taps(FirPlanView pl, const double* scratch, float* taps /* [2][F] */) {
    MGX_LDS;
    double* sm = reinterpret_cast<double*>(mgx_smem);       // [bins]
    double* red = sm + pl.bins;                             // [2][1024]: even-k and odd-k partial sums
    const int plane = blockIdx.y, f = pl.fft, half = f / 2, quarter = f / 4;
    const FirScratch s = fir_scratch(const_cast<double*>(scratch), pl, plane);
    const int row = threadIdx.x % TAP_ROWS, slice = threadIdx.x / TAP_ROWS;
    const int mm = min(blockIdx.x * TAP_ROWS + row, quarter);       // (rows past F/4 repeat it: same stores)
    // bins 1 .. half-1 in slices of an even number of bins, so that every slice starts on an odd bin
    int per = (half - 1 + TAP_SLICES - 1) / TAP_SLICES;
    per += per & 1;
    const int k0 = 1 + slice * per, k1 = min(half, k0 + per);
    // asked for before the barrier: four table look-ups per thread
    const int i0 = (int)(((long long)k0 * mm) & (f - 1));
    double c = pl.cos_table[i0], sn = pl.cos_table[(i0 - quarter) & (f - 1)];        // sin x = cos(x - pi/2)
    const double dc = pl.cos_table[mm], ds = pl.cos_table[(mm - quarter) & (f - 1)];
    for (int k = threadIdx.x; k < pl.bins; k += 1024) sm[k] = s.smooth[k];
    __syncthreads();
    double odd = 0.0, even = 0.0;
    for (int k = k0; k < k1; k += 2) {                      // k odd, k + 1 even
        odd = fma(sm[k], c, odd);
        double cn = fma(c, dc, -sn * ds);
        sn = fma(sn, dc, c * ds);
        c = cn;
        if (k + 1 < k1) even = fma(sm[k + 1], c, even);
        cn = fma(c, dc, -sn * ds);
        sn = fma(sn, dc, c * ds);
        c = cn;
    }
    red[threadIdx.x] = even;
    red[1024 + threadIdx.x] = odd;
    __syncthreads();
    // TAP_ROWS x 2 sums of TAP_SLICES partials each: one wave per (row, parity)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave < 2 * TAP_ROWS) {
        const int r = wave >> 1, parity = wave & 1;
        double t = 0.0;
        for (int l = lane; l < TAP_SLICES; l += 64) t += red[parity * 1024 + l * TAP_ROWS + r];
        t = wave_sum(t);
        if (lane == 0) red[2048 + wave] = t;
    }
    __syncthreads();
    if (threadIdx.x < 4 * TAP_ROWS) {
        const int r = threadIdx.x >> 2, which = threadIdx.x & 3;
        const int m0 = min(blockIdx.x * TAP_ROWS + r, quarter);
        const double e = red[2048 + 2 * r], o = red[2048 + 2 * r + 1];
        // which: 0 -> m0, 1 -> F - m0 (E + O);  2 -> F/2 - m0, 3 -> F/2 + m0 (E - O)
        const int m = (which == 0 ? m0 : which == 1 ? f - m0 : which == 2 ? half - m0 : half + m0) & (f - 1);
        const double sum = which < 2 ? e + o : e - o;
        const int i = (m + half) & (f - 1);                 // ifftshift: tap i holds h0[(i + F/2) mod F]
        const double v = (sm[0] + ((m & 1) ? -sm[half] : sm[half]) + 2.0 * sum) / f * pl.hann[i];
        taps[(size_t)plane * f + i] = (float)v;
    }
}

// The same taps by a transform, for fft_size >= 8192 (below that the sum above is one 8 us launch and wins).
// numpy.fft.irfft of the real, even spectrum H[0..F/2] as ONE complex inverse DFT of N = F/2 points:
//     Z[k] = (H[k] + H[N-k]) + i w^k (H[k] - H[N-k]),  w = exp(2 pi i / F);   z = IDFT_N(Z) / F;
//     h0[2n] = Re z[n],  h0[2n+1] = Im z[n]
// (the even and odd output samples are the real and imaginary parts of one half-length transform), then
// ifftshift and the Hann window as above.  A workgroup is one CU, and one CU needs 32 us for 8192 points in
// float64 however the passes are arranged (measured: instruction issue, not LDS or its banks), so the transform
// is split by decimation in time over R = 8 workgroups per channel:
//   k_fir_taps_sub<LOG2M>   grid (R, 2): workgroup rho transforms Z[R m + rho], m < M = N/R, in LDS -- Z goes in
//       bit-reversed, then passes that do TWO radix-2 stages in registers (four points per group, a barrier per
//       pass; one plain radix-2 stage first when log2 M is odd); twiddles from a quarter-wave table in LDS
//       (M/4 + 1 exact values of cos_table, the rest by symmetry), so no pass waits on global memory;
//   k_fir_taps_combine      grid (N/256, 2): z[n] = sum_rho w_N^(rho n) A_rho[n mod M] in a fixed order, scale,
//       window, store the two taps of z[n].
// O(F log F) instead of the cosine sum's O(F^2 / 8): 13 us against 47 at 16384 taps; float64 throughout,
// twiddles are table values (cos_table holds cos(2 pi j / F)).  M <= 2048 (32768 taps) is 38 KB of LDS.
// (The bit-reversed store puts a wavefront's 64 consecutive m at a stride of M/64 points: one LDS bank.  A spare
// point after every M/64 turns that stride odd -- TapFft::at -- and costs the later passes nothing.)
constexpr int TAP_SPLIT = 8, TAP_TRANSFORM_FROM = 8192;
__host__ __device__ inline size_t fir_taps_sub_lds_bytes(int m) { return ((size_t)m + 64) * 16 + ((size_t)m / 4 + 1) * 8; }
template <int LOG2M>
struct TapFft {
    static constexpr int M = 1 << LOG2M, PAD_SHIFT = LOG2M >= 8 ? LOG2M - 6 : 30;
    static constexpr int T = M / 4 < 64 ? 64 : (M / 4 > 1024 ? 1024 : M / 4);         // threads: a group of four points each
    static __device__ __forceinline__ int at(int i) { return i + (i >> PAD_SHIFT); }
};
template <int M>
__device__ __forceinline__ double2 quarter_wave_twiddle(const double* q, int t) {      // exp(+2 pi i t / M), 0 <= t < M/2
    const int d = t - M / 4;
    return make_double2(d <= 0 ? q[t] : -q[M / 2 - t], q[d < 0 ? -d : d]);
}
__device__ __forceinline__ void dit_butterfly(double2& x, double2& y, double2 w) {
    const double yr = fma(y.x, w.x, -y.y * w.y), yi = fma(y.x, w.y, y.y * w.x);
    y = make_double2(x.x - yr, x.y - yi);
    x = make_double2(x.x + yr, x.y + yi);
}
template <int LOG2M>
__global__ __launch_bounds__(TapFft<LOG2M>::T) void k_fir_taps_sub(FirPlanView pl, const double* scratch,
                                                                   double2* sub /* [2][R][M] */) {
    MGX_LDS;
    using P = TapFft<LOG2M>;
    constexpr int M = P::M, T = P::T;
    double2* z = reinterpret_cast<double2*>(mgx_smem);       // [M + 64], indexed through P::at
    double* q = reinterpret_cast<double*>(z + M + 64);       // [M/4 + 1]: cos(2 pi j / M)
    const int plane = blockIdx.y, rho = blockIdx.x, r = gridDim.x, n = M * r, f = 2 * n;
    const FirScratch s = fir_scratch(const_cast<double*>(scratch), pl, plane);
    for (int j = threadIdx.x; j <= M / 4; j += T) q[j] = pl.cos_table[2 * r * j];
#pragma unroll
    for (int m0 = 0; m0 < M; m0 += T) {
        const int m = m0 + threadIdx.x;
        if (M >= T || m < M) {
            const int k = r * m + rho;
            const double a = s.smooth[k], b = s.smooth[n - k];
            const double c = pl.cos_table[k], sn = pl.cos_table[(k - f / 4) & (f - 1)];     // w^k = c + i sn
            const double sum = a + b, d = a - b;
            z[P::at((int)(__brev((unsigned)m) >> (32 - LOG2M)))] = make_double2(sum - sn * d, c * d);
        }
    }
    __syncthreads();
    int h = 1;
    if (LOG2M & 1) {
#pragma unroll
        for (int b0 = 0; b0 < M / 2; b0 += T) {
            const int b = b0 + threadIdx.x;
            if (M / 2 >= T || b < M / 2) {
                const int i0 = P::at(2 * b), i1 = P::at(2 * b + 1);
                double2 x = z[i0], y = z[i1];
                dit_butterfly(x, y, make_double2(1.0, 0.0));
                z[i0] = x, z[i1] = y;
            }
        }
        __syncthreads();
        h = 2;
    }
#pragma unroll 1
    for (; h < M; h <<= 2) {
#pragma unroll
        for (int b0 = 0; b0 < M / 4; b0 += T) {
            const int b = b0 + threadIdx.x;
            if (M / 4 >= T || b < M / 4) {
                const int rr = b & (h - 1), j = ((b - rr) << 2) + rr;
                const int ta = rr * (M / 2 / h), tb = ta >> 1;
                const int i0 = P::at(j), i1 = P::at(j + h), i2 = P::at(j + 2 * h), i3 = P::at(j + 3 * h);
                double2 a0 = z[i0], a1 = z[i1], a2 = z[i2], a3 = z[i3];
                const double2 wa = quarter_wave_twiddle<M>(q, ta);
                dit_butterfly(a0, a1, wa);
                dit_butterfly(a2, a3, wa);
                dit_butterfly(a0, a2, quarter_wave_twiddle<M>(q, tb));
                dit_butterfly(a1, a3, quarter_wave_twiddle<M>(q, tb + M / 4));
                z[i0] = a0, z[i1] = a1, z[i2] = a2, z[i3] = a3;
            }
        }
        __syncthreads();
    }
    double2* out = sub + ((size_t)plane * r + rho) * M;
#pragma unroll
    for (int i0 = 0; i0 < M; i0 += T) {
        const int i = i0 + threadIdx.x;
        if (M >= T || i < M) out[i] = z[P::at(i)];
    }
}
__global__ __launch_bounds__(256) void k_fir_taps_combine(FirPlanView pl, const double2* sub /* [2][R][M] */, int r,
                                                          float* taps /* [2][F] */) {
    const int plane = blockIdx.y, f = pl.fft, n_all = f / 2, m_len = n_all / r;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= n_all) return;
    const double2* a = sub + (size_t)plane * n_all + (n & (m_len - 1));
    double zr = 0.0, zi = 0.0;
    for (int rho = 0; rho < r; ++rho) {
        const int e = (2 * rho * n) & (f - 1);                // w_N^(rho n) = exp(2 pi i (2 rho n) / F)
        const double c = pl.cos_table[e], sn = pl.cos_table[(e - f / 4) & (f - 1)];
        const double2 v = a[(size_t)rho * m_len];
        zr += fma(v.x, c, -v.y * sn);
        zi += fma(v.x, sn, v.y * c);
    }
    const double inv = 1.0 / (double)f;
    const int i = (2 * n + n_all) & (f - 1);                  // ifftshift: tap i holds h0[(i + F/2) mod F]; i is even
    float2 t;
    t.x = (float)(zr * inv * pl.hann[i]);
    t.y = (float)(zi * inv * pl.hann[i + 1]);
    *reinterpret_cast<float2*>(taps + (size_t)plane * f + i) = t;
}

}  // namespace mgx
