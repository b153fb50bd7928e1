// Matching EQ controls on the device (include/mgx.h, mgx_eq_shape): the shape stage on the smooth curve and the
// minimum-phase form of the designed taps.  Both sit between existing kernels of the FIR design (run_fir.h): the shape
// stage in place on the two smooth planes before the tap synthesis, the minimum-phase chain in place on the [2][F]
// float32 taps behind it.
//
// Minimum phase by the folded cepstrum, float64, on N = 4F points per channel:
//     H = |DFT(lin)|   L = ln(max(H, 1e-9 max H))   c = Re IDFT(L)   fold c   g = Re IDFT(exp(DFT(c)))   taper, store
// i.e. four transforms with the pointwise steps at their ends.  A transform of N points is split by decimation in time
// over R workgroups per channel, as the tap synthesis is (fir_kernels.h, k_fir_taps_sub / k_fir_taps_combine):
//   k_minphase_sub      grid (R, 2): workgroup rho transforms x[R m + rho], m < M = N / R, in LDS -- the step's pointwise
//       INPUT map applied at the load (step 0: the float32 taps, zero padded; step 1: the logarithm, clamped at the
//       floor that the maximum of step 0 sets), bit-reversed store, passes of two radix-2 stages each;
//   k_minphase_combine  grid (N / 256, 2): X[n] = sum_rho w_N^(+-rho n) A_rho[n mod M] in a fixed order, then the step's
//       pointwise OUTPUT map (magnitude and its maximum; fold; complex exponential; taper and the float32 store).
// M = min(N, 4096): 64 KB of points and 32 KB of twiddles in LDS, one workgroup of 1024 threads, 12 stages.  (One CU needs
// ~32 us for 8192 float64 points -- the tap synthesis's finding -- so a channel is never left to ONE workgroup beyond
// 4096 points even where 8192 would fit its LDS.)  F <= 1024 is therefore one workgroup per channel and transform (R = 1,
// the combine is the pointwise map alone), F = 2048 the first size that is split; 16384 taps run R = 16.
// No workgroup waits for another: eight launches hand over through the call's own scratch (CallContext::eq_work).
// The maximum of H crosses from the first combine to the second sub-transform as the bit pattern of a non-negative
// double under an integer atomic maximum: order-free, so two runs give the same bits.
// Twiddles are table values, exp(2 pi i j / N) for j < N, made once per (device, N) on the host (run_fir.h).
//
// The per-thread phase functions compile under a plain host compiler with -DMGX_HOST_EMU (tests/emu/emu_eq_shape.cpp).
#pragma once

#include "mgx_hd.h"

namespace mgx {

// ---- the shape stage ------------------------------------------------------------------------------------------------
struct EqShapeArgs {
    double amount;
    double max_boost_db, max_cut_db;         // NaN: no cap
    double min_value;                        // Config.min_value: the floor under the curve before the logarithm
};
// bin k of one smooth plane, in place; bin 0 stays 0 (match_frequencies.py:72)
MGX_HD void eq_shape_phase(int k, double* smooth, const EqShapeArgs& a) {
    if (k == 0) {
        smooth[0] = 0.0;
        return;
    }
    double d = a.amount * (20.0 * log10(fmax(smooth[k], a.min_value)));
    if (a.max_boost_db == a.max_boost_db) d = fmin(d, a.max_boost_db);
    if (a.max_cut_db == a.max_cut_db) d = fmax(d, -a.max_cut_db);
    smooth[k] = pow(10.0, d / 20.0);
}

// ---- minimum phase --------------------------------------------------------------------------------------------------
// (F from 64 to 16384: mgx_policy.h, EQ_MINPHASE_FFT_MIN / _MAX, is what mgx_eq_shape_check lets through)
constexpr int MINPHASE_OVERSAMPLE = 4;                            // N = 4F
constexpr int MINPHASE_SUB_LOG2_MAX = 12;                            // M <= 4096 points per workgroup
constexpr double MINPHASE_FLOOR = 1e-9;                              // of the largest magnitude

struct MinPhaseArgs {
    int fft;                     // F
    int n;                       // N = 4F
    int log2m, r;                // M = 1 << log2m points per sub-transform, R = N / M of them per channel
    const double2* tw;           // [N] exp(+2 pi i j / N)
    float* taps;                 // [2][F]: the linear-phase taps in, the minimum-phase taps out
    double2* a;                  // [2][R][M] sub-transforms
    double2* b;                  // [2][N] the chain's values between two transforms
    unsigned long long* hmax;    // [2] bits of max H (non-negative doubles order as their bit patterns)
};
MGX_HD void minphase_geometry(int fft, int& log2m, int& r) {
    const int log2n = ilog2(fft * MINPHASE_OVERSAMPLE);
    log2m = log2n < MINPHASE_SUB_LOG2_MAX ? log2n : MINPHASE_SUB_LOG2_MAX;
    r = 1 << (log2n - log2m);
}
// threads of a sub-transform's workgroup: a group of four points each
MGX_HD int minphase_threads(int log2m) {
    const int t = (1 << log2m) / 4;
    return t < 64 ? 64 : (t > 1024 ? 1024 : t);
}
// LDS of a sub-transform: z[M + 64] through minphase_at, q[M / 2] twiddles of the M-point transform
MGX_HD size_t minphase_lds_bytes(int log2m) { return (((size_t)1 << log2m) + 64 + ((size_t)1 << log2m) / 2) * 16; }
// scratch of a call, in bytes: a, b and the two maxima
MGX_HD size_t minphase_work_bytes(int fft) { return (size_t)4 * fft * MINPHASE_OVERSAMPLE * 16 + 16; }
// (the bit-reversed store puts a wavefront's 64 consecutive m at a stride of M / 64 points -- one LDS bank; a spare point
// after every M / 64 turns the stride odd, as TapFft::at does)
MGX_HD int minphase_at(int i, int log2m) { return log2m >= 8 ? i + (i >> (log2m - 6)) : i; }
MGX_HD double2 mp_c(double x, double y) {
    double2 v;
    v.x = x;
    v.y = y;
    return v;
}
MGX_HD void mp_butterfly(double2& x, double2& y, double2 w) {
    const double yr = fma(y.x, w.x, -y.y * w.y), yi = fma(y.x, w.y, y.y * w.x);
    y = mp_c(x.x - yr, x.y - yi);
    x = mp_c(x.x + yr, x.y + yi);
}
MGX_HD int mp_bitrev(int m, int bits) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(MGX_HOST_EMU)
    return (int)(__brev((unsigned)m) >> (32 - bits));
#else
    return bitrev(m, bits);
#endif
}
// steps 0 and 2 are forward transforms (exp(-i ...)), 1 and 3 inverse ones
MGX_HD double minphase_sign(int step) { return (step & 1) ? 1.0 : -1.0; }

// load: the twiddles of this transform's direction, and point m of workgroup rho = the step's input at R m + rho
MGX_HD void minphase_sub_load(int tid, int threads, int plane, int rho, int step, const MinPhaseArgs& a, double2* z,
                              double2* q) {
    const int M = 1 << a.log2m;
    const double sign = minphase_sign(step);
    for (int t = tid; t < M / 2; t += threads) {
        const double2 w = a.tw[(size_t)t * a.r];
        q[t] = mp_c(w.x, sign * w.y);
    }
    double floor_h = 0.0;
    if (step == 1) {
        union {
            unsigned long long u;
            double d;
        } bits;
        bits.u = a.hmax[plane];
        floor_h = MINPHASE_FLOOR * bits.d;
    }
    for (int m = tid; m < M; m += threads) {
        const int k = a.r * m + rho;
        double2 v;
        if (step == 0)
            v = mp_c(k < a.fft ? (double)a.taps[(size_t)plane * a.fft + k] : 0.0, 0.0);
        else if (step == 1)
            v = mp_c(log(fmax(a.b[(size_t)plane * a.n + k].x, floor_h)), 0.0);
        else
            v = a.b[(size_t)plane * a.n + k];
        z[minphase_at(mp_bitrev(m, a.log2m), a.log2m)] = v;
    }
}
// log2 M odd: one plain radix-2 stage first
MGX_HD void minphase_sub_first(int tid, int threads, int log2m, double2* z) {
    const int M = 1 << log2m;
    for (int b = tid; b < M / 2; b += threads) {
        const int i0 = minphase_at(2 * b, log2m), i1 = minphase_at(2 * b + 1, log2m);
        double2 x = z[i0], y = z[i1];
        mp_butterfly(x, y, mp_c(1.0, 0.0));
        z[i0] = x;
        z[i1] = y;
    }
}
// two radix-2 stages, of half-lengths h and 2h, on groups of four points
MGX_HD void minphase_sub_pass(int tid, int threads, int log2m, int h, double2* z, const double2* q) {
    const int M = 1 << log2m;
    for (int b = tid; b < M / 4; b += threads) {
        const int rr = b & (h - 1), j = ((b - rr) << 2) + rr;
        const int ta = rr * (M / 2 / h), tb = ta >> 1;
        const int i0 = minphase_at(j, log2m), i1 = minphase_at(j + h, log2m), i2 = minphase_at(j + 2 * h, log2m),
                  i3 = minphase_at(j + 3 * h, log2m);
        double2 a0 = z[i0], a1 = z[i1], a2 = z[i2], a3 = z[i3];
        const double2 wa = q[ta];
        mp_butterfly(a0, a1, wa);
        mp_butterfly(a2, a3, wa);
        mp_butterfly(a0, a2, q[tb]);
        mp_butterfly(a1, a3, q[tb + M / 4]);
        z[i0] = a0;
        z[i1] = a1;
        z[i2] = a2;
        z[i3] = a3;
    }
}
MGX_HD void minphase_sub_store(int tid, int threads, int plane, int rho, const MinPhaseArgs& a, const double2* z) {
    const int M = 1 << a.log2m;
    double2* out = a.a + ((size_t)plane * a.r + rho) * M;
    for (int i = tid; i < M; i += threads) out[i] = z[minphase_at(i, a.log2m)];
}
// outputs of a combine launch per channel: every point but for the last step, which keeps the first F / 2
MGX_HD int minphase_combine_count(const MinPhaseArgs& a, int step) { return step == 3 ? a.fft / 2 : a.n; }
// output n of the step's transform and its pointwise map.  Returns the magnitude it stored (step 0; 0 otherwise), for the
// caller's maximum.
MGX_HD double minphase_combine(int n, int plane, int step, const MinPhaseArgs& a) {
    const int M = 1 << a.log2m, N = a.n, half = N / 2;
    double2* b = a.b + (size_t)plane * N;
    if (step == 1 && n > half) {                                    // the folded cepstrum's upper half
        b[n] = mp_c(0.0, 0.0);
        return 0.0;
    }
    const double sign = minphase_sign(step);
    const double2* sub = a.a + (size_t)plane * N + (n & (M - 1));
    double xr = 0.0, xi = 0.0;
    for (int rho = 0; rho < a.r; ++rho) {
        const double2 w = a.tw[(int)(((long long)rho * n) & (N - 1))];
        const double c = w.x, s = sign * w.y;
        const double2 v = sub[(size_t)rho * M];
        xr += fma(v.x, c, -v.y * s);
        xi += fma(v.x, s, v.y * c);
    }
    const double inv = 1.0 / (double)N;
    if (step == 0) {
        const double h = sqrt(fma(xr, xr, xi * xi));
        b[n] = mp_c(h, 0.0);
        return h;
    }
    if (step == 1) {
        const double c = xr * inv;
        b[n] = mp_c(n == 0 || n == half ? c : 2.0 * c, 0.0);
        return 0.0;
    }
    if (step == 2) {
        const double e = exp(xr);
        b[n] = mp_c(e * cos(xi), e * sin(xi));
        return 0.0;
    }
    // step 3: g[n] tapered over the second quarter of F, behind F / 2 zeros
    const int quarter = a.fft / 4;
    const double taper = n < quarter ? 1.0 : 0.5 * (1.0 + a.tw[(size_t)8 * (n - quarter)].x);   // cos(pi (n - F/4) / (F/4))
    float* taps = a.taps + (size_t)plane * a.fft;
    taps[n] = 0.f;
    taps[a.fft / 2 + n] = (float)((xr * inv) * taper);
    return 0.0;
}

}  // namespace mgx

#if defined(__HIPCC__) && !defined(MGX_HOST_EMU)
#include "fir_kernels.h"
#include "wave_util.h"

namespace mgx {

// the shape stage, in place on the two smooth planes; grid (ceil(bins / 256), 2)
__global__ __launch_bounds__(256) void k_eq_shape(FirPlanView pl, double* scratch, EqShapeArgs a) {
    const int k = blockIdx.x * 256 + threadIdx.x, plane = blockIdx.y;
    if (k >= pl.bins) return;
    eq_shape_phase(k, fir_scratch(scratch, pl, plane).smooth, a);
}

// grid (R, 2), minphase_threads(log2m) threads, minphase_lds_bytes(log2m) of LDS
__global__ __launch_bounds__(1024) void k_minphase_sub(MinPhaseArgs a, int step) {
    MGX_LDS;
    const int M = 1 << a.log2m, tid = threadIdx.x, threads = blockDim.x, rho = blockIdx.x, plane = blockIdx.y;
    double2* z = reinterpret_cast<double2*>(mgx_smem);       // [M + 64], indexed through minphase_at
    double2* q = z + M + 64;                                 // [M / 2]
    if (step == 0 && rho == 0 && tid == 0) a.hmax[plane] = 0ull;      // (the combine behind this launch raises it)
    minphase_sub_load(tid, threads, plane, rho, step, a, z, q);
    __syncthreads();
    int h = 1;
    if (a.log2m & 1) {
        minphase_sub_first(tid, threads, a.log2m, z);
        __syncthreads();
        h = 2;
    }
#pragma unroll 1
    for (; h < M; h <<= 2) {
        minphase_sub_pass(tid, threads, a.log2m, h, z, q);
        __syncthreads();
    }
    minphase_sub_store(tid, threads, plane, rho, a, z);
}

// grid (ceil(minphase_combine_count / 256), 2)
__global__ __launch_bounds__(256) void k_minphase_combine(MinPhaseArgs a, int step) {
    const int n = blockIdx.x * 256 + threadIdx.x, plane = blockIdx.y;
    double h = 0.0;
    if (n < minphase_combine_count(a, step)) h = minphase_combine(n, plane, step, a);
    if (step == 0) {
        h = wave_max_f64(h);
        if ((threadIdx.x & 63) == 0) atomicMax(&a.hmax[plane], (unsigned long long)__double_as_longlong(h));
    }
}

}  // namespace mgx
#endif
