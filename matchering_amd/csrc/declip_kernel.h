// Clip repair (include/mgx.h, mgx_declip): one streaming pass over float32 frames in HBM that rebuilds short runs at
// the rail by a cubic Hermite segment through the samples around them, then one workgroup that folds the segments'
// counters.  Two launches; no workgroup waits for another, no atomics, every value defined bit for bit.
//
// k_declip: one workgroup per segment of DECLIP_SEGMENT frames, with a halo of DECLIP_HALO = DECLIP_MAX_RUN + 2 frames on
//   either side (the window: 5124 frames, 40992 bytes of LDS).  A run of at most max_run samples that holds a sample of
//   the segment lies inside the window together with its four anchors; a run that reaches an outer edge of a halo (not
//   an end of the track) is longer than DECLIP_MAX_RUN and so `long`.
//   stage   the window's bytes -> LDS as they lie in memory, 16 bytes per load and thread, consecutive threads on
//           consecutive addresses (the window starts on an even frame); an odd last frame by one 8-byte load.  Every
//           thread looks at what it loaded: a window without a sample at the rail is copied out the same way and done.
//   scan    thread t takes the DECLIP_STRETCH consecutive frames [t S, (t + 1) S) of the window and walks them once:
//           the last frame of its stretch at which a run begins (or that is not at the rail), and the first behind which
//           one ends.  An exclusive prefix maximum of the former over the threads (lanes by shuffles, waves through LDS)
//           is where the run that enters a stretch from the left began; an exclusive suffix minimum of the latter where
//           the run that leaves it to the right ends.  Nobody walks further than its own stretch, so a track that sits
//           at the rail throughout costs what any other does.
//   walk    each thread whose stretch meets the segment walks it again: a run's extent is settled where the walk enters
//           it (inside the stretch by looking ahead to the stretch's end, beyond it from the two scans), the run is
//           classed and, where it is repaired, its anchors are read ONCE from the LDS -- which holds the original values
//           to the end, so runs are independent of each other.  Samples of the segment are evaluated and stored, two
//           frames per 16-byte store.  A run is counted by the thread that holds its first sample, if that lies in the
//           segment; samples_raised and the peaks are per sample.
//   fold    the threads' counters by shuffles and LDS into the segment's record: sums, maxima (a peak as the bits of a
//           non-negative float32, whose order is the integers') and a minimum, all exact, so any order gives the same.
// k_declip_fold: one workgroup; thread t folds the segments t, t + T, ... and the threads are folded as above.
//
// The phase functions are MGX_HD and take the window's geometry as numbers, so that tests/emu/emu_declip.cpp runs them
// segment by segment on the host, with a small segment and halo where the test wants borders to be cheap.
#pragma once

#include "mgx_hd.h"

namespace mgx {

constexpr int DECLIP_SEGMENT = 4096;            // frames of a workgroup
constexpr int DECLIP_MAX_RUN = 512;             // the longest run mgx_declip_check lets max_run ask for
constexpr int DECLIP_HALO = DECLIP_MAX_RUN + 2; // the run's own samples but one, and two anchors
constexpr int DECLIP_WINDOW = DECLIP_SEGMENT + 2 * DECLIP_HALO;
constexpr int DECLIP_THREADS = 256;
constexpr int DECLIP_STRETCH = 22;              // consecutive frames of a thread: even (a 16-byte store is two frames)
constexpr int DECLIP_FOLD_THREADS = 256;
static_assert(DECLIP_STRETCH % 2 == 0 && DECLIP_HALO % 2 == 0, "stretches and the segment begin on even frames of the window");
static_assert(DECLIP_THREADS * DECLIP_STRETCH >= DECLIP_WINDOW, "the threads' stretches cover the window");

// a channel's counters, of a thread, a segment or the track: slot k of channel c is word c * DECLIP_SLOTS + k
enum {
    DECLIP_RUNS_REPAIRED = 0, DECLIP_SAMPLES_REPAIRED, DECLIP_SAMPLES_RAISED, DECLIP_RUNS_SHORT, DECLIP_RUNS_LONG,
    DECLIP_RUNS_EDGE,           // ... sums
    DECLIP_LONGEST, DECLIP_PEAK_BEFORE, DECLIP_PEAK_AFTER,      // maxima; a peak is the bits of a float32 >= 0
    DECLIP_FIRST,               // minimum as unsigned: the frame, 0xffffffff where there is none
    DECLIP_SLOTS
};
constexpr int DECLIP_SUM_SLOTS = DECLIP_LONGEST, DECLIP_MAX_SLOTS = DECLIP_FIRST;
constexpr int DECLIP_NO_END = 0x7fffffff;

// how slot k folds; T is int for a thread or a segment, long long for the track
template <typename T>
MGX_HD T declip_fold_slot(int k, T a, T b) {
    if (k < DECLIP_SUM_SLOTS) return a + b;
    if (k < DECLIP_MAX_SLOTS) return a > b ? a : b;
    return (unsigned)a < (unsigned)b ? a : b;
}
MGX_HD int declip_slot_identity(int k) { return k == DECLIP_FIRST ? -1 : 0; }

struct DeclipParams {
    double level, cap;          // lambda, and kappa lambda rounded once
    int min_run, max_run;
};

struct DeclipArgs {
    const float* x;             // [n][2]
    float* out;                 // [n][2]
    long long n;
    long long segments;
    DeclipParams p;
    int* seg;                   // [segments][2][DECLIP_SLOTS]
    long long* totals;          // [2][DECLIP_SLOTS]
};

// ---- what the host decides (everything of the arguments but the pointers) ----------------------------------------------
inline long long declip_segments(long long n) { return (n + DECLIP_SEGMENT - 1) / DECLIP_SEGMENT; }
inline void declip_launch(DeclipArgs& a, long long n, double level, double max_rise, int min_run, int max_run) {
    a.n = n, a.segments = declip_segments(n);
    a.p.level = level, a.p.cap = max_rise * level, a.p.min_run = min_run, a.p.max_run = max_run;
}
inline size_t declip_seg_bytes(const DeclipArgs& a) { return (size_t)a.segments * 2 * DECLIP_SLOTS * sizeof(int); }
constexpr size_t DECLIP_TOTALS_BYTES = 2 * DECLIP_SLOTS * sizeof(long long);

// ---- the phase functions -----------------------------------------------------------------------------------------------
MGX_HD unsigned declip_bits(float f) {
    unsigned u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
MGX_HD bool declip_finite(float f) { return fabsf(f) <= 3.4028235e38f; }
// +1: high, -1: low, 0: neither (a NaN or an infinity is neither)
MGX_HD int declip_class(float f, double level) {
    if (!declip_finite(f)) return 0;
    const double xd = (double)f;
    return xd >= level ? 1 : xd <= -level ? -1 : 0;
}

// The window of one segment: frames [lo, lo + wn) of the track, the segment being [core0, core1) of it.
struct DeclipWindow {
    const float* w;             // [wn][2], the original samples
    int wn;
    int core0, core1;
    long long lo, n;
};
MGX_HD DeclipWindow declip_window(const float* w, long long segment, long long n, int segment_frames, int halo) {
    DeclipWindow W;
    const long long g0 = segment * segment_frames;
    const long long end = g0 + segment_frames < n ? g0 + segment_frames : n;
    const long long hi = end + halo < n ? end + halo : n;
    W.w = w, W.n = n;
    W.lo = g0 >= halo ? g0 - halo : 0;
    W.wn = (int)(hi - W.lo);
    W.core0 = (int)(g0 - W.lo), W.core1 = (int)(end - W.lo);
    return W;
}

// scan: over frames [s0, s1) of channel ch, the last frame at which a run begins or that is not at the rail (-1: none)
// and the first frame BEHIND which a run ends or that is not at the rail, plus one (DECLIP_NO_END: none)
MGX_HD void declip_scan(const DeclipWindow& W, double level, int s0, int s1, int ch, int& last_begin, int& first_end) {
    last_begin = -1, first_end = DECLIP_NO_END;
    if (s0 >= s1) return;
    int before = s0 > 0 ? declip_class(W.w[2 * (s0 - 1) + ch], level) : 0;
    int here = declip_class(W.w[2 * s0 + ch], level);
    for (int f = s0; f < s1; ++f) {
        const int behind = f + 1 < W.wn ? declip_class(W.w[2 * (f + 1) + ch], level) : 0;
        if (here == 0 || here != before) last_begin = f;
        if ((here == 0 || here != behind) && first_end == DECLIP_NO_END) first_end = f + 1;
        before = here, here = behind;
    }
}

// walk: what a thread knows of the run it is inside, per channel
struct DeclipRun {
    int end;                    // the first frame of the stretch the run's piece does not hold; the walk is inside while f < end
    int sign, a;                // +1 / -1; the run's first frame in the window
    bool repaired;
    double h, p0, p1, m0, m1;
};
MGX_HD void declip_run_start(DeclipRun& st, int s0) { st.end = s0, st.sign = 0, st.a = 0, st.repaired = false; }

// One sample of the walk, frames in ascending order from s0: what the output holds at frame f of channel ch.  begin_in:
// the prefix maximum of the threads before this one, end_in: the suffix minimum of those behind it.  cnt: the thread's
// DECLIP_SLOTS counters of the channel.
MGX_HD float declip_step(const DeclipWindow& W, const DeclipParams& P, int s0, int s1, int begin_in, int end_in, int ch,
                         int f, DeclipRun& st, int* cnt) {
    const float x = W.w[2 * f + ch];
    const bool core = f >= W.core0 && f < W.core1;
    if (f >= st.end) {
        st.repaired = false;
        st.end = f + 1;
        const int c = declip_class(x, P.level);
        if (c != 0) {
            int e = f + 1;
            while (e < s1 && declip_class(W.w[2 * e + ch], P.level) == c) ++e;
            // (a piece that begins behind s0 begins its run: the sample before it is not of its class)
            const bool begins = f > s0 || f == 0 || declip_class(W.w[2 * (f - 1) + ch], P.level) != c;
            const bool ends = e < s1 || e == W.wn || declip_class(W.w[2 * e + ch], P.level) != c;
            const int a = begins ? f : begin_in, b = ends ? e : end_in;
            const int r = b - a;
            // an outer edge of a halo that is not an end of the track: the run goes on beyond it
            const bool open = (a == 0 && W.lo > 0) || (b == W.wn && W.lo + W.wn < W.n);
            int kind = DECLIP_RUNS_REPAIRED;
            if (!open && r < P.min_run) kind = DECLIP_RUNS_SHORT;
            else if (open || r > P.max_run) kind = DECLIP_RUNS_LONG;
            else if (a < 2 || b + 1 > W.wn - 1) kind = DECLIP_RUNS_EDGE;
            else {
                const float q0 = W.w[2 * (a - 2) + ch], q1 = W.w[2 * (a - 1) + ch], q2 = W.w[2 * b + ch], q3 = W.w[2 * (b + 1) + ch];
                if (!(declip_finite(q0) && declip_finite(q1) && declip_finite(q2) && declip_finite(q3))) kind = DECLIP_RUNS_EDGE;
                else {
                    st.repaired = true, st.sign = c, st.a = a;
                    st.h = (double)(r + 1);
                    st.p0 = (double)q1, st.p1 = (double)q2;
                    st.m0 = st.h * (st.p0 - (double)q0);
                    st.m1 = st.h * ((double)q3 - st.p1);
                }
            }
            if (begins && core) {
                cnt[DECLIP_RUNS_REPAIRED] += kind == DECLIP_RUNS_REPAIRED;      // (no counter is indexed by a variable)
                cnt[DECLIP_RUNS_SHORT] += kind == DECLIP_RUNS_SHORT;
                cnt[DECLIP_RUNS_LONG] += kind == DECLIP_RUNS_LONG;
                cnt[DECLIP_RUNS_EDGE] += kind == DECLIP_RUNS_EDGE;
                if (kind == DECLIP_RUNS_REPAIRED) {
                    cnt[DECLIP_SAMPLES_REPAIRED] += r;
                    if (r > cnt[DECLIP_LONGEST]) cnt[DECLIP_LONGEST] = r;
                    const unsigned at = (unsigned)(W.lo + a);
                    if (at < (unsigned)cnt[DECLIP_FIRST]) cnt[DECLIP_FIRST] = (int)at;
                }
            }
            st.end = e;
        }
    }
    if (!core) return x;
    float out = x;
    if (st.repaired) {
        const double xd = (double)x;
        const double t = (double)(f - st.a + 1) / st.h, t2 = t * t, t3 = t2 * t;
        double y = (((2.0 * t3 - 3.0 * t2) + 1.0) * st.p0 + ((t3 - 2.0 * t2) + t) * st.m0) +
                   ((3.0 * t2 - 2.0 * t3) * st.p1 + (t3 - t2) * st.m1);
        if (st.sign > 0) {
            if (y > P.cap) y = P.cap;
            if (y > xd) out = (float)y;
        } else {
            if (y < -P.cap) y = -P.cap;
            if (y < xd) out = (float)y;
        }
    }
    const unsigned xb = declip_bits(x), ob = declip_bits(out);
    cnt[DECLIP_SAMPLES_RAISED] += xb != ob;
    const int xa = (int)(xb & 0x7fffffffu), oa = (int)(ob & 0x7fffffffu);       // |.| as bits; finite: below the infinity's
    if (xa < 0x7f800000 && xa > cnt[DECLIP_PEAK_BEFORE]) cnt[DECLIP_PEAK_BEFORE] = xa;
    if (oa < 0x7f800000 && oa > cnt[DECLIP_PEAK_AFTER]) cnt[DECLIP_PEAK_AFTER] = oa;
    return out;
}

// a sample that is copied: only the peaks see it
MGX_HD void declip_copied(float x, int* cnt) {
    const int xa = (int)(declip_bits(x) & 0x7fffffffu);
    if (xa < 0x7f800000 && xa > cnt[DECLIP_PEAK_BEFORE]) cnt[DECLIP_PEAK_BEFORE] = xa;
}

}  // namespace mgx

#if defined(__HIPCC__) && !defined(MGX_HOST_EMU)

namespace mgx {

// The threads' words folded by slot k's rule; `waves`: THREADS / 64 ints of LDS per call that nobody else touches.  The
// result on every thread of wave 0 after the caller's barrier: see the kernels.
__device__ __forceinline__ int declip_wave_fold(int k, int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = declip_fold_slot<int>(k, v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ long long declip_wave_fold(int k, long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = declip_fold_slot<long long>(k, v, __shfl_xor(v, o, 64));
    return v;
}

// (templates only so that their code is emitted with the other templates' instantiations, behind the kernels of the
//  master call: see k_audit_merge)
template <int UNUSED>
__global__ __launch_bounds__(DECLIP_THREADS) void k_declip(DeclipArgs a) {
    constexpr int NW = DECLIP_THREADS / 64;
    constexpr int STAGE_TRIPS = (DECLIP_WINDOW / 2 + DECLIP_THREADS - 1) / DECLIP_THREADS;
    __shared__ __attribute__((aligned(16))) float win[DECLIP_WINDOW * 2];
    __shared__ int wave_scan[4][NW];                            // [begin L, begin R, end L, end R]
    __shared__ int wave_cnt[NW][2 * DECLIP_SLOTS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const DeclipWindow W = declip_window(win, blockIdx.x, a.n, DECLIP_SEGMENT, DECLIP_HALO);
    const DeclipParams P = a.p;
    int cnt[2][DECLIP_SLOTS];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int k = 0; k < DECLIP_SLOTS; ++k) cnt[c][k] = declip_slot_identity(k);

    // ---- stage ----  (W.lo is even: the window's first byte is 16-byte aligned where x is)
    const float* base = a.x + W.lo * 2;
    const int pairs = W.wn >> 1;
    int rail = 0;
#pragma unroll
    for (int k = 0; k < STAGE_TRIPS; ++k) {
        const int q = tid + k * DECLIP_THREADS;
        if (q < pairs) {
            const float4 v = reinterpret_cast<const float4*>(base)[q];
            reinterpret_cast<float4*>(win)[q] = v;
            rail |= declip_class(v.x, P.level) | declip_class(v.y, P.level) | declip_class(v.z, P.level) | declip_class(v.w, P.level);
        }
    }
    if (tid == 0 && (W.wn & 1)) {                               // the track's last frame
        const float2 v = reinterpret_cast<const float2*>(base)[W.wn - 1];
        reinterpret_cast<float2*>(win)[W.wn - 1] = v;
        rail |= declip_class(v.x, P.level) | declip_class(v.y, P.level);
    }
    const int any = __syncthreads_or(rail);

    float* out = a.out + W.lo * 2;
    if (!any) {
        // ---- a copy: the segment's frames as they were staged ----
        const int first = W.core0 >> 1, cpairs = (W.core1 - W.core0) >> 1;
        for (int q = tid; q < cpairs; q += DECLIP_THREADS) {
            const float4 v = reinterpret_cast<const float4*>(win)[first + q];
            reinterpret_cast<float4*>(out)[first + q] = v;
            declip_copied(v.x, cnt[0]), declip_copied(v.y, cnt[1]), declip_copied(v.z, cnt[0]), declip_copied(v.w, cnt[1]);
        }
        if (tid == 0 && ((W.core1 - W.core0) & 1)) {
            const float2 v = reinterpret_cast<const float2*>(win)[W.core1 - 1];
            reinterpret_cast<float2*>(out)[W.core1 - 1] = v;
            declip_copied(v.x, cnt[0]), declip_copied(v.y, cnt[1]);
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) cnt[c][DECLIP_PEAK_AFTER] = cnt[c][DECLIP_PEAK_BEFORE];
    } else {
        // ---- scan ----
        const int s0 = tid * DECLIP_STRETCH < W.wn ? tid * DECLIP_STRETCH : W.wn;
        const int s1 = s0 + DECLIP_STRETCH < W.wn ? s0 + DECLIP_STRETCH : W.wn;
        int v[4];                                               // inclusive over the lanes: [begin L, begin R, end L, end R]
        declip_scan(W, P.level, s0, s1, 0, v[0], v[2]);
        declip_scan(W, P.level, s0, s1, 1, v[1], v[3]);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int up = __shfl_up(v[c], o, 64), down = __shfl_down(v[2 + c], o, 64);
                if (lane >= o && up > v[c]) v[c] = up;
                if (lane + o < 64 && down < v[2 + c]) v[2 + c] = down;
            }
        }
        if (lane == 63) wave_scan[0][wave] = v[0], wave_scan[1][wave] = v[1];
        if (lane == 0) wave_scan[2][wave] = v[2], wave_scan[3][wave] = v[3];
        int in[4];                                              // exclusive
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            in[c] = __shfl_up(v[c], 1, 64), in[2 + c] = __shfl_down(v[2 + c], 1, 64);
            if (lane == 0) in[c] = -1;
            if (lane == 63) in[2 + c] = DECLIP_NO_END;
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NW; ++w) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (w < wave && wave_scan[c][w] > in[c]) in[c] = wave_scan[c][w];
                if (w > wave && wave_scan[2 + c][w] < in[2 + c]) in[2 + c] = wave_scan[2 + c][w];
            }
        }

        // ---- walk ----
        if (s0 < W.core1 && s1 > W.core0) {
            DeclipRun left, right;
            declip_run_start(left, s0), declip_run_start(right, s0);
            float keep_l = 0.f, keep_r = 0.f;
            for (int f = s0; f < s1; ++f) {
                const float yl = declip_step(W, P, s0, s1, in[0], in[2], 0, f, left, cnt[0]);
                const float yr = declip_step(W, P, s0, s1, in[1], in[3], 1, f, right, cnt[1]);
                if (f < W.core0 || f >= W.core1) continue;
                if (!(f & 1)) {
                    keep_l = yl, keep_r = yr;
                    if (f + 1 == W.core1) reinterpret_cast<float2*>(out)[f] = make_float2(yl, yr);    // the track's odd last frame
                } else {
                    reinterpret_cast<float4*>(out)[f >> 1] = make_float4(keep_l, keep_r, yl, yr);
                }
            }
        }
    }

    // ---- fold ----
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int k = 0; k < DECLIP_SLOTS; ++k) {
            const int s = declip_wave_fold(k, cnt[c][k]);
            if (lane == 0) wave_cnt[wave][c * DECLIP_SLOTS + k] = s;
        }
    __syncthreads();
    if (tid < 2 * DECLIP_SLOTS) {
        const int k = tid % DECLIP_SLOTS;
        int s = wave_cnt[0][tid];
#pragma unroll
        for (int w = 1; w < NW; ++w) s = declip_fold_slot<int>(k, s, wave_cnt[w][tid]);
        a.seg[(size_t)blockIdx.x * 2 * DECLIP_SLOTS + tid] = s;
    }
}

template <int UNUSED>
__global__ __launch_bounds__(DECLIP_FOLD_THREADS) void k_declip_fold(DeclipArgs a) {
    constexpr int T = DECLIP_FOLD_THREADS, NW = T / 64;
    __shared__ long long wave_cnt[NW][2 * DECLIP_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long cnt[2 * DECLIP_SLOTS];
#pragma unroll
    for (int j = 0; j < 2 * DECLIP_SLOTS; ++j) cnt[j] = declip_slot_identity(j % DECLIP_SLOTS);
    for (long long s = tid; s < a.segments; s += T) {
        const int* g = a.seg + (size_t)s * 2 * DECLIP_SLOTS;
#pragma unroll
        for (int j = 0; j < 2 * DECLIP_SLOTS; ++j) cnt[j] = declip_fold_slot<long long>(j % DECLIP_SLOTS, cnt[j], (long long)g[j]);
    }
#pragma unroll
    for (int j = 0; j < 2 * DECLIP_SLOTS; ++j) {
        const long long s = declip_wave_fold(j % DECLIP_SLOTS, cnt[j]);
        if (lane == 0) wave_cnt[wave][j] = s;
    }
    __syncthreads();
    if (tid < 2 * DECLIP_SLOTS) {
        const int k = tid % DECLIP_SLOTS;
        long long s = wave_cnt[0][tid];
#pragma unroll
        for (int w = 1; w < NW; ++w) s = declip_fold_slot<long long>(k, s, wave_cnt[w][tid]);
        a.totals[tid] = s;
    }
}

}  // namespace mgx
#endif
