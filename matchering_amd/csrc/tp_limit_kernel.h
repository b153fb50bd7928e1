// True-peak look-ahead limiter for deliveries (include/mgx.h, mgx_tp_limit) -- tests/tp_limiter_oracle.py is the numpy form.
//
//     e[m]  = g max over the meter's four phases and both channels of |sum_j h[p + 4 j] x[m - j]|      (the meter's envelope)
//     d0[m] = 1 - c / e[m] where e[m] > c, else 0                                                       (required reduction)
//     d[m]  = max d0[m - L .. m + L]                                                                    (look-ahead and hold)
//     q[m]  = max(d[m], rho q[m - 1])                                                                   (release)
//     s[m]  = sum_|k|<=L (L + 1 - |k|) / (L + 1)^2 q[clamp(m + k, 0, n - 1)]                            (two box-cars of L + 1)
//     out[m][ch] = (float)(((double)x[m][ch] g) (1 - s[m]))
//
// Three launches over tiles of TPL_TILE frames, and nothing in them waits for another workgroup: no flags, no tickets,
// no atomics.  What crosses workgroups is carried by the launch boundary.
//   k_tp_envelope   stages a tile and an apron of 8 frames in LDS, computes e in float64 with the meter's register window
//                   (loudness_kernel.h) and writes the d0 plane, float32 rounded to nearest.
//   k_tp_aggregate  the release is q[m] = max(d[m], rho u[m - L - 1]) with u[p] = max_i<=p rho^(p - i) d0[i], a max-plus
//                   recurrence on the d0 plane itself.  Block k holds the TPL_BLOCK frames that END where tile k + 1's
//                   window into the plane BEGINS (frame (k + 1) T - 2 L - 2); its aggregate is u at its last frame from
//                   u = 0 at its first.
//   k_tp_apply      a tile's carry u[t0 - 2 L - 2] = max_j rho^(j T) agg[tile - 1 - j], cut where rho^(j T) < 2^-40 (q < 1:
//                   an absolute bound on the gain); then u, d (a windowed maximum by doubling, in place), q, the two
//                   box-cars as prefix sums, the multiply, the store and the tile's largest s.
// The phases are MGX_HD functions over a per-thread TplThread, so that tests/emu/emu_tp_limit.cpp runs the same code.
#pragma once

#include "mgx_hd.h"
#include "loudness_plan.h"

namespace mgx {

constexpr int TPL_THREADS = 256;
constexpr int TPL_RUN = 16;                                     // consecutive frames per thread
constexpr int TPL_TILE = TPL_THREADS * TPL_RUN;                 // T
constexpr int TPL_BLOCK = TPL_TILE;                             // B: frames of an aggregate
constexpr int TPL_GROUPS = TPL_THREADS / 16;
constexpr int TPL_APRON = 8;                                    // >= LOUD_TP_BEFORE, LOUD_TP_AFTER
constexpr int TPL_LOOKAHEAD_MAX = 2048;                         // 10 ms at 192 kHz is 1920
constexpr double TPL_RELEASE_MAX = 4194304.0;                   // 2^22 frames
constexpr int TPL_CUT_BITS = 40;                                // a carry below 2^-40 of its source is dropped

struct TpLimitArgs {
    const float* x;             // [n][2] float32
    long long n;
    float* out;                 // [n][2]
    double pre_gain, ceiling;
    double taps[18];            // phase 1's twelve taps (phase 3's backwards), then the first six of phase 2 (its own mirror)
    double rho;
    double rho_run, rho_run16;          // rho^16, rho^256: a thread's run and a group's in k_tp_aggregate
    double rho_chunk, rho_chunk16;      // rho^chunk, rho^(16 chunk): the same in k_tp_apply
    double rho_tile[9];                 // rho^(T 2^k), k = 0 .. 8
    int lookahead;              // L
    int chunk;                  // entries of u / q / the first prefix sum a thread of k_tp_apply owns
    int chunk2;                 // ... of the second prefix sum
    int lookback;               // aggregates a carry looks back over at most
    long long tiles;
    float* d0;                  // [tiles * T]
    double* agg;                // [tiles]
    double* peak;               // [tiles]: the tile's largest s
};

// ---- what the host decides (mgx_tp_limit and the emulation alike) ------------------------------------------------------
inline double tpl_rho_power(double release, double frames) { return release > 0.0 ? std::exp(-frames / release) : 0.0; }
inline int tpl_odd_chunk(int entries) { return ((entries + TPL_THREADS - 1) / TPL_THREADS) | 1; }   // (odd: the threads' runs start in different LDS banks)
inline size_t tpl_region_a(int L) {
    const size_t d0 = (size_t)(TPL_TILE + 4 * L + 1) * sizeof(float), sums = (size_t)(TPL_TILE + L + 1) * sizeof(double);
    return ((d0 > sums ? d0 : sums) + 15) / 16 * 16;
}
inline size_t tpl_region_b(int L) { return (size_t)TPL_THREADS * tpl_odd_chunk(TPL_TILE + 2 * L + 1) * sizeof(double); }
inline size_t tpl_apply_lds_bytes(int L) { return tpl_region_a(L) + tpl_region_b(L) + (TPL_THREADS + TPL_GROUPS) * sizeof(double); }
constexpr size_t TPL_ENVELOPE_SLOTS = (TPL_TILE + 2 * TPL_APRON) + (TPL_TILE + 2 * TPL_APRON) / 16 + 1;
constexpr size_t TPL_ENVELOPE_LDS_BYTES = TPL_ENVELOPE_SLOTS * sizeof(float2);
constexpr size_t TPL_AGGREGATE_LDS_BYTES = (TPL_THREADS + TPL_GROUPS) * sizeof(double);

// everything of the arguments but the pointers; `taps49` from loudness_true_peak_taps
inline void tpl_plan(TpLimitArgs& a, long long n, double pre_gain, double ceiling, int L, double release, const double* taps49) {
    a.n = n;
    a.pre_gain = pre_gain;
    a.ceiling = ceiling;
    for (int i = 0; i < LOUD_TP_TAPS; ++i) a.taps[i] = taps49[1 + 4 * (i - LOUD_TP_AFTER) + 24];        // x[m + 6 - i] by h[1 + 4 (i - 6)]
    for (int i = 0; i < LOUD_TP_TAPS / 2; ++i) a.taps[LOUD_TP_TAPS + i] = taps49[2 + 4 * (i - LOUD_TP_AFTER) + 24];
    a.lookahead = L;
    a.chunk = tpl_odd_chunk(TPL_TILE + 2 * L + 1);
    a.chunk2 = tpl_odd_chunk(TPL_TILE + L + 1);
    a.tiles = (n + TPL_TILE - 1) / TPL_TILE;
    a.rho = tpl_rho_power(release, 1.0);
    a.rho_run = tpl_rho_power(release, (double)TPL_RUN);
    a.rho_run16 = tpl_rho_power(release, 16.0 * TPL_RUN);
    a.rho_chunk = tpl_rho_power(release, (double)a.chunk);
    a.rho_chunk16 = tpl_rho_power(release, 16.0 * a.chunk);
    for (int k = 0; k < 9; ++k) a.rho_tile[k] = tpl_rho_power(release, (double)TPL_TILE * (double)(1 << k));
    // rho^(j T) < 2^-CUT  <=>  j > CUT ln 2 R / T
    const double reach = release > 0.0 ? std::ceil(TPL_CUT_BITS * 0.6931471805599453 * release / TPL_TILE) + 1.0 : 0.0;
    a.lookback = (int)(reach < (double)a.tiles ? reach : (double)a.tiles);
}

// ---- LDS ---------------------------------------------------------------------------------------------------------------
MGX_HD int tpl_slot(int i) { return i + (i >> 4); }             // frame i of a staged tile (loudness_kernel.h's layout)

struct TplLds {
    float* w;                   // region A: the window into the d0 plane, [T + 4 L + 1] ...
    double* sums;               // ... and, once that is spent, the second prefix sum, [T + L + 1]
    double* u;                  // region B: u, then q, then the first prefix sum, [THREADS * chunk]
    double* s;                  // [THREADS]
    double* g;                  // [GROUPS]
};
MGX_HD TplLds tpl_lds(char* base, size_t region_a, size_t region_b) {
    TplLds l;
    l.w = reinterpret_cast<float*>(base);
    l.sums = reinterpret_cast<double*>(base);
    l.u = reinterpret_cast<double*>(base + region_a);
    l.s = reinterpret_cast<double*>(base + region_a + region_b);
    l.g = l.s + TPL_THREADS;
    return l;
}

struct TplThread {
    float hold[TPL_RUN];        // the windowed maximum's values between its read and its write
    double in, pw;              // a scan's value from the thread's own group, and the decay from the group's start
    double carry;
    double qa, qb;              // q at the first and the last frame of the track the tile's window holds
    double total;
};

// ---- scans over the threads of a workgroup: s[t] is what thread t's entries leave from nothing -----------------------------
// max-plus with decay f per thread (F = f^16 per group).  First half: what reaches thread t from the earlier threads of
// its group of 16, and the group's own value into g; second half (behind a barrier): from the earlier groups as well.
MGX_HD void tpl_decay_group(const TplLds& l, int tid, double f, TplThread& th) {
    double in = 0.0, pw = 1.0;
    for (int u = tid & ~15; u < tid; ++u) {
        in = fmax(f * in, l.s[u]);
        pw *= f;
    }
    th.in = in;
    th.pw = pw;
    if ((tid & 15) == 15) l.g[tid >> 4] = fmax(f * in, l.s[tid]);
}
MGX_HD double tpl_decay_finish(const TplLds& l, int tid, double F, const TplThread& th) {
    double gin = 0.0;
    for (int u = 0; u < (tid >> 4); ++u) gin = fmax(F * gin, l.g[u]);
    return fmax(th.in, th.pw * gin);
}
// the same shape for sums, in thread order: two runs agree bit for bit
MGX_HD void tpl_sum_group(const TplLds& l, int tid, TplThread& th) {
    double in = 0.0;
    for (int u = tid & ~15; u < tid; ++u) in += l.s[u];
    th.in = in;
    if ((tid & 15) == 15) l.g[tid >> 4] = in + l.s[tid];
}
MGX_HD double tpl_sum_finish(const TplLds& l, int tid, const TplThread& th) {
    double gin = 0.0;
    for (int u = 0; u < (tid >> 4); ++u) gin += l.g[u];
    return gin + th.in;
}
// plain maximum: threads 0 .. 15 fold their group of s, then everybody (or whoever wants it) folds g
MGX_HD void tpl_max_groups(const TplLds& l, int tid) {
    if (tid >= TPL_GROUPS) return;
    double m = 0.0;
    for (int i = 0; i < 16; ++i) m = fmax(m, l.s[tid * 16 + i]);
    l.g[tid] = m;
}
MGX_HD double tpl_max_all(const TplLds& l) {
    double m = 0.0;
    for (int i = 0; i < TPL_GROUPS; ++i) m = fmax(m, l.g[i]);
    return m;
}

// d0 of frame f, zero outside the plane (frames behind the track inside it were written as zero)
MGX_HD float tpl_d0(const TpLimitArgs& a, long long f) { return f >= 0 && f < a.tiles * TPL_TILE ? a.d0[f] : 0.0f; }

// ---- k_tp_envelope -------------------------------------------------------------------------------------------------------
MGX_HD void tpl_envelope_stage(const TpLimitArgs& a, long long first, float2* lx, int tid) {
    const float2* x = reinterpret_cast<const float2*>(a.x);
    for (int i = tid; i < TPL_TILE + 2 * TPL_APRON; i += TPL_THREADS) {
        const long long m = first - TPL_APRON + i;
        lx[tpl_slot(i)] = m >= 0 && m < a.n ? x[m] : make_float2(0.0f, 0.0f);
    }
}

// the thread's 16 frames: phase p of frame m is sum_j h[p + 4 j] x[m - j], phase 0 the frame itself (loud_energy's window)
MGX_HD void tpl_envelope(const TpLimitArgs& a, long long first, const float2* lx, int tid) {
    double h1[LOUD_TP_TAPS], h2[LOUD_TP_TAPS / 2];
    MGX_UNROLL
    for (int k = 0; k < LOUD_TP_TAPS; ++k) h1[k] = a.taps[k];
    MGX_UNROLL
    for (int k = 0; k < LOUD_TP_TAPS / 2; ++k) h2[k] = a.taps[LOUD_TP_TAPS + k];
    constexpr int WINDOW = TPL_RUN + LOUD_TP_BEFORE + LOUD_TP_AFTER;
    const int start = TPL_APRON + tid * TPL_RUN - LOUD_TP_BEFORE;
    double wl[WINDOW], wr[WINDOW];
    MGX_UNROLL
    for (int j = 0; j < WINDOW; ++j) {
        const float2 f = lx[tpl_slot(start + j)];
        wl[j] = (double)f.x;
        wr[j] = (double)f.y;
    }
    float d[TPL_RUN];
    MGX_UNROLL
    for (int i = 0; i < TPL_RUN; ++i) {
        double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        MGX_UNROLL
        for (int k = 0; k < LOUD_TP_TAPS; ++k) {
            const double xl = wl[i + LOUD_TP_BEFORE + LOUD_TP_AFTER - k], xr = wr[i + LOUD_TP_BEFORE + LOUD_TP_AFTER - k];
            const double p2 = h2[k < LOUD_TP_TAPS / 2 ? k : LOUD_TP_TAPS - 1 - k];
            s[0] = fma(h1[k], xl, s[0]);
            s[1] = fma(h1[k], xr, s[1]);
            s[2] = fma(p2, xl, s[2]);
            s[3] = fma(p2, xr, s[3]);
            s[4] = fma(h1[LOUD_TP_TAPS - 1 - k], xl, s[4]);
            s[5] = fma(h1[LOUD_TP_TAPS - 1 - k], xr, s[5]);
        }
        double peak = fmax(fabs(wl[i + LOUD_TP_BEFORE]), fabs(wr[i + LOUD_TP_BEFORE]));
        MGX_UNROLL
        for (int p = 0; p < 6; ++p) peak = fmax(peak, fabs(s[p]));
        const double e = a.pre_gain * peak;
        // (a NaN compares false; the frames behind the track, which the interpolator's tail still reaches, ask for nothing)
        d[i] = e > a.ceiling && first + tid * TPL_RUN + i < a.n ? (float)(1.0 - a.ceiling / e) : 0.0f;
    }
    float4* out = reinterpret_cast<float4*>(a.d0 + first + tid * TPL_RUN);  // (the plane holds whole tiles)
    MGX_UNROLL
    for (int i = 0; i < TPL_RUN / 4; ++i) out[i] = make_float4(d[4 * i], d[4 * i + 1], d[4 * i + 2], d[4 * i + 3]);
}

// ---- k_tp_aggregate ------------------------------------------------------------------------------------------------------
// block k: frames [(k + 1) T - 2 L - 1 - T, (k + 1) T - 2 L - 1)
MGX_HD void tpl_aggregate_run(const TpLimitArgs& a, long long block, const TplLds& l, int tid) {
    const long long first = (block + 1) * TPL_TILE - 2 * a.lookahead - 1 - TPL_BLOCK + tid * TPL_RUN;
    double v = 0.0;
    MGX_UNROLL
    for (int i = 0; i < TPL_RUN; ++i) v = fmax((double)tpl_d0(a, first + i), a.rho * v);
    l.s[tid] = v;
}
MGX_HD void tpl_aggregate_finish(const TpLimitArgs& a, long long block, const TplLds& l, int tid, const TplThread& th) {
    const double in = tpl_decay_finish(l, tid, a.rho_run16, th);
    if (tid == TPL_THREADS - 1) a.agg[block] = fmax(l.s[tid], a.rho_run * in);
}

// ---- k_tp_apply ----------------------------------------------------------------------------------------------------------
// The tile's window into the plane starts at frame w0 = t0 - 2 L - 1 and holds T + 4 L + 1 entries; u, q and the first
// prefix sum are indexed by j: u[j] belongs to frame w0 + j, q[j] to frame t0 - L + j.
MGX_HD void tpl_apply_stage(const TpLimitArgs& a, long long tile, const TplLds& l, int tid) {
    const int L = a.lookahead;
    const long long w0 = tile * TPL_TILE - 2 * L - 1;
    for (int i = tid; i < TPL_TILE + 4 * L + 1; i += TPL_THREADS) l.w[i] = tpl_d0(a, w0 + i);
    // the carry: thread t looks at aggregates tile - 1 - j for j = t, t + 256, ...
    double pw = 1.0;
    MGX_UNROLL
    for (int k = 0; k < 8; ++k) pw = (tid >> k) & 1 ? pw * a.rho_tile[k] : pw;
    const long long reach = tile < a.lookback ? tile : a.lookback;
    double c = 0.0;
    for (long long j = tid; j < reach; j += TPL_THREADS) {
        c = fmax(c, pw * a.agg[tile - 1 - j]);
        pw *= a.rho_tile[8];
    }
    l.s[tid] = c;
}

// u over the thread's entries from nothing -- thread 0 from the carry
MGX_HD void tpl_apply_run(const TpLimitArgs& a, const TplLds& l, int tid, TplThread& th) {
    const int count = TPL_TILE + 2 * a.lookahead + 1;
    th.carry = tpl_max_all(l);
    double v = tid == 0 ? th.carry : 0.0;
    for (int r = 0; r < a.chunk; ++r) {
        const int i = tid * a.chunk + r;
        v = fmax(i < count ? (double)l.w[i] : 0.0, a.rho * v);
        l.u[i] = v;
    }
    th.total = v;
}
MGX_HD void tpl_put_total(const TplLds& l, int tid, const TplThread& th) { l.s[tid] = th.total; }

// ... and with what reaches them from the threads before
MGX_HD void tpl_apply_release(const TpLimitArgs& a, const TplLds& l, int tid, const TplThread& th) {
    const double in = tpl_decay_finish(l, tid, a.rho_chunk16, th);
    double p = a.rho;
    for (int r = 0; r < a.chunk; ++r) {
        const int i = tid * a.chunk + r;
        l.u[i] = fmax(l.u[i], p * in);
        p *= a.rho;
    }
}

// the windowed maximum by doubling, in place: step `step` turns maxima over 2^step entries into maxima over 2^(step + 1),
// a piece of T entries at a time in rising order -- a piece reads itself and entries ahead, never one that is written
MGX_HD int tpl_hold_steps(int L) {
    int k = 0;
    while ((2 << k) <= 2 * L + 1) ++k;
    return k;                                                   // 2^k <= 2 L + 1 < 2^(k + 1)
}
MGX_HD void tpl_hold_read(const TpLimitArgs& a, int step, int piece, const TplLds& l, int tid, TplThread& th) {
    const int count = TPL_TILE + 4 * a.lookahead + 1;
    MGX_UNROLL
    for (int e = 0; e < TPL_RUN; ++e) {
        const int i = piece * TPL_TILE + e * TPL_THREADS + tid, far = i + (1 << step);
        th.hold[e] = i < count ? pmax(l.w[i], far < count ? l.w[far] : 0.0f) : 0.0f;
    }
}
MGX_HD void tpl_hold_write(const TpLimitArgs& a, int piece, const TplLds& l, int tid, const TplThread& th) {
    const int count = TPL_TILE + 4 * a.lookahead + 1;
    MGX_UNROLL
    for (int e = 0; e < TPL_RUN; ++e) {
        const int i = piece * TPL_TILE + e * TPL_THREADS + tid;
        if (i < count) l.w[i] = th.hold[e];
    }
}

// q over the frames of the track, in place of u; entries of frames outside the track are left for tpl_apply_edges
MGX_HD void tpl_apply_q(const TpLimitArgs& a, long long tile, int steps, const TplLds& l, int tid) {
    const int L = a.lookahead, count = TPL_TILE + 2 * L, second = 2 * L + 1 - (1 << steps);
    const long long m0 = tile * TPL_TILE - L;
    for (int r = 0; r < a.chunk; ++r) {
        const int j = tid * a.chunk + r;
        if (j >= count) break;
        const long long m = m0 + j;
        double q = 0.0;
        if (m >= 0 && m < a.n) {
            const float d = pmax(l.w[j + 1], l.w[j + 1 + second]);          // frames m - L .. m + L: entries j + 1 .. j + 2 L + 1
            q = fmax((double)d, a.rho * l.u[j]);                            // u[j]: frame m - L - 1
        }
        l.u[j] = q;
    }
}
MGX_HD void tpl_apply_edges(const TpLimitArgs& a, long long tile, const TplLds& l, TplThread& th) {
    const long long m0 = tile * TPL_TILE - a.lookahead, last = m0 + TPL_TILE + 2 * a.lookahead - 1;
    th.qa = l.u[m0 < 0 ? -m0 : 0];
    th.qb = l.u[(last < a.n ? last : a.n - 1) - m0];
}

// exclusive prefix sums of q, the edge frames' values standing in for the frames outside the track; in place
MGX_HD void tpl_apply_sum1(const TpLimitArgs& a, long long tile, const TplLds& l, int tid, TplThread& th) {
    const int count = TPL_TILE + 2 * a.lookahead;
    const long long m0 = tile * TPL_TILE - a.lookahead;
    double sum = 0.0;
    for (int r = 0; r < a.chunk; ++r) {
        const int j = tid * a.chunk + r;
        const long long m = m0 + j;
        const double v = j >= count ? 0.0 : m < 0 ? th.qa : m >= a.n ? th.qb : l.u[j];
        l.u[j] = sum;
        sum += v;
    }
    th.total = sum;
}
MGX_HD void tpl_apply_offset1(const TpLimitArgs& a, const TplLds& l, int tid, const TplThread& th) {
    const double offset = tpl_sum_finish(l, tid, th);
    for (int r = 0; r < a.chunk; ++r) l.u[tid * a.chunk + r] += offset;
}
// the first box-car b[i] = P1[i + L + 1] - P1[i], i < T + L, and its exclusive prefix sums into region A
MGX_HD void tpl_apply_sum2(const TpLimitArgs& a, const TplLds& l, int tid, TplThread& th) {
    const int L = a.lookahead, count = TPL_TILE + L;
    double sum = 0.0;
    for (int r = 0; r < a.chunk2; ++r) {
        const int i = tid * a.chunk2 + r;
        if (i > count) break;
        l.sums[i] = sum;
        if (i < count) sum += l.u[i + L + 1] - l.u[i];
    }
    th.total = sum;
}
MGX_HD void tpl_apply_offset2(const TpLimitArgs& a, const TplLds& l, int tid, const TplThread& th) {
    const double offset = tpl_sum_finish(l, tid, th);
    for (int r = 0; r < a.chunk2; ++r) {
        const int i = tid * a.chunk2 + r;
        if (i > TPL_TILE + a.lookahead) break;
        l.sums[i] += offset;
    }
}

MGX_HD void tpl_apply_store(const TpLimitArgs& a, long long tile, const TplLds& l, int tid, TplThread& th) {
    const int L = a.lookahead;
    const double weight = (double)(L + 1) * (double)(L + 1);
    const float2* x = reinterpret_cast<const float2*>(a.x);
    float2* out = reinterpret_cast<float2*>(a.out);
    double peak = 0.0;
    MGX_UNROLL
    for (int e = 0; e < TPL_RUN; ++e) {
        const int o = e * TPL_THREADS + tid;
        const long long m = tile * TPL_TILE + o;
        if (m < a.n) {
            const double s = fmax((l.sums[o + L + 1] - l.sums[o]) / weight, 0.0);
            const double gain = 1.0 - s;
            const float2 f = x[m];
            out[m] = make_float2((float)(((double)f.x * a.pre_gain) * gain), (float)(((double)f.y * a.pre_gain) * gain));
            peak = fmax(peak, s);
        }
    }
    l.s[tid] = peak;
}
MGX_HD void tpl_apply_peak(const TpLimitArgs& a, long long tile, const TplLds& l, int tid) {
    if (tid == 0) a.peak[tile] = tpl_max_all(l);
}

#if defined(__HIPCC__) && !defined(MGX_HOST_EMU)
__global__ __launch_bounds__(TPL_THREADS) void k_tp_envelope(TpLimitArgs a) {
    extern __shared__ __attribute__((aligned(16))) char tpl_smem[];
    float2* lx = reinterpret_cast<float2*>(tpl_smem);
    const long long first = (long long)blockIdx.x * TPL_TILE;
    tpl_envelope_stage(a, first, lx, threadIdx.x);
    __syncthreads();
    tpl_envelope(a, first, lx, threadIdx.x);
}

__global__ __launch_bounds__(TPL_THREADS) void k_tp_aggregate(TpLimitArgs a) {
    extern __shared__ __attribute__((aligned(16))) char tpl_smem[];
    const TplLds l = tpl_lds(tpl_smem, 0, 0);
    const int tid = threadIdx.x;
    TplThread th;
    tpl_aggregate_run(a, blockIdx.x, l, tid);
    __syncthreads();
    tpl_decay_group(l, tid, a.rho_run, th);
    __syncthreads();
    tpl_aggregate_finish(a, blockIdx.x, l, tid, th);
}

__global__ __launch_bounds__(TPL_THREADS) void k_tp_apply(TpLimitArgs a, unsigned region_a, unsigned region_b) {
    extern __shared__ __attribute__((aligned(16))) char tpl_smem[];
    const TplLds l = tpl_lds(tpl_smem, region_a, region_b);
    const int tid = threadIdx.x;
    const long long tile = blockIdx.x;
    TplThread th;
    tpl_apply_stage(a, tile, l, tid);
    __syncthreads();
    tpl_max_groups(l, tid);
    __syncthreads();
    tpl_apply_run(a, l, tid, th);
    tpl_put_total(l, tid, th);                                  // (s was last read before the barrier above)
    __syncthreads();
    tpl_decay_group(l, tid, a.rho_chunk, th);
    __syncthreads();
    tpl_apply_release(a, l, tid, th);
    __syncthreads();
    const int steps = tpl_hold_steps(a.lookahead), pieces = (TPL_TILE + 4 * a.lookahead + 1 + TPL_TILE - 1) / TPL_TILE;
    for (int step = 0; step < steps; ++step)
        for (int piece = 0; piece < pieces; ++piece) {
            tpl_hold_read(a, step, piece, l, tid, th);
            __syncthreads();
            tpl_hold_write(a, piece, l, tid, th);
            __syncthreads();
        }
    tpl_apply_q(a, tile, steps, l, tid);
    __syncthreads();
    tpl_apply_edges(a, tile, l, th);
    __syncthreads();
    tpl_apply_sum1(a, tile, l, tid, th);
    tpl_put_total(l, tid, th);
    __syncthreads();
    tpl_sum_group(l, tid, th);
    __syncthreads();
    tpl_apply_offset1(a, l, tid, th);
    __syncthreads();
    tpl_apply_sum2(a, l, tid, th);
    tpl_put_total(l, tid, th);
    __syncthreads();
    tpl_sum_group(l, tid, th);
    __syncthreads();
    tpl_apply_offset2(a, l, tid, th);
    __syncthreads();
    tpl_apply_store(a, tile, l, tid, th);
    __syncthreads();
    tpl_max_groups(l, tid);
    __syncthreads();
    tpl_apply_peak(a, tile, l, tid);
}
#endif

}  // namespace mgx
