// Loudness metering on the device: the K-weighted energy of every 100 ms sub-block, the 4x oversampled true peak and the
// sample peak of a track in HBM, in one launch that reads the frames once (loudness_plan.h has the definitions).
//
// A workgroup owns a run of `own` whole sub-blocks.  It starts at least `warmup` frames before them (clipped at frame 0)
// with filter state zero and walks to the end of its range in tiles of LOUD_TILE frames, so every e[s][c] is written by
// exactly one workgroup with a plain store: no atomics, no flags, nobody waits for anybody.  Per tile:
//   stage   the tile and an apron of 8 frames either side -> LDS (frames outside the track read as zero)
//   run     each thread takes LOUD_RUN consecutive frames from state zero (thread 0: from the state the last tile left)
//           and keeps the state v they leave
//   scan    eight steps of v[t] += P^(2^k) v[t - 2^k] through LDS: v[t] becomes the state behind thread t's frames
//   energy  each thread runs its frames again from its true entering state v[t - 1] and sums y^2, split at the one
//           sub-block boundary its run may hold; the same frames give its true-peak and sample-peak candidates
//   reduce  groups of 16 threads (256 frames: one boundary at most) are summed in thread order by one thread each,
//           then the groups of every sub-block of the tile in group order: a fixed order, so two runs agree bit for bit
// The phases are MGX_HD functions over a per-thread LoudThread, so that tests/emu/emu_loudness.cpp runs the same code;
// what the host decides of a launch -- the arguments but the pointers and the error slot -- is loudness_launch, for
// mgx_loudness and the emulation alike (the grid is the geometry's `workgroups`, the LDS LOUD_LDS_BYTES).
#pragma once

#include "mgx_hd.h"
#include "loudness_plan.h"

namespace mgx {

struct LoudnessArgs {
    const float* x;             // [n][2] float32
    long long n;
    const double* table;        // LOUD_TABLE_DOUBLES (loudness_plan.h)
    double c[10];               // shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2
    int S, own, warmup;
    long long nsub;
    double* e;                  // [nsub][2]
    double* peaks;              // [workgroups][2]: true peak, sample peak
    int* error;                 // the handle's error words, or null
    int error_slot;
};

// ---- what the host decides (mgx_loudness and the emulation alike) ------------------------------------------------------
// everything of the arguments but the pointers and the error slot
inline void loudness_launch(LoudnessArgs& a, const LoudnessPlan& plan, const LoudnessGeometry& g, long long n) {
    a.n = n, a.nsub = g.nsub;
    for (int i = 0; i < 10; ++i) a.c[i] = plan.c[i];
    a.S = g.S, a.own = g.own, a.warmup = g.warmup;
}

constexpr int LOUD_APRON = 8;                                               // >= LOUD_TP_AFTER, LOUD_TP_BEFORE
// a tile in LDS: frame i of [first - APRON, first + TILE + APRON) at slot i + i / 16, so that the threads of a wave,
// which read frames 16 apart, meet different banks
constexpr int LOUD_X_SLOTS = (LOUD_TILE + 2 * LOUD_APRON) + (LOUD_TILE + 2 * LOUD_APRON) / 16 + 1;
MGX_HD int loud_slot(int i) { return i + (i >> 4); }

// LDS of a workgroup, in bytes
constexpr int LOUD_GROUPS = LOUD_THREADS / 16;
constexpr size_t LOUD_LDS_X = 0;                                            // float2[LOUD_X_SLOTS]
constexpr size_t LOUD_LDS_SCAN = (LOUD_X_SLOTS * sizeof(float2) + 15) / 16 * 16;   // double[2][8][THREADS]; buffer 1 doubles as the energy rows
constexpr size_t LOUD_LDS_GROUP = LOUD_LDS_SCAN + 2 * 8 * LOUD_THREADS * sizeof(double);   // double[GROUPS][2][2]
constexpr size_t LOUD_LDS_ACC = LOUD_LDS_GROUP + LOUD_GROUPS * 4 * sizeof(double);         // double[OWN_MAX][2]
constexpr size_t LOUD_LDS_CARRY = LOUD_LDS_ACC + LOUD_OWN_MAX * 2 * sizeof(double);        // double[2][8]
constexpr size_t LOUD_LDS_BYTES = LOUD_LDS_CARRY + 2 * 8 * sizeof(double);

struct LoudLds {
    float2* x;
    double* scan;               // [2][8][THREADS]
    double* group;              // [GROUPS][channel][before / behind the boundary]
    double* acc;                // [OWN_MAX][2]
    double* carry;              // [2][8]
};
MGX_HD LoudLds loud_lds(char* base) {
    LoudLds l;
    l.x = reinterpret_cast<float2*>(base + LOUD_LDS_X);
    l.scan = reinterpret_cast<double*>(base + LOUD_LDS_SCAN);
    l.group = reinterpret_cast<double*>(base + LOUD_LDS_GROUP);
    l.acc = reinterpret_cast<double*>(base + LOUD_LDS_ACC);
    l.carry = reinterpret_cast<double*>(base + LOUD_LDS_CARRY);
    return l;
}

// what is the same for every thread of a workgroup
struct LoudRange {
    long long sub0, sub1;       // sub-blocks [sub0, sub1) are this workgroup's
    long long begin, end;       // frames [begin, end) give its peaks: its sub-blocks, and for the last workgroup the rest
    long long start;            // first frame it reads: begin - warmup or earlier, not below 0
    int tiles;
};
MGX_HD LoudRange loud_range(const LoudnessArgs& a, long long wg, long long workgroups) {
    LoudRange r;
    r.sub0 = wg * a.own;
    r.sub1 = r.sub0 + a.own < a.nsub ? r.sub0 + a.own : a.nsub;
    r.begin = r.sub0 * a.S;
    r.end = wg == workgroups - 1 ? a.n : r.sub1 * a.S;
    // at least `warmup` frames ahead of its sub-blocks, and as many more as make its last tile end where its range ends:
    // the frames a tile holds past that end would be run for nothing, the same number ahead lengthen the warm-up
    const long long latest = r.begin > a.warmup ? r.begin - a.warmup : 0;
    const long long whole = r.end - (r.end - latest + LOUD_TILE - 1) / LOUD_TILE * LOUD_TILE;
    r.start = whole > 0 ? whole : 0;
    r.tiles = (int)((r.end - r.start + LOUD_TILE - 1) / LOUD_TILE);
    return r;
}

struct LoudThread {
    double v[8];                // [channel][s1 s2 t1 t2]: the scan's value, then the state the thread's frames meet
    double true_peak, sample_peak;
    int bad;                    // a sample that is not a finite number
};

MGX_HD void loud_init(const LoudLds& l, int tid, LoudThread& th) {
    th.true_peak = th.sample_peak = 0.0;
    th.bad = 0;
    if (tid < 16) l.carry[tid] = 0.0;
    if (tid < LOUD_OWN_MAX * 2) l.acc[tid] = 0.0;
}

// phase "stage"
MGX_D void loud_stage(const LoudnessArgs& a, long long first, const LoudLds& l, int tid) {
    const MemView xv = mem_view(a.x, a.n * (long long)sizeof(float2));
    for (int i = tid; i < LOUD_TILE + 2 * LOUD_APRON; i += LOUD_THREADS) {
        // (a frame before the track wraps to an offset near 4 G, one behind it lies past the view: both read zero)
        const unsigned off = (unsigned)((first - LOUD_APRON + i) * (long long)sizeof(float2));
        l.x[loud_slot(i)] = ld_f2_or_zero(xv, off);
    }
}

// one frame of one channel through the cascade: z = (s1, s2, t1, t2), returns the K-weighted sample
MGX_HD double loud_frame(const double* c, double* z, double x) {
    const double y1 = fma(c[0], x, z[0]);
    z[0] = fma(-c[3], y1, fma(c[1], x, z[1]));
    z[1] = fma(-c[4], y1, c[2] * x);
    const double y2 = fma(c[5], y1, z[2]);
    z[2] = fma(-c[8], y2, fma(c[6], y1, z[3]));
    z[3] = fma(-c[9], y2, c[7] * y1);
    return y2;
}

MGX_HD void loud_scan_put(const LoudLds& l, int buffer, int tid, const LoudThread& th) {
    double* s = l.scan + buffer * 8 * LOUD_THREADS;
    MGX_UNROLL
    for (int i = 0; i < 8; ++i) s[i * LOUD_THREADS + tid] = th.v[i];
}

// phase "run": the state the thread's frames leave from zero -- thread 0 from the carried state -- into scan buffer 0
MGX_HD void loud_run(const LoudnessArgs& a, int tile, const LoudLds& l, int tid, LoudThread& th) {
    MGX_UNROLL
    for (int i = 0; i < 8; ++i) th.v[i] = tid == 0 ? l.carry[(tile & 1) * 8 + i] : 0.0;
    const float2* x = l.x + loud_slot(LOUD_APRON + tid * LOUD_RUN);         // (a run of 16 from a multiple of 16 + 8: slots
    MGX_UNROLL                                                              //  advance by one, with one gap after frame 7)
    for (int i = 0; i < LOUD_RUN; ++i) {
        const float2 f = x[i + (i >> 3)];
        loud_frame(a.c, th.v, (double)f.x);
        loud_frame(a.c, th.v + 4, (double)f.y);
    }
    loud_scan_put(l, 0, tid, th);
}

// phase "scan", step k (behind a barrier): v[t] += P^(2^k) v[t - 2^k], read from buffer k & 1, written to the other
MGX_HD void loud_scan_step(const LoudnessArgs& a, int k, const LoudLds& l, int tid, LoudThread& th) {
    const int from = tid - (1 << k);
    if (from >= 0) {
        const double* s = l.scan + (k & 1) * 8 * LOUD_THREADS + from;
        const double* P = a.table + LOUD_TABLE_POWERS + 16 * k;
        double p[8];
        MGX_UNROLL
        for (int i = 0; i < 8; ++i) p[i] = s[i * LOUD_THREADS];
        MGX_UNROLL
        for (int ch = 0; ch < 2; ++ch) {
            MGX_UNROLL
            for (int i = 0; i < 4; ++i) {
                double sum = th.v[4 * ch + i];
                MGX_UNROLL
                for (int j = 0; j < 4; ++j) sum = fma(P[4 * i + j], p[4 * ch + j], sum);
                th.v[4 * ch + i] = sum;
            }
        }
    }
    loud_scan_put(l, (k + 1) & 1, tid, th);
}

// phase "energy" (behind the barrier of the last scan step, whose values lie in buffer 0): the thread's frames again
// from the state they really meet; the energy of its run, before and behind the sub-block boundary, into the rows of
// buffer 1; its peak candidates
MGX_D void loud_energy(const LoudnessArgs& a, const LoudRange& r, int tile, const LoudLds& l, int tid, LoudThread& th) {
    if (tid == LOUD_THREADS - 1) {
        MGX_UNROLL
        for (int i = 0; i < 8; ++i) l.carry[((tile + 1) & 1) * 8 + i] = th.v[i];    // what the next tile's thread 0 starts from
    }
    MGX_UNROLL
    for (int i = 0; i < 8; ++i)
        th.v[i] = tid == 0 ? l.carry[(tile & 1) * 8 + i] : l.scan[i * LOUD_THREADS + tid - 1];
    const long long m0 = r.start + (long long)tile * LOUD_TILE + tid * LOUD_RUN;
    const unsigned sub = (unsigned)m0 / (unsigned)a.S;                      // (frames stay below 2^31: LOUD_FRAMES_MAX)
    const long long boundary = (long long)(sub + 1) * a.S;
    const int before = boundary - m0 < LOUD_RUN ? (int)(boundary - m0) : LOUD_RUN;  // frames of the run in sub-block `sub`
    const float2* x = l.x + loud_slot(LOUD_APRON + tid * LOUD_RUN);
    double e[4] = {0.0, 0.0, 0.0, 0.0};                                     // [behind the boundary][channel]
    MGX_UNROLL
    for (int i = 0; i < LOUD_RUN; ++i) {
        const float2 f = x[i + (i >> 3)];
        const double yl = loud_frame(a.c, th.v, (double)f.x);
        const double yr = loud_frame(a.c, th.v + 4, (double)f.y);
        const bool behind = i >= before;
        e[0] = fma(behind ? 0.0 : yl, yl, e[0]);
        e[1] = fma(behind ? 0.0 : yr, yr, e[1]);
        e[2] = fma(behind ? yl : 0.0, yl, e[2]);
        e[3] = fma(behind ? yr : 0.0, yr, e[3]);
        th.bad |= !(fabsf(f.x) <= 3.4028235e38f) || !(fabsf(f.y) <= 3.4028235e38f);
    }
    // the workgroup's range begins and ends on sub-block boundaries: each half of the run lies in it or outside
    const bool in0 = (long long)sub >= r.sub0 && (long long)sub < r.sub1;
    const bool in1 = (long long)sub + 1 >= r.sub0 && (long long)sub + 1 < r.sub1;
    double* rows = l.scan + 8 * LOUD_THREADS;
    rows[0 * LOUD_THREADS + tid] = in0 ? e[0] : 0.0;
    rows[1 * LOUD_THREADS + tid] = in0 ? e[1] : 0.0;
    rows[2 * LOUD_THREADS + tid] = in1 ? e[2] : 0.0;
    rows[3 * LOUD_THREADS + tid] = in1 ? e[3] : 0.0;

    // true peak: phase p of frame m is sum_j h[p + 4 j] x[m - j]; phase 0 is the frame itself.  The run's 16 frames
    // and the 5 before and 6 behind them are read once and kept as float64; h is even, so phase 3's taps are phase 1's
    // backwards and phase 2's are their own mirror: 18 numbers, which stay in scalar registers.
    if (m0 + LOUD_RUN <= r.begin || m0 >= r.end) return;
    const double* taps = a.table + LOUD_TABLE_TAPS;
    double h1[LOUD_TP_TAPS], h2[LOUD_TP_TAPS / 2];
    MGX_UNROLL
    for (int k = 0; k < LOUD_TP_TAPS; ++k) h1[k] = taps[k];
    MGX_UNROLL
    for (int k = 0; k < LOUD_TP_TAPS / 2; ++k) h2[k] = taps[LOUD_TP_TAPS + k];
    constexpr int WINDOW = LOUD_RUN + LOUD_TP_BEFORE + LOUD_TP_AFTER;       // frames m0 - 5 .. m0 + 21
    const int first = LOUD_APRON + tid * LOUD_RUN - LOUD_TP_BEFORE;
    double wl[WINDOW], wr[WINDOW];
    MGX_UNROLL
    for (int j = 0; j < WINDOW; ++j) {
        const float2 f = l.x[loud_slot(first + j)];
        wl[j] = (double)f.x;
        wr[j] = (double)f.y;
    }
    double tp = th.true_peak, sp = th.sample_peak;
    MGX_UNROLL
    for (int i = 0; i < LOUD_RUN; ++i) {
        double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        MGX_UNROLL
        for (int k = 0; k < LOUD_TP_TAPS; ++k) {
            // tap k reads frame m + LOUD_TP_AFTER - k: entry i + 11 - k of the window
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
        const bool mine = m0 + i >= r.begin && m0 + i < r.end;             // (a run may straddle an end of the range)
        sp = mine ? fmax(sp, peak) : sp;
        MGX_UNROLL
        for (int p = 0; p < 6; ++p) peak = fmax(peak, fabs(s[p]));
        tp = mine ? fmax(tp, peak) : tp;
    }
    th.sample_peak = sp;
    th.true_peak = tp;
}

// phase "reduce", first half: thread g * 16 + ch (ch < 2) sums group g's rows of channel ch in thread order, before and
// behind the one boundary the group's 256 frames may hold
MGX_HD void loud_reduce_groups(const LoudnessArgs& a, const LoudRange& r, int tile, const LoudLds& l, int tid) {
    const int g = tid >> 4, ch = tid & 15;
    if (ch >= 2) return;
    const double* rows = l.scan + 8 * LOUD_THREADS;
    const long long m0 = r.start + (long long)tile * LOUD_TILE + g * 16 * LOUD_RUN;
    const long long boundary = (long long)((unsigned)m0 / (unsigned)a.S + 1) * a.S;
    double first = 0.0, second = 0.0;
    for (int i = 0; i < 16; ++i) {
        const int t = g * 16 + i;
        const double e0 = rows[ch * LOUD_THREADS + t], e1 = rows[(2 + ch) * LOUD_THREADS + t];
        if (m0 + i * LOUD_RUN < boundary) {         // the thread's run starts in the group's first sub-block
            first += e0;
            second += e1;
        } else {
            second += e0;                           // (its second half is empty: S > 256)
        }
    }
    l.group[(g * 2 + ch) * 2] = first;
    l.group[(g * 2 + ch) * 2 + 1] = second;
}

// ... second half: thread q * 2 + ch adds the groups of the tile's q-th sub-block, in group order, to the accumulator
MGX_HD void loud_reduce_tile(const LoudnessArgs& a, const LoudRange& r, int tile, const LoudLds& l, int tid) {
    if (tid >= LOUD_TILE_SUBS * 2) return;
    const int q = tid >> 1, ch = tid & 1;
    const long long first = r.start + (long long)tile * LOUD_TILE;
    const long long sub = (long long)((unsigned)first / (unsigned)a.S) + q;
    if (sub < r.sub0 || sub >= r.sub1) return;
    double sum = 0.0;
    for (int g = 0; g < LOUD_GROUPS; ++g) {
        const long long sg = (long long)((unsigned)(first + g * 16 * LOUD_RUN) / (unsigned)a.S);
        if (sg == sub) sum += l.group[(g * 2 + ch) * 2];
        if (sg + 1 == sub) sum += l.group[(g * 2 + ch) * 2 + 1];
    }
    l.acc[(sub - r.sub0) * 2 + ch] += sum;
}

// behind the last tile: the workgroup's sub-block energies, and every thread's peaks into the scan area
MGX_HD void loud_finish_put(const LoudnessArgs& a, const LoudRange& r, const LoudLds& l, int tid, const LoudThread& th) {
    if (tid < a.own * 2 && r.sub0 + (tid >> 1) < r.sub1) a.e[(r.sub0 + (tid >> 1)) * 2 + (tid & 1)] = l.acc[tid];
    l.scan[tid] = th.true_peak;
    l.scan[LOUD_THREADS + tid] = th.sample_peak;
    l.scan[2 * LOUD_THREADS + tid] = th.bad ? 1.0 : 0.0;
}
MGX_HD void loud_finish_groups(const LoudLds& l, int tid) {
    if (tid >= LOUD_GROUPS) return;
    MGX_UNROLL
    for (int w = 0; w < 3; ++w) {
        double m = 0.0;
        for (int i = 0; i < 16; ++i) m = fmax(m, l.scan[w * LOUD_THREADS + tid * 16 + i]);
        l.group[w * LOUD_GROUPS + tid] = m;
    }
}
MGX_HD void loud_finish(const LoudnessArgs& a, long long wg, const LoudLds& l, int tid) {
    if (tid != 0) return;
    double m[3];
    for (int w = 0; w < 3; ++w) {
        m[w] = 0.0;
        for (int g = 0; g < LOUD_GROUPS; ++g) m[w] = fmax(m[w], l.group[w * LOUD_GROUPS + g]);
    }
    a.peaks[wg * 2] = m[0];
    a.peaks[wg * 2 + 1] = m[1];
    if (m[2] != 0.0 && a.error) a.error[a.error_slot] = 1;
}

#if defined(__HIPCC__) && !defined(MGX_HOST_EMU)
__global__ __launch_bounds__(LOUD_THREADS) void k_loudness(LoudnessArgs a) {
    extern __shared__ __attribute__((aligned(16))) char loud_smem[];
    const LoudLds l = loud_lds(loud_smem);
    const int tid = threadIdx.x;
    const LoudRange r = loud_range(a, blockIdx.x, gridDim.x);
    LoudThread th;
    loud_init(l, tid, th);
    for (int tile = 0; tile < r.tiles; ++tile) {
        loud_stage(a, r.start + (long long)tile * LOUD_TILE, l, tid);
        __syncthreads();
        loud_run(a, tile, l, tid, th);
        __syncthreads();
        for (int k = 0; k < LOUD_SCAN_STEPS; ++k) {
            loud_scan_step(a, k, l, tid, th);
            __syncthreads();
        }
        loud_energy(a, r, tile, l, tid, th);
        __syncthreads();
        loud_reduce_groups(a, r, tile, l, tid);
        __syncthreads();
        loud_reduce_tile(a, r, tile, l, tid);
    }
    __syncthreads();
    loud_finish_put(a, r, l, tid, th);
    __syncthreads();
    loud_finish_groups(l, tid);
    __syncthreads();
    loud_finish(a, blockIdx.x, l, tid);
}
#endif

}  // namespace mgx
