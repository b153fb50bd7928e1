// The audit (include/mgx.h, mgx_audit): one streaming pass over frames or file PCM in HBM, then one workgroup that folds
// what the pass left.  Two launches; no workgroup waits for another, no atomics, every sum in a fixed order.
//
// k_audit<BITS>: one workgroup per segment of AUDIT_SEGMENT frames (the last may be shorter).
//   stage   the segment's bytes -> LDS as they lie in memory, 16 bytes per load and thread, consecutive threads on
//           consecutive addresses; the last dwords one by one, and of a packed 24-bit stream that ends on half a dword
//           the last two bytes by a 2-byte load: no load touches a byte behind the stream.  Thread t's AUDIT_RUN frames
//           are W dwords, kept at stride W + 1 (odd), so that the threads of a wave read different banks.
//   walk    each thread takes its AUDIT_RUN consecutive frames in order: sums, peaks, counts, the three sub-block sums
//           split at the one sub-block boundary its frames may hold, and the run record of each predicate
//           (left at the rail, right at the rail, frame silent).
//   fold    run records by an ordered tree over the lanes (shuffles) and the waves (LDS); sums by wave_sum and the waves
//           in wave order.  The segment's record and its share of each sub-block it meets go to scratch.
// k_audit_merge: one workgroup; each thread folds a contiguous chunk of segment records in segment order, the same
//   ordered tree folds the threads; a run that crosses a segment border is settled by the combine step, the track's ends
//   by audit_finish.  Sub-block k is the sum of the shares of the segments that meet it, in segment order; thread t takes
//   the sub-blocks (and the segments' plain sums) t, t + T, ..., and the totals sum L^2, sum R^2 and sum L R are the
//   threads' sums of their sub-blocks, added by the same fixed tree every time.
//
// The run record is a monoid (audit_combine is associative, a record of length 0 its identity), written MGX_HD so that
// tests/emu/emu_audit.cpp folds it on the host in any association.
#pragma once

#include "mgx_hd.h"

namespace mgx {

constexpr int AUDIT_SEGMENT = 4096;             // frames of a workgroup: deliberately no multiple of a sub-block
constexpr int AUDIT_THREADS = 256;
constexpr int AUDIT_RUN = AUDIT_SEGMENT / AUDIT_THREADS;        // consecutive frames of a thread
constexpr int AUDIT_SUB_MIN = 800;              // the shortest sub-block (8000 Hz, loudness_plan.h LOUD_MIN_RATE)
constexpr int AUDIT_SUBS_MAX = AUDIT_SEGMENT / AUDIT_SUB_MIN + 2;   // sub-blocks a segment can meet
constexpr int AUDIT_MERGE_THREADS = 1024;

// A stretch of a predicate sequence, frames [start, start + len), seen from outside: the run it begins with and the run
// it ends with are open (a neighbour may lengthen them); every run between two false elements of the stretch is closed
// and counted.  prefix == len: the whole stretch is one run (then suffix == len too).
struct AuditRun {
    int start, len;
    int prefix, suffix;         // lengths of the open runs at either end
    int best, best_at;          // the longest closed run and its first frame (0, -1: none); of equal runs the earliest
    int events, samples;        // closed runs of at least min_run elements, and the elements inside them
    int first;                  // first frame of the first such run, -1: none
};

MGX_HD AuditRun audit_empty(int start) { return AuditRun{start, 0, 0, 0, 0, -1, 0, 0, -1}; }

// a run of j elements from frame `at` is closed
MGX_HD void audit_close(AuditRun& r, int j, int at, int min_run) {
    if (j > r.best) r.best = j, r.best_at = at;
    if (j >= min_run) {
        r.events += 1;
        r.samples += j;
        if (r.first < 0) r.first = at;
    }
}

// the stretch grows by one element
MGX_HD void audit_push(AuditRun& r, bool p, int min_run) {
    if (p) {
        if (r.prefix == r.len) r.prefix += 1;
        r.suffix += 1;
    } else {
        if (r.suffix > 0 && r.prefix != r.len) audit_close(r, r.suffix, r.start + r.len - r.suffix, min_run);
        r.suffix = 0;
    }
    r.len += 1;
}

// a, then b right behind it
MGX_HD AuditRun audit_combine(const AuditRun& a, const AuditRun& b, int min_run) {
    if (a.len == 0) return b;
    if (b.len == 0) return a;
    const bool whole_a = a.prefix == a.len, whole_b = b.prefix == b.len;
    AuditRun r = a;
    r.len = a.len + b.len;
    r.prefix = whole_a ? a.len + b.prefix : a.prefix;
    r.suffix = whole_b ? a.suffix + b.len : b.suffix;
    // the run across the border is closed where neither side is one run; a's closed runs come before it, b's behind it
    if (!whole_a && !whole_b && a.suffix + b.prefix > 0)
        audit_close(r, a.suffix + b.prefix, a.start + a.len - a.suffix, min_run);
    if (b.best > r.best) r.best = b.best, r.best_at = b.best_at;
    r.events += b.events;
    r.samples += b.samples;
    if (r.first < 0) r.first = b.first;
    return r;
}

// the whole track: its ends close the open runs.  prefix and suffix are left as they are (head and tail silence).
MGX_HD AuditRun audit_finish(const AuditRun& t, int min_run) {
    AuditRun r = t;
    if (t.len == 0) return r;
    r.best = 0, r.best_at = -1, r.events = 0, r.samples = 0, r.first = -1;
    if (t.prefix == t.len) {
        audit_close(r, t.len, t.start, min_run);
        return r;
    }
    if (t.prefix > 0) audit_close(r, t.prefix, t.start, min_run);
    if (t.best > r.best) r.best = t.best, r.best_at = t.best_at;
    r.events += t.events;
    r.samples += t.samples;
    if (r.first < 0) r.first = t.first;
    if (t.suffix > 0) audit_close(r, t.suffix, t.start + t.len - t.suffix, min_run);
    return r;
}

constexpr int AUDIT_RAIL_L = 0, AUDIT_RAIL_R = 1, AUDIT_SILENT = 2, AUDIT_PREDICATES = 3;

// what k_audit leaves of a segment
struct AuditSegment {
    double sum[2], peak[2];
    AuditRun run[AUDIT_PREDICATES];
    int nonfinite[2];
};

// what k_audit_merge leaves of the track: the measured fields of mgx_audit_report
struct AuditTotals {
    double sum[2], sumsq[2], peak[2], sum_lr;
    long long nonfinite[2];
    long long clip_events[2], clip_samples[2], clip_longest[2], clip_first[2];
    long long head_silence, tail_silence, gap_longest, gap_at;
};

struct AuditArgs {
    const void* x;              // [n][2] float32 or PCM
    long long n;
    int B;                      // frames of a sub-block
    int subs;                   // sub-block slots of a segment in `part`: AUDIT_SEGMENT / B + 2
    int clip_run;
    double clip_level, silence_level;
    long long segments, count;  // segments, sub-blocks
    AuditSegment* seg;          // [segments]
    double* part;               // [segments][subs][3]: the segment's share of the q-th sub-block it meets
    AuditTotals* totals;
    double* sub_sums;           // [count][3]
};

// ---- what the host decides (everything of the arguments but the pointers) ----------------------------------------------
inline long long audit_segments(long long n) { return (n + AUDIT_SEGMENT - 1) / AUDIT_SEGMENT; }
inline long long audit_sub_blocks(long long n, int B) { return (n + B - 1) / B; }
inline void audit_launch(AuditArgs& a, long long n, int B, double clip_level, double silence_level, int clip_run) {
    a.n = n, a.B = B, a.subs = AUDIT_SEGMENT / B + 2;
    a.clip_run = clip_run, a.clip_level = clip_level, a.silence_level = silence_level;
    a.segments = audit_segments(n), a.count = audit_sub_blocks(n, B);
}
// bytes of scratch, in the order seg, part, totals, sub_sums (each a multiple of 8 bytes)
inline size_t audit_seg_bytes(const AuditArgs& a) { return (size_t)a.segments * sizeof(AuditSegment); }
inline size_t audit_part_bytes(const AuditArgs& a) { return (size_t)a.segments * a.subs * 3 * sizeof(double); }
inline size_t audit_result_bytes(const AuditArgs& a) { return sizeof(AuditTotals) + (size_t)a.count * 3 * sizeof(double); }

}  // namespace mgx

#if defined(__HIPCC__) && !defined(MGX_HOST_EMU)
#include "wave_util.h"

namespace mgx {

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ AuditRun audit_shfl_down(const AuditRun& r, int o) {
    AuditRun s;
    s.start = __shfl_down(r.start, o, 64), s.len = __shfl_down(r.len, o, 64);
    s.prefix = __shfl_down(r.prefix, o, 64), s.suffix = __shfl_down(r.suffix, o, 64);
    s.best = __shfl_down(r.best, o, 64), s.best_at = __shfl_down(r.best_at, o, 64);
    s.events = __shfl_down(r.events, o, 64), s.samples = __shfl_down(r.samples, o, 64);
    s.first = __shfl_down(r.first, o, 64);
    return s;
}

// The records of `lanes` consecutive lanes folded in lane order: an ordered tree, the result on lane 0.
__device__ __forceinline__ AuditRun audit_wave_fold(AuditRun r, int min_run, int lanes = 64) {
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < lanes; o <<= 1) {
        const AuditRun behind = audit_shfl_down(r, o);
        if ((lane & (2 * o - 1)) == 0) r = audit_combine(r, behind, min_run);
    }
    return r;
}

// ... and of the THREADS threads of a workgroup in thread order; the result on thread 0.  `waves`: THREADS / 64 records
// of LDS that nobody else touches until the next barrier.
template <int THREADS>
__device__ __forceinline__ AuditRun audit_block_fold(AuditRun r, int min_run, AuditRun* waves) {
    constexpr int NW = THREADS / 64;
    r = audit_wave_fold(r, min_run);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x < 64) {
        r = threadIdx.x < NW ? waves[threadIdx.x] : audit_empty(0);
        r = audit_wave_fold(r, min_run, NW);
    }
    return r;
}

// sample s (two per frame) of the thread's dwords, as a double; `finite` false for a NaN or an infinity
template <int BITS>
__device__ __forceinline__ double audit_sample(const unsigned* mine, int s, bool& finite) {
    finite = true;
    if constexpr (BITS == 0) {
        const float f = __uint_as_float(mine[s]);
        finite = fabsf(f) <= 3.4028235e38f;
        return finite ? (double)f : 0.0;
    } else if constexpr (BITS == 32) {
        return (double)(int)mine[s] * (1.0 / 2147483648.0);
    } else if constexpr (BITS == 16) {
        const unsigned w = mine[s >> 1];
        return (double)(short)((s & 1) ? (w >> 16) : (w & 0xffffu)) * (1.0 / 32768.0);
    } else {                                    // bytes 3 s .. 3 s + 2, little-endian
        const int w = (3 * s) >> 2, shift = ((3 * s) & 3) * 8;
        unsigned v = mine[w] >> shift;
        if (shift > 8) v |= mine[w + 1] << (32 - shift);
        return (double)((int)(v << 8) >> 8) * (1.0 / 8388608.0);
    }
}

template <int BITS>
__global__ __launch_bounds__(AUDIT_THREADS) void k_audit(AuditArgs a) {
    constexpr int FRAME_BYTES = BITS == 16 ? 4 : BITS == 24 ? 6 : 8;
    constexpr int W = AUDIT_RUN * FRAME_BYTES / 4;              // dwords of a thread's frames: 16, 24 or 32
    constexpr int NW = AUDIT_THREADS / 64;
    constexpr int SLOTS = 2 + 3 * AUDIT_SUBS_MAX;               // sum[2], then three sums per sub-block met
    static_assert(W % 4 == 0, "a 16-byte load stays inside one thread's dwords");
    __shared__ unsigned raw[AUDIT_THREADS * (W + 1)];
    __shared__ double wave_sums[NW][SLOTS];
    __shared__ double wave_peaks[NW][2];
    __shared__ int wave_counts[NW][2];
    __shared__ AuditRun wave_runs[AUDIT_PREDICATES][NW];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long first = (long long)blockIdx.x * AUDIT_SEGMENT;
    const int frames = (int)(a.n - first < AUDIT_SEGMENT ? a.n - first : AUDIT_SEGMENT);
    const int bytes = frames * FRAME_BYTES;
    const char* base = static_cast<const char*>(a.x) + first * FRAME_BYTES;     // 16-byte aligned: x is, a segment's bytes are a multiple

    // ---- stage ----
    const int quads = bytes >> 4;
#pragma unroll
    for (int k = 0; k < W / 4; ++k) {
        const int q = tid + k * AUDIT_THREADS;
        if (q < quads) {
            const uint4 v = reinterpret_cast<const uint4*>(base)[q];
            unsigned* to = raw + 4 * q + (4 * q) / W;
            to[0] = v.x, to[1] = v.y, to[2] = v.z, to[3] = v.w;
        }
    }
    if (tid < 4) {                                              // what is left of the last 16 bytes: whole dwords, then two bytes
        const int d = 4 * quads + tid, at = 4 * d;
        if (at + 4 <= bytes) raw[d + d / W] = *reinterpret_cast<const unsigned*>(base + at);
        else if (at + 2 <= bytes) raw[d + d / W] = *reinterpret_cast<const unsigned short*>(base + at);
    }
    __syncthreads();

    // ---- walk ----
    const unsigned* mine = raw + tid * (W + 1);
    const int m0 = (int)first + tid * AUDIT_RUN;                // (frames stay below 2^31: LOUD_FRAMES_MAX)
    const int mine_frames = frames - tid * AUDIT_RUN < 0 ? 0 : frames - tid * AUDIT_RUN < AUDIT_RUN ? frames - tid * AUDIT_RUN : AUDIT_RUN;
    const int B = a.B;
    const int sub0 = (int)((unsigned)first / (unsigned)B);      // the first sub-block the segment meets
    const int sub = (int)((unsigned)m0 / (unsigned)B);          // ... and the thread
    const int before = (sub + 1) * B - m0 < AUDIT_RUN ? (sub + 1) * B - m0 : AUDIT_RUN;     // its frames in `sub`; the rest in sub + 1
    const double clip = a.clip_level, quiet = a.silence_level;
    const int clip_run = a.clip_run;
    double sum[2] = {0.0, 0.0}, peak[2] = {0.0, 0.0};
    double e[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};               // [behind the boundary][L^2, R^2, L R]
    int bad[2] = {0, 0};
    AuditRun run[AUDIT_PREDICATES];
#pragma unroll
    for (int p = 0; p < AUDIT_PREDICATES; ++p) run[p] = audit_empty(m0);
#pragma unroll
    for (int i = 0; i < AUDIT_RUN; ++i) {
        if (i < mine_frames) {
            bool fl, fr;
            const double xl = audit_sample<BITS>(mine, 2 * i, fl), xr = audit_sample<BITS>(mine, 2 * i + 1, fr);
            const double al = fabs(xl), ar = fabs(xr);
            const double ll = xl * xl, rr = xr * xr, lr = xl * xr;      // (a sample that is not finite is 0 here)
            sum[0] += xl;
            sum[1] += xr;
            peak[0] = fmax(peak[0], al);
            peak[1] = fmax(peak[1], ar);
            bad[0] += !fl;
            bad[1] += !fr;
            const bool behind = i >= before;
            e[0] += behind ? 0.0 : ll;
            e[1] += behind ? 0.0 : rr;
            e[2] += behind ? 0.0 : lr;
            e[3] += behind ? ll : 0.0;
            e[4] += behind ? rr : 0.0;
            e[5] += behind ? lr : 0.0;
            audit_push(run[AUDIT_RAIL_L], fl && al >= clip, clip_run);
            audit_push(run[AUDIT_RAIL_R], fr && ar >= clip, clip_run);
            audit_push(run[AUDIT_SILENT], fl && fr && al <= quiet && ar <= quiet, 1);
        }
    }

    // ---- fold ----
    const int subs = (int)((unsigned)(first + frames - 1) / (unsigned)B) - sub0 + 1;        // sub-blocks the segment meets: <= a.subs
    const int q0 = sub - sub0;
    for (int c = 0; c < 2; ++c) {
        const double s = wave_sum(sum[c]), m = wave_max_f64(peak[c]);
        const int k = wave_sum_int(bad[c]);
        if (lane == 0) wave_sums[wave][c] = s, wave_peaks[wave][c] = m, wave_counts[wave][c] = k;
    }
    for (int q = 0; q < subs; ++q) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double s = wave_sum(q == q0 ? e[c] : q == q0 + 1 ? e[3 + c] : 0.0);
            if (lane == 0) wave_sums[wave][2 + 3 * q + c] = s;
        }
    }
    AuditRun total[AUDIT_PREDICATES];
#pragma unroll
    for (int p = 0; p < AUDIT_PREDICATES; ++p)          // (the barrier inside also publishes the sums above)
        total[p] = audit_block_fold<AUDIT_THREADS>(run[p], p == AUDIT_SILENT ? 1 : clip_run, wave_runs[p]);
    AuditSegment* out = a.seg + blockIdx.x;
    if (tid < 2 + 3 * subs) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) s += wave_sums[w][tid];
        if (tid < 2) out->sum[tid] = s;
        else a.part[(size_t)blockIdx.x * a.subs * 3 + (tid - 2)] = s;
    }
    if (tid >= 64 && tid < 66) {
        const int c = tid - 64;
        double m = 0.0;
        int k = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) m = fmax(m, wave_peaks[w][c]), k += wave_counts[w][c];
        out->peak[c] = m;
        out->nonfinite[c] = k;
    }
    if (tid == 0) {
#pragma unroll
        for (int p = 0; p < AUDIT_PREDICATES; ++p) out->run[p] = total[p];
    }
}

// (a template only so that its code is emitted with the other templates' instantiations, behind the kernels of the
//  master call: a plain kernel would lie in front of them and move every one of them in the code object)
template <int UNUSED>
__global__ __launch_bounds__(AUDIT_MERGE_THREADS) void k_audit_merge(AuditArgs a) {
    constexpr int T = AUDIT_MERGE_THREADS, NW = T / 64;
    __shared__ AuditRun wave_runs[AUDIT_PREDICATES][NW];
    __shared__ double wave_sums[NW][5];
    __shared__ double wave_peaks[NW][2];
    __shared__ long long wave_counts[NW][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int clip_run = a.clip_run;

    // ---- the segment records' runs: a contiguous chunk per thread, in segment order ----
    const long long per = (a.segments + T - 1) / T;
    const long long s0 = tid * per < a.segments ? tid * per : a.segments;
    const long long s1 = s0 + per < a.segments ? s0 + per : a.segments;
    AuditRun run[AUDIT_PREDICATES];
#pragma unroll
    for (int p = 0; p < AUDIT_PREDICATES; ++p) run[p] = audit_empty(0);
#pragma unroll 2
    for (long long s = s0; s < s1; ++s) {
        const AuditSegment* g = a.seg + s;
#pragma unroll
        for (int p = 0; p < AUDIT_PREDICATES; ++p) run[p] = audit_combine(run[p], g->run[p], p == AUDIT_SILENT ? 1 : clip_run);
    }
    // ---- their sums, peaks and counts: thread t takes the segments t, t + T, ... (any fixed order serves a sum) ----
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                    // sum[2], then sum L^2, sum R^2, sum L R
    double peak[2] = {0.0, 0.0};
    long long bad[2] = {0, 0};
#pragma unroll 2
    for (long long s = tid; s < a.segments; s += T) {
        const AuditSegment* g = a.seg + s;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            v[c] += g->sum[c];
            peak[c] = fmax(peak[c], g->peak[c]);
            bad[c] += g->nonfinite[c];
        }
    }

    // ---- the sub-blocks t, t + T, ...: each the shares of the segments that meet it, in segment order ----
    // (frames stay below 2^31, LOUD_FRAMES_MAX: 32-bit divisions; the shares are read-only here, so that the loads of
    //  one sub-block need not wait for the stores of the one before)
    const unsigned B = (unsigned)a.B;
    const double* __restrict__ part = a.part;
    double* __restrict__ sub_sums = a.sub_sums;
#pragma unroll 2
    for (long long k = tid; k < a.count; k += T) {
        const unsigned begin = (unsigned)k * B;
        const unsigned end = (long long)begin + B < a.n ? begin + B : (unsigned)a.n;
        const unsigned g0 = begin / AUDIT_SEGMENT, g1 = (end - 1) / AUDIT_SEGMENT;
        double acc[3] = {0.0, 0.0, 0.0};
        for (unsigned g = g0; g <= g1; ++g) {
            const unsigned q = (unsigned)k - g * AUDIT_SEGMENT / B;     // sub-block k is the q-th that segment g meets
            const double* share = part + ((size_t)g * a.subs + q) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += share[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            sub_sums[k * 3 + c] = acc[c];
            v[2 + c] += acc[c];
        }
    }

    // ---- the threads, in thread order ----
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const double s = wave_sum(v[c]);
        if (lane == 0) wave_sums[wave][c] = s;
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const double m = wave_max_f64(peak[c]);
        long long k = bad[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) k += __shfl_xor(k, o, 64);
        if (lane == 0) wave_peaks[wave][c] = m, wave_counts[wave][c] = k;
    }
    AuditRun total[AUDIT_PREDICATES];
#pragma unroll
    for (int p = 0; p < AUDIT_PREDICATES; ++p)          // (the barrier inside also publishes the sums above)
        total[p] = audit_block_fold<T>(run[p], p == AUDIT_SILENT ? 1 : clip_run, wave_runs[p]);
    AuditTotals* out = a.totals;
    if (tid >= 64 && tid < 69) {
        const int c = tid - 64;
        double s = 0.0;
        for (int w = 0; w < NW; ++w) s += wave_sums[w][c];
        if (c < 2) out->sum[c] = s;
        else if (c < 4) out->sumsq[c - 2] = s;
        else out->sum_lr = s;
    }
    if (tid >= 128 && tid < 130) {
        const int c = tid - 128;
        double m = 0.0;
        long long k = 0;
        for (int w = 0; w < NW; ++w) m = fmax(m, wave_peaks[w][c]), k += wave_counts[w][c];
        out->peak[c] = m;
        out->nonfinite[c] = k;
    }
    if (tid == 0) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const AuditRun r = audit_finish(total[c], clip_run);
            out->clip_events[c] = r.events;
            out->clip_samples[c] = r.samples;
            out->clip_longest[c] = r.best;
            out->clip_first[c] = r.first;
        }
        const AuditRun& q = total[AUDIT_SILENT];                // (not finished: a gap lies strictly between two frames that are not silent)
        out->head_silence = q.prefix;
        out->tail_silence = q.suffix;
        out->gap_longest = q.best;
        out->gap_at = q.best_at;
    }
}

}  // namespace mgx
#endif
