// The level-correction stage (stages.py:138-170) on the device; the host side is run_correction.h.
// Device only, and the only place this logic exists:
//   * CorrectionState, the stage's scalars, and k_clipped_sumsq (the stage-level API's one round),
//   * the band split of the mid plane (BandInfo, BandChunk) and RoundArgs,
//   * k_correction_round: one round per launch, the last workgroup to arrive decides (correction_decide),
//   * k_correction_tail: every round after the first in one resident grid (poll_word, tail_decider),
//   * k_correction_init and k_finalize_scalars.
// MGX_TAIL_TRACE builds stamp the phases (tools/tail_trace.py); MGX_TEST_TAIL_* builds make a tail give up
// (tests/test_device_errors.py).
#pragma once

#include "levels_kernels.h"
#include "limiter_kernel.h"
#include "wave_util.h"

namespace mgx {

#ifdef MGX_TEST_TAIL_EXPIRE       // tests/test_device_errors.py: the tails this process has launched (tail_decider)
__device__ int g_test_tail_launches;
#endif

#ifdef MGX_TAIL_TRACE      // experiments: 100 MHz timestamps of the phases (tools/tail_trace.py)
__device__ unsigned long long g_tail_trace[160 * 32];
__device__ unsigned long long g_round_trace[8];
#define TAIL_STAMP(slot) do { if (threadIdx.x == 0 && blockIdx.x < 160) g_tail_trace[blockIdx.x * 32 + (slot)] = wall_clock64(); } while (0)
#define ROUND_STAMP(slot) do { if (threadIdx.x == 0) g_round_trace[slot] = wall_clock64(); } while (0)
#else
#define TAIL_STAMP(slot) do {} while (0)
#define ROUND_STAMP(slot) do {} while (0)
#endif
// ---------------------------------------------------------------------------
// level correction (stages.py:138-170)
// ---------------------------------------------------------------------------
struct CorrectionState {
    double gain;              // product of the coefficients so far
    double coeffs[16];
    double result_peak;       // max |gain * y|
    double normalize_c;       // stages.py:186-191
    int limiter_active;
    int steps_done;
};
// What a call's back half reads and writes once round 0 of the level correction has been launched: the correction
// state and the reference's two scalars.  One per handle (handle.h, mgx_handle::back), like y and mid, not one per
// call context: round 0's launch (k_finalize_scalars where there are no rounds) copies the state the front half reset
// and the two scalars out of the context, and every launch behind it works here.  The context is then free for the
// front half of the next call but one.
struct BackState {
    CorrectionState cs;
    double reference_match_rms;         // TrackStats::match_rms of the reference, or its profile's
    double reference_amplitude_c;       // ... and its amplitude coefficient (the limiter's post gain)
};
static_assert(offsetof(BackState, reference_amplitude_c) == offsetof(BackState, reference_match_rms) + sizeof(double),
              "RoundArgs::back_refs addresses the two scalars as [0] and [1]");

// partial[d*chunks + ch] = sum over the chunk of clip(gain*mid, -1, 1)^2
__global__ __launch_bounds__(256) void k_clipped_sumsq(const float* mid, long long piece, int chunks,
                                                       const double* gain_ptr, double gain_mul,
                                                       double* partial) {
    __shared__ double scratch[4];
    const int d = blockIdx.x / chunks, ch = blockIdx.x % chunks;
    const long long len = (piece + chunks - 1) / chunks;
    const long long b = (long long)d * piece + ch * len;
    const long long e = min((long long)(d + 1) * piece, b + len);
    const double g = (gain_ptr ? *gain_ptr : 1.0) * gain_mul;
    double acc = 0.0;
    // float64 product then clip: the reference clips the float64 mid (dsp.py:109-110)
    long long i = b + threadIdx.x;
    for (; i + 3 * 256 < e; i += 4 * 256) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = mid[i + u * 256];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double c = fmin(fmax((double)v[u] * g, -1.0), 1.0);
            acc = fma(c, c, acc);
        }
    }
    for (; i < e; i += 256) {
        const double c = fmin(fmax((double)mid[i] * g, -1.0), 1.0);
        acc = fma(c, c, acc);
    }
    const double s = block_sum<256>(acc, scratch);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// One round of stages.py:149-168 in ONE launch: every workgroup sums its chunk of
// clip(gain*mid)^2, and the workgroup that arrives last at the ticket counter takes the decision
// (loud pieces, coefficient, accumulated gain) -- split-K style "last arriver combines"
// (MI355X_MICROARCH.md, fanin / splitk-seam): partials are published write-through (sc1) and drained
// before the ticket, the last arriver acquires before reading them.  With `final_peaks` the same
// workgroup also derives the peak / limiter early-out / normalisation scalars (k_finalize_scalars).
// Band bookkeeping of one workgroup's chunk (k_correction_round).  Every correction coefficient is
// close to 1 (it is the ratio of two loudness estimates of nearly the same signal), so the
// accumulated gain g of an ordinary pair stays inside [BAND_G_LO, BAND_G_HI].  For such g a sample with
// |m| <= 1/BAND_G_HI is never clipped (contributes g^2 m^2), one with |m| > 1/BAND_G_LO always is
// (contributes 1), and only the few samples in between -- the band -- need to be looked at again.
// Round 0 streams the whole mid plane once, evaluates its own sum directly AND leaves
// {sum of m^2 of the never-clipped, count of the always-clipped, the band's values compacted per
// wave}; later rounds read just that (a few MB instead of 85) unless the gain has left the range,
// in which case they stream the plane again.  The split is exact: sum min(g^2 m^2, 1) is the same
// number either way, up to float64 summation order.
constexpr double BAND_G_LO = 0.7, BAND_G_HI = 1.5;
constexpr int BAND_SLACK = 2048;             // floats of padding per workgroup in the band buffer
// float32 thresholds on |m|, each rounded towards the inside of the band: |m| <= never implies
// |m| <= 1/BAND_G_HI exactly, |m| >= always implies |m| > 1/BAND_G_LO
__device__ __forceinline__ float band_threshold_never() {
    const float t = (float)(1.0 / BAND_G_HI);
    return (double)t <= 1.0 / BAND_G_HI ? t : __uint_as_float(__float_as_uint(t) - 1u);
}
__device__ __forceinline__ float band_threshold_always() {
    const float t = (float)(1.0 / BAND_G_LO);
    return (double)t > 1.0 / BAND_G_LO ? t : __uint_as_float(__float_as_uint(t) + 1u);
}
struct BandInfo {
    double unclipped_sumsq;                  // A: sum of m^2 over |m| <= 1/BAND_G_HI
    double clipped_count;                    // C: samples with |m| > 1/BAND_G_LO
    int count[4];                            // band samples compacted by each of the four waves
    int pad[2];
};
// frames [b, e) of chunk `ch` of piece `d`, and where the four per-wave band lists of that chunk start:
// a region of (e - b) + BAND_SLACK floats per chunk, a quarter of it (each wave sees a quarter of the
// chunk's samples, give or take the scalar head and tail) per wave
struct BandChunk {
    long long b, e, wave_cap;
    float* lists;
};
__device__ __forceinline__ BandChunk band_chunk(float* band, long long piece, int chunks, int d, int ch) {
    BandChunk c;
    const long long len = (piece + chunks - 1) / chunks;
    c.b = (long long)d * piece + ch * len;
    c.e = min((long long)(d + 1) * piece, c.b + len);
    c.wave_cap = (c.e - c.b + 3) / 4 + BAND_SLACK / 4 - 4;
    c.lists = band + c.b + ((long long)d * chunks + ch) * BAND_SLACK;
    return c;
}
struct RoundArgs {
    const float* mid;
    long long piece;
    int chunks, divisions;
    double* partial;            // [divisions][chunks]
    unsigned* arrivals;         // [1 + divisions] counters, zero between launches: [0] pieces done, [1+d] chunks of piece d
    const double* reference_match_rms;      // round 0: in the reference's TrackStats or profile; later launches: in the BackState
    double eps, threshold;
    CorrectionState* cs;                    // the BackState's
    // round 0 alone (null in every later launch): what it copies into the BackState (back_state_fill) -- the context's
    // state as the front half reset it (-> *cs), *reference_match_rms and *front_amplitude_c (-> back_refs[0], [1])
    const CorrectionState* front_cs;
    const double* front_amplitude_c;
    double* back_refs;
    const float* final_peaks;   // per-pair peaks of the convolution, or null
    long long npeaks;
    float* band;                // [n + workgroups * BAND_SLACK] compacted band samples
    BandInfo* info;             // [workgroups]
    int build_band;             // 1: round 0 (stream + build), 0: later rounds (use the band if g allows)
    int step;                   // index of the (first) round this launch runs
    // the limiter's look-back words, preset to "unpublished" here when a limiter launch follows (saves
    // two fill launches on the stream); null otherwise
    unsigned long long* lim_published;
    long long lim_words;
    int* lim_ticket;
    unsigned long long* tail_gains;   // [tail_rounds + 1] gains published between the rounds of k_correction_tail (slot r:
                                      // the gain after its round r; slot tail_rounds: the gain after round 0), or null;
                                      // behind them [tail_rounds][tail_total] words for its workgroups' partial sums
                                      // (the value is the flag)
    int tail_total;                   // summing workgroups of the k_correction_tail launch that follows (0: none);
                                      // with one, this launch leaves its partials and the decision to that kernel
    int tail_rounds;                  // rounds that kernel runs (rms_correction_steps - 1; any number: defaults.py:118-120)
    int* error;                       // set when a bounded wait expired
};
// Round 0's copy into the BackState.  Where the launch takes a decision, the ONE thread that takes it copies first (its
// stores to *cs follow the copy in program order).  Where k_correction_tail decides, the copy rides along in workgroup
// 0 (BackFillLane): nobody else writes the BackState in that launch.  The launch boundary makes it visible to whatever
// follows.
__device__ __forceinline__ void back_state_fill(const RoundArgs& a) {
    if (!a.front_cs) return;
    *a.cs = *a.front_cs;
    a.back_refs[0] = *a.reference_match_rms;
    a.back_refs[1] = *a.front_amplitude_c;
}
// The same copy as one 8-byte word per lane: loaded on entry, stored on exit, so that the latency of the (cold) loads
// passes under the workgroup's own streaming instead of holding its first wave up before it starts (a thread that
// loaded and stored on the spot made workgroup 0, and with it the launch, about a microsecond late).
typedef unsigned long long __attribute__((may_alias)) back_word;
constexpr int BACK_STATE_WORDS = (int)(sizeof(CorrectionState) / sizeof(back_word));
static_assert(sizeof(CorrectionState) % sizeof(back_word) == 0, "the CorrectionState is copied in 8-byte words");
struct BackFillLane {
    back_word word = 0;
    back_word* to = nullptr;
    __device__ __forceinline__ void load(const RoundArgs& a, int w) {
        if (!a.front_cs || w >= BACK_STATE_WORDS + 2) return;
        const back_word* from = w < BACK_STATE_WORDS    ? reinterpret_cast<const back_word*>(a.front_cs) + w
                                : w == BACK_STATE_WORDS ? reinterpret_cast<const back_word*>(a.reference_match_rms)
                                                        : reinterpret_cast<const back_word*>(a.front_amplitude_c);
        to = w < BACK_STATE_WORDS ? reinterpret_cast<back_word*>(a.cs) + w
                                  : reinterpret_cast<back_word*>(a.back_refs) + (w - BACK_STATE_WORDS);
        word = *from;
    }
    __device__ __forceinline__ void store() const {
        if (to) *to = word;
    }
};
// The decision of one round (stages.py:149-168), taken by ONE 256-thread workgroup after every partial
// sum has been published: piece sums -> loud pieces -> coefficient -> accumulated gain; with
// `final_peaks` also the peak / limiter early-out / normalisation scalars.  `total` partials, `per`
// of them per piece.  Every load is a cold miss: issued in batches of eight per thread, staged in LDS.
// `step` = index of this round, `gain_in` = the gain it ran with: nothing is read back from the
// CorrectionState, whose last writer may sit behind another XCD's L2 when rounds share a launch.
__device__ __forceinline__ double correction_decide(const RoundArgs& a, int total, int per, double* red, double* sums,
                                                    bool reset_arrivals, int step, double gain_in) {
    double* stage = sums + a.divisions;                          // [total]
    for (int k0 = threadIdx.x; k0 < total; k0 += 8 * 256) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)       // (write-through stores on the other side, L2-bypassing loads here)
            v[u] = k0 + 256 * u < total ? __hip_atomic_load(a.partial + k0 + 256 * u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (k0 + 256 * u < total) stage[k0 + 256 * u] = v[u];
    }
    __shared__ float fscratch[4];
    __shared__ double new_gain;
    float m = 0.f;
    if (a.final_peaks) {
        for (long long k0 = threadIdx.x; k0 < a.npeaks; k0 += 8 * 256) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = k0 + 256 * u < a.npeaks ? a.final_peaks[k0 + 256 * u] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) m = fmaxf(m, v[u]);
        }
    }
    __syncthreads();
    // (the last arriver works alone while the chip waits: lanes side by side on a piece and ONE wave's decision,
    // 2.5 us where wave-per-piece sums and three block-wide reductions took 5.3 -- profiles/r03_z_correction_phases.txt)
    piece_sums_by_groups(stage, per, a.divisions, sums);
    float pk = 0.f;
    if (a.final_peaks) pk = block_max<256>(m, fscratch);                   // (uniform)
    double avg = 0.0, match = 1.0;
    int count = 0;
    if (threadIdx.x < 64) wave_decide(sums, a.divisions, a.piece, 1.0, nullptr, nullptr, avg, match, count);
    if (threadIdx.x == 0) {
        const double c = *a.reference_match_rms / fmax(a.eps, match);      // match_levels.py:106-111
        back_state_fill(a);
        CorrectionState* cs = a.cs;
        new_gain = gain_in * c;
        if (step < 16) cs->coeffs[step] = c;
        cs->steps_done = step + 1;
        cs->gain = new_gain;
        if (a.final_peaks) {
            const double peak = (double)(float)((double)pk * new_gain);      // max |float32(y*gain)|
            cs->result_peak = peak;
            const double rect = fmax(peak, a.threshold) / a.threshold;
            cs->limiter_active = fabs(rect - 1.0) > (1e-8 + 1e-5) ? 1 : 0;   // numpy.isclose defaults, hyrax.py:83
            cs->normalize_c = fmax(a.eps, peak / a.threshold);               // dsp.py:93-100
        }
        if (reset_arrivals)                                                  // ready for the next round or launch
            __hip_atomic_store(a.arrivals, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    return new_gain;
}

__global__ __launch_bounds__(256) void k_correction_round(RoundArgs a) {
    if (blockIdx.x == 0) ROUND_STAMP(0);
    warm_code(CODE_ROUND);
    MGX_LDS;
    double* red = reinterpret_cast<double*>(mgx_smem);          // 64 doubles of scratch
    double* sums = red + 64;                                     // [divisions]
    __shared__ int is_last;
    const int d = blockIdx.x / a.chunks, ch = blockIdx.x % a.chunks;
    const BandChunk bc = band_chunk(a.band, a.piece, a.chunks, d, ch);
    const long long b = bc.b, e = bc.e;
    const double g = (a.front_cs ? a.front_cs : a.cs)->gain;    // (round 0 starts from the context's state: the copy is under way)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (a.tail_gains && blockIdx.x == 0)                                                         // "not yet": k_correction_tail
        for (int i = threadIdx.x; i < a.tail_rounds + 1 + a.tail_rounds * a.tail_total; i += 256) a.tail_gains[i] = ~0ull;
    BackFillLane back_fill;                                     // (no decision in this launch: stored on the way out)
    if (a.build_band && a.tail_total > 0 && blockIdx.x == 0) back_fill.load(a, threadIdx.x);
    if (a.lim_published) {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.lim_words; i += (long long)gridDim.x * 256)
            a.lim_published[i] = ~0ull;
        if (blockIdx.x == 0 && threadIdx.x == 0) a.lim_ticket[0] = a.lim_ticket[2] = 0;      // ticket and "gave up" (run_limiter.h run_limiter); a raised error sticks
    }
    // this workgroup's slice of the band buffer, one compacted list per wave
    float* wave_band = bc.lists + wave * bc.wave_cap;
    BandInfo* info = a.info + blockIdx.x;
    double acc = 0.0;
    // float64 product then clip: the reference clips the float64 mid (dsp.py:109-110)
    auto add = [&](float v) {
        const double c = fmin(fmax((double)v * g, -1.0), 1.0);
        acc = fma(c, c, acc);
    };
    const bool use_band = !a.build_band && g >= BAND_G_LO && g <= BAND_G_HI;
    if (use_band) {
        const int count = info->count[wave];
        for (int k = lane; k < count; k += 64) add(wave_band[k]);
        if (threadIdx.x == 0) acc += g * g * info->unclipped_sumsq + info->clipped_count;
    } else {
        // Straight-line per-sample code (no divergent branches: every lane walks the same iterations and
        // masks with `ok`; a branchy version of this loop made round 0 instruction-bound).  The band
        // test runs in float32 against thresholds rounded INTO the band, which can only move a sample
        // from the closed-form parts into the list -- the sum is the same either way.
        double low = 0.0;
        int filled = 0, clipped = 0;          // wave-uniform: band samples stored, always-clipped samples seen
        const unsigned long long below = (1ull << lane) - 1ull;
        const float t_never = band_threshold_never(), t_always = band_threshold_always();
        const bool build = a.build_band != 0;
        auto visit = [&](float v, bool ok) {
            const double d = (double)(ok ? v : 0.f);
            const double c = fmin(fmax(d * g, -1.0), 1.0);
            acc = fma(c, c, acc);
            if (build) {                       // uniform
                const float m = fabsf(v);
                const bool never = ok && m <= t_never, always = ok && m >= t_always;
                low = fma(never ? d : 0.0, d, low);
                clipped += __popcll(__ballot(always));
                const bool in_band = ok && !never && !always;
                const unsigned long long mask = __ballot(in_band);
                const long long slot = filled + __popcll(mask & below);
                if (in_band && slot < bc.wave_cap) wave_band[slot] = v;      // (a wave's quarter + slack never overflows)
                filled += __popcll(mask);
            }
        };
        // scalar head up to a 16-byte boundary, float4 body (64 B per thread in flight), scalar tail
        const long long head = min(e, (b + 3) & ~3ll);
        {
            const bool ok = b + threadIdx.x < head;
            visit(ok ? a.mid[b + threadIdx.x] : 0.f, ok);
        }
        const long long body_end = head + ((e - head) & ~3ll);
        int clipped_mine = 0;                  // per thread (the fast path below)
        if (build && g == 1.0) {
            // Round 0 of mgx_master (the level gain of stages.py:80-88 is in the filter, so g is exactly 1):
            // float32 arithmetic -- clip(v) is exact, the squares are summed 16 at a time before they join
            // the float64 sums -- and the band samples are compacted per THREAD: each thread counts its
            // own, one prefix sum over the wave places them, no ballot and no scalar chain per sample.
            // (A frame past the end loads as 0: clips to 0, counts as never clipped, adds nothing.)
            // Four 16-byte loads per thread in flight, the sixteen samples then summed and compacted in order.  Two and
            // three such groups in flight were measured in round 6 -- the whole stage 52.1 -> 54.2 / 54.3 us -- as were
            // more, shorter workgroups (51.5 -> 56.1 at twice as many): this kernel is not short of loads in flight
            // (profiles/r06_b_*, r06_g_*).
            for (long long s0 = head; s0 < body_end; s0 += 4 * 1024) {
                float x[16];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const long long i = s0 + u * 1024 + 4ll * threadIdx.x;
                    const float4 q = i < body_end ? *reinterpret_cast<const float4*>(a.mid + i) : make_float4(0.f, 0.f, 0.f, 0.f);
                    x[4 * u] = q.x; x[4 * u + 1] = q.y; x[4 * u + 2] = q.z; x[4 * u + 3] = q.w;
                }
                float sq = 0.f, lo = 0.f;
                int mine = 0;
                unsigned bits = 0;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float c = __builtin_amdgcn_fmed3f(x[i], -1.0f, 1.0f);
                    sq = fmaf(c, c, sq);
                    const float m = fabsf(x[i]);
                    const bool never = m <= t_never, always = m >= t_always;
                    lo = fmaf(never ? x[i] : 0.f, x[i], lo);
                    clipped_mine += always ? 1 : 0;
                    const bool in_band = !never && !always;
                    mine += in_band ? 1 : 0;
                    bits |= (in_band ? 1u : 0u) << i;
                }
                acc += (double)sq;
                low += (double)lo;
                const int through = wave_inclusive_sum(mine);
                int slot = filled + through - mine;
                if (bits) {
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        if (bits & (1u << i)) {
                            if (slot < bc.wave_cap) wave_band[slot] = x[i];
                            ++slot;
                        }
                }
                filled += __builtin_amdgcn_readlane(through, 63);
            }
        } else
        for (long long s0 = head; s0 < body_end; s0 += 4 * 1024) {
            float4 v[4];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long long i = s0 + u * 1024 + 4ll * threadIdx.x;
                ok[u] = i < body_end;
                v[u] = ok[u] ? *reinterpret_cast<const float4*>(a.mid + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                visit(v[u].x, ok[u]);
                visit(v[u].y, ok[u]);
                visit(v[u].z, ok[u]);
                visit(v[u].w, ok[u]);
            }
        }
        {
            const bool ok = body_end + threadIdx.x < e;
            visit(ok ? a.mid[body_end + threadIdx.x] : 0.f, ok);
        }
        if (build) {
            if (lane == 0) info->count[wave] = filled;
            const double lo = block_sum<256>(low, red);
            __syncthreads();
            const double hi = block_sum<256>((lane == 0 ? (double)clipped : 0.0) + (double)clipped_mine, red + 8);
            if (threadIdx.x == 0) {
                info->unclipped_sumsq = lo;
                info->clipped_count = hi;
            }
            __syncthreads();
        }
    }
    const double s = block_sum<256>(acc, red);
    if (a.build_band && a.tail_total > 0) {                              // uniform: k_correction_tail decides round 0
        if (threadIdx.x == 0) a.partial[blockIdx.x] = s;
        back_fill.store();
        return;
    }
    if (threadIdx.x == 0) {
        // write-through 8-byte store + drained vmcnt instead of a release fence (a fence per workgroup
        // would write back the XCD's whole L2 two thousand times)
        __hip_atomic_store(a.partial + blockIdx.x, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // two-level arrival count (one word takes ~88 atomics per microsecond; 2048 workgroups on a
        // single word would cost more than the sums themselves)
        is_last = 0;
        if (atomicAdd(a.arrivals + 1 + d, 1u) == (unsigned)a.chunks - 1) {
            a.arrivals[1 + d] = 0;                                         // ready for the next launch
            is_last = atomicAdd(a.arrivals, 1u) == (unsigned)a.divisions - 1;
        }
        if (is_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
    if (!is_last) return;
    ROUND_STAMP(1);
    correction_decide(a, a.divisions * a.chunks, a.chunks, red, sums, true, a.step, g);
    ROUND_STAMP(2);
}

// Rounds 1 .. K-1 of stages.py:149-168 in ONE launch.  After round 0 a round only touches the band
// lists (a few MB) and a handful of scalars, so a launch per round was mostly launch, ramp and a chain
// of cold round trips: 16 us each for ~1 us of work.  Here a small grid (divisions x groups workgroups,
// at most ~128: every one of them must be resident at once, also next to other handles' kernels) keeps
// running.  Before the first round a workgroup adds up the closed-form parts of its chunks, copies
// their band lists into LDS (when they fit) and reduces its share of the convolution's pair peaks; a
// round is then: sum from LDS -> publish the partial as an 8-byte word whose value is the flag (preset
// to all-ones by round 0) -> the deciding workgroup (one past the summing ones: tail_decider, which also
// takes round 0's decision while the others copy their lists) polls the words, one lane per word, decides
// with one wave and publishes the new gain the same way -> everybody polls it (one lane, bounded) and goes on.  Every wait
// is bounded and raises the handle's error word.  A gain outside [BAND_G_LO, BAND_G_HI] makes a
// workgroup stream its part of the mid plane instead (slow with so few workgroups).  Ordinary pairs stay inside
// the band -- coefficients are ratios of two loudness estimates of nearly the same signal -- but hard material does
// leave it: a sparse or narrow-band target against a dense reference goes below BAND_G_LO from round 1 on
// (running gains 0.35 .. 0.07, 0.61 .. 0.54, 0.52), an ordinary target against a hard-clipped reference crosses
// BAND_G_HI in the middle of the tail, a click train reaches 35 (tests/test_gpu_band_exits.py holds each).
// Phase stamps of this kernel and of round 0's last workgroup: profiles/r03_z_correction_phases.txt
// (-DMGX_TAIL_TRACE, tools/tail_trace.py).
#ifdef MGX_TEST_TAIL_MAX_SPINS                             // tests/test_device_errors.py: a tail that gives up quickly
constexpr int TAIL_MAX_SPINS = MGX_TEST_TAIL_MAX_SPINS;
#else
constexpr int TAIL_MAX_SPINS = 0;                          // product: bounded by time (wait_on, limiter_kernel.h)
#endif
// one lane's bounded wait for an 8-byte flag word to leave the all-ones pattern (`on_expiry` and the error word on expiry)
__device__ __forceinline__ unsigned long long poll_word(const unsigned long long* w, int* error, unsigned long long on_expiry) {
    unsigned long long v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int spins = 0;
    long long t0 = 0;
    while (v == ~0ull && wait_on(spins, t0, nullptr, TAIL_MAX_SPINS)) {
        if (spins < 64) __builtin_amdgcn_s_sleep(1);
        else __builtin_amdgcn_s_sleep(16);
        v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ++spins;
    }
    if (v == ~0ull) {
        error[DEVICE_ERROR_SLOT_TAIL] = 1;
        v = on_expiry;
    }
    return v;
}
// CorrectionState::coeffs mirrors mgx_report: the first 16 coefficients are kept for the log, the product of all is the gain
__device__ __forceinline__ void keep_coefficient(CorrectionState* cs, int step, double c) {
    if (step < 16) __hip_atomic_store(&cs->coeffs[step], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The deciding workgroup of k_correction_tail (the one past the summing ones).  First round 0's decision from the
// partials k_correction_round left (the launch boundary made them visible; that kernel skips its own arrival
// count and decision when a tail follows -- they were 4 us with the whole chip waiting, here they run beside the
// other workgroups' list copies), then every round: poll the summing workgroups' words, decide, publish.
__device__ __forceinline__ void tail_decider(const RoundArgs& a, int groups, int rounds, int total, double* red, double* sums,
                                             double* stage, double* stage0, float* fscratch) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __shared__ double decided;
    double* peak_words = a.partial + (size_t)a.divisions * a.chunks;
    const float* final_peaks = a.final_peaks;
    auto put = [](double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto puti = [](int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    {
        const int n0 = a.divisions * a.chunks;
        for (int k0 = threadIdx.x; k0 < n0; k0 += 8 * 256) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = k0 + 256 * u < n0 ? a.partial[k0 + 256 * u] : 0.0;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (k0 + 256 * u < n0) stage0[k0 + 256 * u] = v[u];
        }
        const double gain_in = a.cs->gain;
        __syncthreads();
        piece_sums_by_groups(stage0, a.chunks, a.divisions, sums);
        if (wave == 0) {
            double avg, match;
            int count;
            wave_decide(sums, a.divisions, a.piece, 1.0, nullptr, nullptr, avg, match, count);
            if (lane == 0) {
                const double c = *a.reference_match_rms / fmax(a.eps, match);          // match_levels.py:106-111
                const double next = gain_in * c;
#ifdef MGX_TEST_TAIL_EXPIRE               // tests/test_device_errors.py: the first tail of the process never hears of round 0's gain
                if (atomicAdd(&g_test_tail_launches, 1) > 0)
#endif
                __hip_atomic_store(a.tail_gains + a.tail_rounds, double_bits(next), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                keep_coefficient(a.cs, a.step - 1, c);
                decided = next;
            }
        }
        __syncthreads();
    }
    double g = decided;
    for (int r = 0; r < rounds; ++r) {
        const unsigned long long* words = a.tail_gains + a.tail_rounds + 1 + (size_t)r * total;
        const bool last_round = r == rounds - 1;
        for (int k = threadIdx.x; k < total; k += 256) stage[k] = bits_double(poll_word(words + k, a.error, 0ull));
        asm volatile("" ::: "memory");        // the peak words are read AFTER their flag words were seen (compiler order;
                                              // the publisher waited for its peak store before it stored the flag)
        float m = 0.f;
        if (last_round && final_peaks)
            for (int k = threadIdx.x; k < total; k += 256)
                m = fmaxf(m, (float)__hip_atomic_load(peak_words + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        __syncthreads();
        for (int p = threadIdx.x; p < a.divisions; p += 256) {
            double t = 0.0;
            for (int q = 0; q < groups; ++q) t += stage[p * groups + q];
            sums[p] = t;
        }
        const float pk = block_max<256>(m, fscratch);                     // (barrier inside: sums[] is complete after it)
        if (wave == 0) {
            double avg, match;
            int count;
            wave_decide(sums, a.divisions, a.piece, 1.0, nullptr, nullptr, avg, match, count);
            if (lane == 0) {
                const double c = *a.reference_match_rms / fmax(a.eps, match);          // match_levels.py:106-111
                const double next = g * c;
                // the gain word first: a hundred workgroups are polling it
                if (!last_round)
                    __hip_atomic_store(a.tail_gains + r, double_bits(next), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                CorrectionState* cs = a.cs;
                keep_coefficient(cs, a.step + r, c);
                if (last_round) {
                    puti(&cs->steps_done, a.step + r + 1);
                    put(&cs->gain, next);
                    if (final_peaks) {
                        const double peak = (double)(float)((double)pk * next);      // max |float32(y*gain)|
                        const double rect = fmax(peak, a.threshold) / a.threshold;
                        put(&cs->result_peak, peak);
                        puti(&cs->limiter_active, fabs(rect - 1.0) > (1e-8 + 1e-5) ? 1 : 0);   // numpy.isclose defaults, hyrax.py:83
                        put(&cs->normalize_c, fmax(a.eps, peak / a.threshold));               // dsp.py:93-100
                    }
                }
                decided = next;
            }
        }
        __syncthreads();
        g = decided;
    }
}
constexpr int TAIL_CACHE_PER_WAVE = 3072;        // floats of band list a wave keeps in LDS
__host__ __device__ inline size_t correction_tail_lds_bytes(int divisions, int groups, int chunks) {
    const size_t cache = (size_t)4 * TAIL_CACHE_PER_WAVE * 4, stage0 = (size_t)divisions * chunks * 8;   // (the decider's)
    return ((size_t)64 + divisions + (size_t)divisions * groups) * 8 + (cache > stage0 ? cache : stage0) + 16;
}
__global__ __launch_bounds__(256) void k_correction_tail(RoundArgs a, int groups, int rounds) {
    warm_code(CODE_TAIL);
    TAIL_STAMP(0);
    MGX_LDS;
    double* red = reinterpret_cast<double*>(mgx_smem);          // 64 doubles of scratch
    double* sums = red + 64;                                     // [divisions]
    double* stage = sums + a.divisions;                          // [divisions * groups]
    float* cache = reinterpret_cast<float*>(stage + a.divisions * groups);
    __shared__ double gain_now;
    __shared__ float fscratch[4];
    const int d = blockIdx.x / groups, grp = blockIdx.x % groups;
    const int ch0 = (int)((long long)grp * a.chunks / groups), ch1 = (int)((long long)(grp + 1) * a.chunks / groups);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, total = a.divisions * groups;
    if (a.lim_published) {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.lim_words; i += (long long)gridDim.x * 256)
            a.lim_published[i] = ~0ull;
        if (blockIdx.x == 0 && threadIdx.x == 0) a.lim_ticket[0] = a.lim_ticket[2] = 0;      // ticket and "gave up" (run_limiter.h run_limiter); a raised error sticks
    }
    TAIL_STAMP(1);
    if ((int)blockIdx.x == total) {                                      // uniform: the extra workgroup decides
        tail_decider(a, groups, rounds, total, red, sums, stage, reinterpret_cast<double*>(cache), fscratch);
        return;
    }
    // ---- once: closed-form parts and band lists of this workgroup's chunks (lane c <-> chunk ch0 + c) ----
    const int nch = ch1 - ch0;                                           // <= 64 (host)
    int my_count = 0;
    double part_a = 0.0, part_c = 0.0;
    if (lane < nch) {
        const BandInfo* info = a.info + d * a.chunks + ch0 + lane;
        my_count = info->count[wave];
        if (wave == 0) { part_a = info->unclipped_sumsq; part_c = info->clipped_count; }
    }
    const double closed_a = wave_sum(part_a), closed_c = wave_sum(part_c);   // meaningful on wave 0
    int before = my_count;                                               // exclusive prefix of the counts over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(before, o, 64);
        if (lane >= o) before += v;
    }
    const int wave_total = __shfl(before, 63, 64);
    before -= my_count;
    const bool cached = wave_total <= TAIL_CACHE_PER_WAVE;               // uniform per wave
    float* mine = cache + wave * TAIL_CACHE_PER_WAVE;
    if (cached) {
        // two chunks' lists at a time, six loads per lane and list in flight before the first is stored: a loop
        // of load -> wait -> store per 64 samples was 48 round trips in a row (profiles/r03_z_correction_phases.txt).
        // (Four chunks at a time, the first four asked for before the counts are known, eight chunks at a time
        // with 16-byte loads, and round 0's loads software-pipelined were all measured slower: more loads in
        // flight on these cold, scattered lists cost more than they hide.)
        constexpr int PER = 6;
        for (int c0 = 0; c0 < nch; c0 += 2) {
            const float* list[2];
            int n[2], off[2];
            float v[2][PER];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int c = c0 + u < nch ? c0 + u : c0;
                const BandChunk bc = band_chunk(a.band, a.piece, a.chunks, d, ch0 + c);
                list[u] = bc.lists + wave * bc.wave_cap;
                n[u] = c0 + u < nch ? __shfl(my_count, c, 64) : 0;
                off[u] = __shfl(before, c, 64);
#pragma unroll
                for (int j = 0; j < PER; ++j) v[u][j] = lane + 64 * j < n[u] ? list[u][lane + 64 * j] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
#pragma unroll
                for (int j = 0; j < PER; ++j)
                    if (lane + 64 * j < n[u]) mine[off[u] + lane + 64 * j] = v[u][j];
                for (int k = lane + 64 * PER; k < n[u]; k += 64) mine[off[u] + k] = list[u][k];
            }
        }
    }
    // this workgroup's share of the convolution's pair peaks, for the decider of the last round
    float my_peak = 0.f;
    if (a.final_peaks) {
        float m = 0.f;
        for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < a.npeaks; k += (long long)total * 256)
            m = fmaxf(m, a.final_peaks[k]);
        my_peak = block_max<256>(m, fscratch);
    }
    double* peak_words = a.partial + (size_t)a.divisions * a.chunks;     // [total], behind round 0's partials
    const float* final_peaks = a.final_peaks;
    TAIL_STAMP(2);
    if (threadIdx.x == 0) gain_now = bits_double(poll_word(a.tail_gains + a.tail_rounds, a.error, double_bits(1.0)));
    __syncthreads();
    double g = gain_now;                                                 // round 0's, from the deciding workgroup
    for (int r = 0; r < rounds; ++r) {
        double acc = 0.0;
        auto add = [&](float v) {
            const double c = fmin(fmax((double)v * g, -1.0), 1.0);       // float64 product, then clip (dsp.py:109-110)
            acc = fma(c, c, acc);
        };
        if (g >= BAND_G_LO && g <= BAND_G_HI) {                          // uniform over the grid
            if (cached) {
                int k = lane;
                for (; k + 192 < wave_total; k += 256) {                 // four LDS loads in flight, summed in order
                    const float v0 = mine[k], v1 = mine[k + 64], v2 = mine[k + 128], v3 = mine[k + 192];
                    add(v0), add(v1), add(v2), add(v3);
                }
                for (; k < wave_total; k += 64) add(mine[k]);
            } else {
                for (int c = 0; c < nch; ++c) {
                    const BandChunk bc = band_chunk(a.band, a.piece, a.chunks, d, ch0 + c);
                    const float* list = bc.lists + wave * bc.wave_cap;
                    const int n = __shfl(my_count, c, 64);
                    for (int k = lane; k < n; k += 64) add(list[k]);
                }
            }
            if (threadIdx.x == 0) acc += g * g * closed_a + closed_c;
        } else {
            for (int c = 0; c < nch; ++c) {
                const BandChunk bc = band_chunk(a.band, a.piece, a.chunks, d, ch0 + c);
                for (long long i = bc.b + threadIdx.x; i < bc.e; i += 256) add(a.mid[i]);
            }
        }
        const double s = block_sum<256>(acc, red);
        TAIL_STAMP(3 + 6 * r);
        // The partial sum is published as an 8-byte word whose value is the flag (a sum of squares is never the
        // all-ones pattern round 0 left there); the deciding workgroup polls the words, one lane per word.  An
        // arrival counter cost each round the publisher's wait for its store, the atomic's round trip (a hundred
        // of them on one word take a microsecond) and the last arriver's read of the partials.
        unsigned long long* words = a.tail_gains + a.tail_rounds + 1 + (size_t)r * total;
        const bool last_round = r == rounds - 1;
        if (threadIdx.x == 0) {
            if (last_round && final_peaks) {                             // the peak word first, and landed
                __hip_atomic_store(peak_words + blockIdx.x, (double)my_peak, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __hip_atomic_store(words + blockIdx.x, double_bits(s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        TAIL_STAMP(5 + 6 * r);
        if (last_round) break;
        if (threadIdx.x == 0) gain_now = bits_double(poll_word(a.tail_gains + r, a.error, double_bits(1.0)));
        __syncthreads();
        g = gain_now;
        __syncthreads();
        TAIL_STAMP(8 + 6 * r);
    }
}

__device__ void correction_reset(CorrectionState* cs, double gain) {
    cs->gain = gain;
    cs->steps_done = 0;
    cs->result_peak = 0.0;
    cs->normalize_c = 1.0;
    cs->limiter_active = 1;
    for (int i = 0; i < 16; ++i) cs->coeffs[i] = 0.0;
}
__global__ void k_correction_init(CorrectionState* cs, double gain) {
    if (blockIdx.x == 0 && threadIdx.x == 0) correction_reset(cs, gain);
}

// peak of the corrected result, limiter early-out decision (hyrax.py:83-85 with numpy.isclose
// defaults) and the normalisation coefficient of stages.py:186-191 / dsp.py:93-100
// `front_cs`: a master call without correction rounds, whose BackState this launch fills as round 0 would
// (back_state_fill): *front_cs -> *cs, the reference's two scalars -> back_refs[0], [1].  Null: *cs is the caller's.
__global__ __launch_bounds__(256) void k_finalize_scalars(const float* block_peak, long long nblocks,
                                                          double threshold, double eps, CorrectionState* cs,
                                                          const CorrectionState* front_cs, const double* front_match_rms,
                                                          const double* front_amplitude_c, double* back_refs) {
    __shared__ float scratch[4];
    float m = 0.f;
    for (long long i = threadIdx.x; i < nblocks; i += 256) m = fmaxf(m, block_peak[i]);
    const float pk = block_max<256>(m, scratch);
    if (threadIdx.x == 0) {
        if (front_cs) {
            *cs = *front_cs;
            back_refs[0] = *front_match_rms;
            back_refs[1] = *front_amplitude_c;
        }
        const double peak = (double)(float)((double)pk * cs->gain);      // max |float32(y*gain)|
        cs->result_peak = peak;
        const double rect = fmax(peak, threshold) / threshold;
        cs->limiter_active = fabs(rect - 1.0) > (1e-8 + 1e-5) ? 1 : 0;
        cs->normalize_c = fmax(eps, peak / threshold);
    }
}

}  // namespace mgx
