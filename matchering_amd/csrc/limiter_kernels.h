// The limiter's kernels (device only).  limiter_kernel.h and limiter_general.h hold the phase functions, which the CPU
// emulation drives too; here are the affine scans across a wave and a workgroup, one chunk of the first-order limiter
// (limit_chunk, limit_chunk_quiet) and of the order-K one (limit_chunk_general), and the __global__ kernels k_limit
// and k_limit_general.  MGX_DEV_LIMITER_PHASES builds record where a chunk's time goes (tools/limiter_phases.py).
#pragma once

#include "limiter_general.h"
#include "wave_util.h"

namespace mgx {

// ---------------------------------------------------------------------------
// limiter (limiter_kernel.h): one launch, grid = chunks
// ---------------------------------------------------------------------------
// Ordered composition of affine maps across a workgroup: inclusive scan over the 64 lanes of each
// wave by shuffles (scan order = lane order, or reversed), wave totals through LDS, then every
// thread composes the totals of the waves before it.  Returns the composition of all maps BEFORE
// this thread in scan order; `*whole` (if wanted) the composition of everything.
template <bool REVERSE>
__device__ __forceinline__ Affine wave_inclusive(Affine m) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        Affine o;
        o.a = REVERSE ? __shfl_down(m.a, d, 64) : __shfl_up(m.a, d, 64);
        o.b = REVERSE ? __shfl_down(m.b, d, 64) : __shfl_up(m.b, d, 64);
        const bool has = REVERSE ? (lane + d < 64) : (lane >= d);
        if (has) m = affine_then(o, m);
    }
    return m;
}
template <bool REVERSE>
__device__ __forceinline__ Affine wave_exclusive(Affine inclusive) {
    const int lane = threadIdx.x & 63;
    Affine o;
    o.a = REVERSE ? __shfl_down(inclusive.a, 1, 64) : __shfl_up(inclusive.a, 1, 64);
    o.b = REVERSE ? __shfl_down(inclusive.b, 1, 64) : __shfl_up(inclusive.b, 1, 64);
    const bool first = REVERSE ? lane == 63 : lane == 0;
    return first ? affine_identity() : o;
}
// totals[w] = inclusive total of wave w (written by the caller before the barrier)
template <bool REVERSE, int WAVES>
__device__ __forceinline__ Affine compose_waves(const Affine* totals, Affine exclusive_in_wave, Affine* whole) {
    const int w = threadIdx.x >> 6;
    Affine before = affine_identity(), all = affine_identity();
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
        const int k = REVERSE ? WAVES - 1 - i : i;           // waves in scan order
        const Affine t = totals[k];
        const bool earlier = REVERSE ? k > w : k < w;
        if (earlier) before = affine_then(before, t);
        all = affine_then(all, t);
    }
    if (whole) *whole = all;
    return affine_then(before, exclusive_in_wave);
}

// maximum over the eight lanes that share lane >> 3 (non-negative values): three DPP steps
__device__ __forceinline__ float dpp_max8(float v) {
    // (integer maxima of the bit patterns: the values are non-negative, pmax in mgx_hd.h)
    int x = __float_as_int(v);
    x = max(x, __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    x = max(x, __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    x = max(x, __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true));   // row_half_mirror
    return __int_as_float(x);
}

#ifdef MGX_DEV_LIMITER_PHASES      // development builds only: where a chunk's time goes (tools/limiter_phases.py)
constexpr int DEV_PHASE_CHUNKS = 16384;
__device__ unsigned mgx_dev_phase_ticks[DEV_PHASE_CHUNKS][16];       // [chunk][mark]: ticks since the previous mark; [15] = start time
// every chunk's life, quiet ones included: {kernel entry, frames loaded, end, kind (0 edge, 1 busy, 2 quiet) | cu << 8 | xcc << 20}
__device__ long long mgx_dev_chunk_life[DEV_PHASE_CHUNKS][8];    // [4] hold word out, [5] hold carry in, [6] release word out, [7] release carry in
#define DEV_LIFE(slot, value)                                                                        \
    do {                                                                                             \
        if (threadIdx.x == 0 && chunk < DEV_PHASE_CHUNKS) mgx_dev_chunk_life[chunk][slot] = (value); \
    } while (0)
#define DEV_MARK(k)                                                                                  \
    do {                                                                                             \
        if (threadIdx.x == 0 && chunk < DEV_PHASE_CHUNKS) {                                          \
            const long long now = wall_clock64();                                                    \
            mgx_dev_phase_ticks[chunk][k] = (unsigned)(now - dev_last);                              \
            dev_last = now;                                                                          \
        }                                                                                            \
    } while (0)
#else
#define DEV_MARK(k)
#define DEV_LIFE(slot, value)
#endif
// one chunk, from the load phase to the store; FULL = the chunk lies strictly inside the track
template <int T, bool FULL>
__device__ __forceinline__ void limit_chunk(const LimiterArgs& a, long long chunk, float* lds) {
    using LB = LimiterBlock<T>;
    // (opaque: nothing derived from the thread id may be hoisted out of a persistent caller's loop)
    const int tid = opaque((int)threadIdx.x), lane = tid & 63, wave = tid >> 6;
#ifdef MGX_DEV_LIMITER_PHASES
    long long dev_last = wall_clock64();
    if (threadIdx.x == 0 && chunk < DEV_PHASE_CHUNKS) mgx_dev_phase_ticks[chunk][15] = (unsigned)dev_last;
#endif
    if (!FULL) {                                 // (a FULL chunk was loaded by the kernel: limit_chunk_quiet's frames)
        float pm[LB::E / 2];
        LB::template phase_load<FULL>(opaque(tid), chunk, a, lds, pm);
#pragma unroll
        for (int j = 0; j < LB::E / 2; ++j) {
            const float m = dpp_max8(pm[j]);
            if ((tid & 7) == 0) LB::block_max(lds)[LB::block_of(tid, j)] = m;
        }
        __syncthreads();
    }
    DEV_MARK(0);      // load

    // hold filter first (scan 1): its aggregate is published as early as possible
    typename LB::Thread th;
    Affine whole;
    const bool busy = __any(LB::neighbourhood_max(opaque(tid), a, lds) > 0.f) != 0;      // wave-uniform
    {
        const Affine m1 = LB::template phase_hold_window<FULL>(opaque(tid), chunk, a, th, lds, busy);
        const Affine i1 = wave_inclusive<false>(m1);
        if (lane == 63) LB::wave_totals(lds, 1)[wave] = i1;
        const Affine e1 = wave_exclusive<false>(i1);
        __syncthreads();
        th.hold_pre = compose_waves<false, LB::WAVES>(LB::wave_totals(lds, 1), e1, &whole);
    }
    DEV_MARK(1);      // hold window + scan
    if (tid == 0) LB::lookback_publish(chunk, 0, a, whole.b);
    DEV_LIFE(4, wall_clock64());
    // ask for the predecessors' words now, take them after the attack path (wave 0: hold, wave 1: attack)
    typename LB::Polls polls;
    if (wave == 0) LB::lookback_ask(lane, chunk, 0, a, polls);
    // forward attack smoother (scan 0)
    Affine p0;
    {
        const Affine m0 = LB::template phase_attack_window<FULL>(opaque(tid), a, th, lds, busy);
        const Affine i0 = wave_inclusive<false>(m0);
        if (lane == 63) LB::wave_totals(lds, 0)[wave] = i0;
        const Affine e0 = wave_exclusive<false>(i0);
        __syncthreads();
        p0 = compose_waves<false, LB::WAVES>(LB::wave_totals(lds, 0), e0, nullptr);
    }
    DEV_MARK(2);      // attack window + scan
    if (tid == LB::T - a.gr) LB::lookback_publish(chunk, 2, a, p0.b);          // attack state at the end of the core
    if (wave == 1) LB::lookback_ask(lane, chunk, 2, a, polls);
    const bool tail = !FULL && LB::tail_chunk(chunk, a);                        // uniform
    double att_now = 0.0;
    if (tail) {
        if (wave == 1) {
            const double s = wave_sum(LB::lookback_take(lane, chunk, 2, a, polls));
            if (lane == 0) LB::scalars(lds)[2] = s;
        }
        __syncthreads();
        att_now = LB::scalars(lds)[2];
    }

    // backward attack smoother, right to left (scan 2)
    const Affine mb = LB::template phase_attack_forward<FULL>(opaque(tid), a, th, p0, att_now, lds);
    const Affine ib = wave_inclusive<true>(mb);
    if (lane == 0) LB::wave_totals(lds, 2)[wave] = ib;
    const Affine eb = wave_exclusive<true>(ib);
    __syncthreads();
    const Affine pb = compose_waves<true, LB::WAVES>(LB::wave_totals(lds, 2), eb, nullptr);
    LB::template phase_attack_backward<FULL>(opaque(tid), a, th, pb);
    DEV_MARK(3);      // attack forward, scan, backward
    if (wave == 0) {
        const double s = wave_sum(LB::lookback_take(lane, chunk, 0, a, polls));
        if (lane == 0) LB::scalars(lds)[0] = s;
    }
    if (wave == 1 && !tail) {
        const double s = wave_sum(LB::lookback_take(lane, chunk, 2, a, polls));
        if (lane == 0) LB::scalars(lds)[2] = s;
    }
    DEV_MARK(4);      // take hold (wave 0)
    DEV_LIFE(5, wall_clock64());
    __syncthreads();
    DEV_MARK(5);      // barrier after the takes (waits for wave 1's attack take)

    // hold output, release filter (scan 3)
    const Affine mr = LB::template phase_hold<FULL>(opaque(tid), a, th, LB::scalars(lds)[0], tail ? 0.0 : LB::scalars(lds)[2]);
    const Affine ir = wave_inclusive<false>(mr);
    if (lane == 63) LB::wave_totals(lds, 3)[wave] = ir;
    const Affine er = wave_exclusive<false>(ir);
    __syncthreads();
    const Affine pr = compose_waves<false, LB::WAVES>(LB::wave_totals(lds, 3), er, &whole);
    DEV_MARK(6);      // hold output + release scan
    if (tid == 0) LB::lookback_publish(chunk, 1, a, whole.b);
    DEV_LIFE(6, wall_clock64());
    if (wave == 0) LB::lookback_ask(lane, chunk, 1, a, polls);
    typename LB::Reload again;
    if (FULL) LB::phase_reload(opaque(tid), chunk, a, again);
    DEV_MARK(7);      // publish, ask, reload issue
    if (wave == 0) {
        const double s = wave_sum(LB::lookback_take(lane, chunk, 1, a, polls));
        if (lane == 0) LB::scalars(lds)[1] = s;
    }
    DEV_MARK(8);      // take release
    DEV_LIFE(7, wall_clock64());
    __syncthreads();
    LB::template phase_gain<FULL>(opaque(tid), a, th, pr, LB::scalars(lds)[1], lds);
    __syncthreads();
    DEV_MARK(9);      // gain
    if (FULL) LB::phase_store_reloaded(opaque(tid), chunk, a, again, lds);
    else LB::template phase_store<FULL>(opaque(tid), chunk, a, true, lds);
    DEV_MARK(10);     // store
}

// A chunk without a single frame above the threshold (limiter_kernel.h, "quiet chunks"): two look-backs, no
// windows, no scans, no reload.  45 % of the chunks of the benchmark's 8-minute pair; none of a track that is
// limited everywhere.
template <int T>
__device__ __forceinline__ void limit_chunk_quiet(const LimiterArgs& a, long long chunk, float* lds,
                                                  const typename LimiterBlock<T>::Reload& kept) {
    using LB = LimiterBlock<T>;
    const int tid = opaque((int)threadIdx.x), lane = tid & 63, wave = tid >> 6;
    if (tid == 0) {
        LB::lookback_publish(chunk, 0, a, 0.0);
        LB::lookback_publish(chunk, 2, a, 0.0);
    }
    DEV_LIFE(4, wall_clock64());
    typename LB::Polls polls;
    if (wave == 0) {
        LB::lookback_ask(lane, chunk, 0, a, polls);
        const double s = wave_sum(LB::lookback_take(lane, chunk, 0, a, polls));
        if (lane == 0) LB::scalars(lds)[0] = s;
    }
    if (wave == 1) {
        LB::lookback_ask(lane, chunk, 2, a, polls);
        const double s = wave_sum(LB::lookback_take(lane, chunk, 2, a, polls));
        if (lane == 0) LB::scalars(lds)[2] = s;
    }
    __syncthreads();
    const double hc = LB::scalars(lds)[0], ac = LB::scalars(lds)[2];
    DEV_LIFE(5, wall_clock64());
    if (tid == 0) LB::lookback_publish(chunk, 1, a, hc * a.quiet_rel_gain);
    DEV_LIFE(6, wall_clock64());
    if (wave == 0) {
        LB::lookback_ask(lane, chunk, 1, a, polls);
        const double s = wave_sum(LB::lookback_take(lane, chunk, 1, a, polls));
        if (lane == 0) LB::scalars(lds)[1] = s;
    }
    __syncthreads();
    DEV_LIFE(7, wall_clock64());
    LB::phase_quiet_store(tid, chunk, a, kept, hc, ac, LB::scalars(lds)[1]);
}

// One chunk with hold / release filters of order up to K (limiter_general.h): the load, window, attack and
// store phases of the first-order kernel; the two low-passes as K-state maps scanned through LDS.
template <int K>
__device__ __forceinline__ void limit_chunk_general(const LimiterArgs& a, const GeneralArgs<K>& g, long long chunk, float* lds) {
    using LB = LimiterBlock<256>;
    using LG = LimiterGeneral<K>;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        float pm[LB::E / 2];
        LB::template phase_load<false>(tid, chunk, a, lds, pm);
#pragma unroll
        for (int j = 0; j < LB::E / 2; ++j) {
            const float m = dpp_max8(pm[j]);
            if ((tid & 7) == 0) LB::block_max(lds)[LB::block_of(tid, j)] = m;
        }
    }
    __syncthreads();
    typename LB::Thread th;
    LB::template phase_hold_window<false>(tid, chunk, a, th, lds);          // (its first-order map is not used)
    LG::scan_put(lds, tid, th.core && th.valid > 0 ? LG::block_map(g.hold, th.sh, th.valid, g.pow_hold) : LG::identity());
    __syncthreads();
    LG::scan_groups(lds, tid);
    __syncthreads();
    LG::scan_top(lds, tid);
    __syncthreads();
    const StateMap<K> hold_pre = LG::scan_prefix(lds, tid);
    if (tid == 0) LG::publish(g, a.nchunks, 0, chunk, LG::scan_whole(lds).v);

    // the attack path, as in limit_chunk
    typename LB::Polls polls;
    Affine p0;
    {
        const Affine m0 = LB::template phase_attack_window<false>(tid, a, th, lds);
        const Affine i0 = wave_inclusive<false>(m0);
        if (lane == 63) LB::wave_totals(lds, 0)[wave] = i0;
        const Affine e0 = wave_exclusive<false>(i0);
        __syncthreads();
        p0 = compose_waves<false, LB::WAVES>(LB::wave_totals(lds, 0), e0, nullptr);
    }
    if (tid == LB::T - a.gr) LB::lookback_publish(chunk, 2, a, p0.b);
    if (wave == 1) LB::lookback_ask(lane, chunk, 2, a, polls);
    const bool tail = LB::tail_chunk(chunk, a);
    double att_now = 0.0;
    if (tail) {
        if (wave == 1) {
            const double s = wave_sum(LB::lookback_take(lane, chunk, 2, a, polls));
            if (lane == 0) LB::scalars(lds)[2] = s;
        }
        __syncthreads();
        att_now = LB::scalars(lds)[2];
    }
    const Affine mb = LB::template phase_attack_forward<false>(tid, a, th, p0, att_now, lds);
    const Affine ib = wave_inclusive<true>(mb);
    if (lane == 0) LB::wave_totals(lds, 2)[wave] = ib;
    const Affine eb = wave_exclusive<true>(ib);
    __syncthreads();
    const Affine pb = compose_waves<true, LB::WAVES>(LB::wave_totals(lds, 2), eb, nullptr);
    LB::template phase_attack_backward<false>(tid, a, th, pb);

    // carries of the hold filter (wave 0) and of the attack smoother (wave 1)
    double* carries = LG::carries(lds);
    if (wave == 0) {
        double acc[K];
        LG::take(lane, chunk, 0, g, a, acc);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double s = wave_sum(acc[k]);
            if (lane == 0) carries[k] = s;
        }
    }
    if (wave == 1 && !tail) {
        const double s = wave_sum(LB::lookback_take(lane, chunk, 2, a, polls));
        if (lane == 0) LB::scalars(lds)[2] = s;
    }
    __syncthreads();
    double hold_carry[K];
#pragma unroll
    for (int k = 0; k < K; ++k) hold_carry[k] = carries[k];
    const StateMap<K> mr = LG::phase_hold(tid, a, g, th, hold_pre, hold_carry, tail ? 0.0 : LB::scalars(lds)[2]);
    __syncthreads();                                                          // every prefix of the hold scan has been read
    LG::scan_put(lds, tid, mr);
    __syncthreads();
    LG::scan_groups(lds, tid);
    __syncthreads();
    LG::scan_top(lds, tid);
    __syncthreads();
    const StateMap<K> rel_pre = LG::scan_prefix(lds, tid);
    if (tid == 0) LG::publish(g, a.nchunks, 1, chunk, LG::scan_whole(lds).v);
    if (wave == 0) {
        double acc[K];
        LG::take(lane, chunk, 1, g, a, acc);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double s = wave_sum(acc[k]);
            if (lane == 0) carries[K + k] = s;
        }
    }
    __syncthreads();
    double rel_carry[K];
#pragma unroll
    for (int k = 0; k < K; ++k) rel_carry[k] = carries[K + k];
    LG::phase_gain(tid, g, th, rel_pre, rel_carry, lds);
    __syncthreads();
    LB::template phase_store<false>(tid, chunk, a, true, lds);
}

template <int K>
__global__ __launch_bounds__(256, 2) void k_limit_general(LimiterArgs a, GeneralArgs<K> g) {
    using LB = LimiterBlock<256>;
    MGX_LDS;
    float* lds = reinterpret_cast<float*>(mgx_smem);
    int& ticket = *reinterpret_cast<int*>(LB::scalars(lds) + 4);
    const bool active = a.active ? (*a.active != 0) : true;
    if (!active) {                       // hyrax.py:83-85
        LB::phase_store(threadIdx.x, blockIdx.x, a, false, lds);
        return;
    }
    long long chunk = blockIdx.x;            // (the workgroup's number, or a ticket: see k_limit)
    if (a.ticket) {
        if (threadIdx.x == 0) ticket = atomicAdd(a.ticket, 1);
        __syncthreads();
        chunk = ticket;
    }
    limit_chunk_general<K>(a, g, chunk, lds);
}

// T = threads = 16-frame blocks per chunk (256, or 1024 for long attack / hold times); WGS = workgroups
// per CU the kernel is compiled for (register budget 512 / (WGS * T / 256) per lane)
// HW / HB / GR >= 0: an instantiation for ONE window geometry (attack half window, hold look-back, right halo blocks;
// gl and gw follow from them): the bounds of every window loop are literals, the masked ragged-edge reads of the
// general form fold away and the code is a third shorter.  The host launches it when the configuration's numbers are
// exactly these (44.1 and 48 kHz with the reference's default 1 ms attack and hold, defaults.py:25-58), the general
// instantiation (-1) otherwise; the results are the same to the bit.
template <int T, int WGS, int HW = -1, int HB = -1, int GR = -1>
__global__ __launch_bounds__(T, WGS * T / 256) void k_limit(LimiterArgs a0) {
    warm_code(CODE_LIMIT, T == 256 ? 0 : 1);
    using LB = LimiterBlock<T>;
    LimiterArgs a = a0;
    if (HW >= 0) {
        a.hw = HW;
        a.hb = HB;
        a.gl = (HW + HB + LB::E - 1) / LB::E;
        a.gw = (HW + LB::E - 1) / LB::E;
        a.gr = GR;
    }
    MGX_LDS;
    float* lds = reinterpret_cast<float*>(mgx_smem);
    int& ticket = *reinterpret_cast<int*>(LB::scalars(lds) + 4);      // dynamic LDS only (16-byte aligned base)
    const int tid = threadIdx.x;
    const bool active = a.active ? (*a.active != 0) : true;
    if (!active) {                       // hyrax.py:83-85: the array passes through, then stages.py:203
        LB::phase_store(tid, blockIdx.x, a, false, lds);
        return;
    }
#ifdef MGX_DEV_LIMITER_PHASES
    const long long dev_entry = wall_clock64();
#endif
    // Which chunk?  The workgroup's own number.  A chunk waits for words of LOWER-numbered chunks only, and the
    // dispatcher walks a grid in the order of the workgroup numbers (the walk may stall on an XCD whose slots are all
    // taken, but whatever it has handed out is lower-numbered than what it has not): the lowest unfinished chunk has
    // always been handed out, all it waits for is finished, so it finishes -- no chunk can wait for ever.  An atomic
    // ticket (a.ticket != null) gives the same guarantee without leaning on the dispatch order, at the price of a
    // returning atomic and a barrier in front of every chunk's loads (entry to loaded 6.2 -> 3.3 us, the kernel
    // 152 -> 134 us: profiles/r05_g_*); a handle falls back to it if a bounded look-back wait ever expires.
    long long chunk = blockIdx.x;
    if (a.ticket) {
        if (tid == 0) ticket = atomicAdd(a.ticket, 1);
        __syncthreads();
        chunk = ticket;
    }
    DEV_LIFE(0, dev_entry);
    if (!LB::full_chunk(chunk, a)) {
        limit_chunk<T, false>(a, chunk, lds);
        DEV_LIFE(2, wall_clock64());
        DEV_LIFE(3, 0ll | ((long long)__builtin_amdgcn_s_getreg((4 << 11) | 4) << 8));
        return;
    }
    // a chunk inside the track: load (the frames stay in registers until it is known whether the chunk is
    // quiet), block maxima, one flag per wave
    typename LB::Reload kept;
    {
        float pm[LB::E / 2];
        LB::phase_load_full(opaque(tid), chunk, a, lds, pm, kept);
        float mine = 0.f;
#pragma unroll
        for (int j = 0; j < LB::E / 2; ++j) {
            mine = fmaxf(mine, pm[j]);
            const float m = dpp_max8(pm[j]);
            if ((tid & 7) == 0) LB::block_max(lds)[LB::block_of(tid, j)] = m;
        }
        const bool wave_busy = __any(mine > 0.f) != 0;
        if ((tid & 63) == 0) LB::edge_sl(lds)[tid >> 6] = wave_busy ? 1.f : 0.f;   // (16 floats; the track's ends use them, not these chunks)
    }
    __syncthreads();
    bool chunk_busy = false;
#pragma unroll
    for (int w = 0; w < LB::WAVES; ++w) chunk_busy = chunk_busy || LB::edge_sl(lds)[w] != 0.f;
    DEV_LIFE(1, wall_clock64());
    if (!chunk_busy && a.quiet_ok) limit_chunk_quiet<T>(a, chunk, lds, kept);
    else limit_chunk<T, true>(a, chunk, lds);
    DEV_LIFE(2, wall_clock64());
    // HW_ID (hwreg 4): cu_id bits 11:8, sh 12, se 15:13; XCC_ID (hwreg 20)
    DEV_LIFE(3, (long long)((!chunk_busy && a.quiet_ok) ? 2 : 1) | ((long long)__builtin_amdgcn_s_getreg((15 << 11) | 4) << 8) |
                    ((long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32));
}

}  // namespace mgx
