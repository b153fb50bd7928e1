// The library's device code, stage by stage (device only; included by mgx.hip, the one translation unit).
//
// This file itself holds the __global__ wrappers around the convolution and analysis phase functions
// (conv2_kernel.h, conv_delay_kernel.h, conv_wide_kernel.h, analysis2_kernel.h): k_conv*, k_conv*_prep and
// k_analyze*.  The CPU emulation drives those phase functions directly and includes none of the *_kernels.h files.
// The other stages have a header each, included at the end in the order of the master chain.
#pragma once

#include <hip/hip_runtime.h>

#include "analysis2_kernel.h"
#include "conv2_kernel.h"
#include "conv_delay_kernel.h"
#include "conv_wide_kernel.h"
#include "fft2_lanes.h"
#include "small_fft_kernels.h"     // fft_size 8 .. 32
#include "wave_util.h"

namespace mgx {

// ---------------------------------------------------------------------------
// convolution
// ---------------------------------------------------------------------------
template <int LOG2N>
constexpr size_t conv_lds_bytes() {
    // (+ 16 floats for block_max and one int, the next pair's number: see k_conv)
    return ((size_t)Fft2<LOG2N>::LDS_ELEMS + Fft2<LOG2N>::MID_TABLE) * sizeof(float2) + 80;
}

// workgroups of k_conv a CU holds (LDS and thread limits), and the waves per SIMD that makes: the
// register budget the kernel is compiled for
template <int LOG2N>
constexpr int conv_workgroups_per_cu() {
    constexpr int w = workgroups_per_cu(Fft2<LOG2N>::T, conv_lds_bytes<LOG2N>());
    return w > 2 ? 2 : w;                            // more than two co-resident transforms do not pay
}
template <int LOG2N>
constexpr int conv_waves_per_simd() {
    constexpr int w = conv_workgroups_per_cu<LOG2N>() * (Fft2<LOG2N>::T / 64) / 4;
    return w < 2 ? 2 : w;
}

// One channel of one pair, from pass 0 (`pass0`) up to the inverse middle pass (conv2_kernel.h).
template <int LOG2N, bool SIDE, class Pass0>
__device__ __forceinline__ void conv_channel(int tid, const Conv2Args& a, float2* lds, const float2* mid_table,
                                             Pass0 pass0) {
    using CB = Conv2Block<LOG2N>;
    using F = Fft2<LOG2N>;
    typename CB::RowFilter rf;
    pass0();
    // (the scheduler must not lift the filter loads above pass 0: there is no room for them yet)
    __builtin_amdgcn_sched_barrier(0);
    CB::fetch_filter(tid, SIDE ? a.h_side : a.h_mid, rf);      // a phase early: the middle pass hides its latency
    __syncthreads();
    fwd_middle_passes<F, false>(opaque(tid), lds, mid_table);
    CB::phase_filter(tid, rf, lds);
    inv_middle_passes<F, false>(opaque(tid), lds, mid_table);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);      // keeps the next phase's LDS reads from being lifted into this one
}
// uniformly partitioned overlap-save: one forward transform per filter partition, products
// accumulated on the thread's row, one inverse transform
template <int LOG2N, bool SIDE>
__device__ __forceinline__ void conv_channel_partitioned(int tid, long long pair, bool edge, const Conv2Args& a,
                                                         const typename Conv2Block<LOG2N>::Persist& ps,
                                                         float2* lds, const float2* mid_table) {
    using CB = Conv2Block<LOG2N>;
    using F = Fft2<LOG2N>;
    const float2* h = SIDE ? a.h_side : a.h_mid;
    typename CB::RowFilter rf;
    typename CB::RowAcc acc;
    CB::clear_acc(acc);
    // radix-32 middle passes (16384 points) need the registers the early filter fetch would hold
    constexpr bool LATE_FILTER = F::R(1) >= 32;
    for (int k = 0; k < a.parts; ++k) {
        CB::template phase_load<SIDE>(opaque(tid), pair, edge, a, ps, lds, k);
        __builtin_amdgcn_sched_barrier(0);
        if (!LATE_FILTER) CB::fetch_filter(tid, h + (size_t)k * F::N, rf);
        __syncthreads();
        fwd_middle_passes<F, false>(opaque(tid), lds, mid_table);
        __builtin_amdgcn_sched_barrier(0);
        if (LATE_FILTER) CB::fetch_filter(opaque(tid), h + (size_t)k * F::N, rf);
        CB::phase_accumulate(tid, rf, lds, acc);
        __syncthreads();                    // (the next partition's pass 0 writes everywhere)
        __builtin_amdgcn_sched_barrier(0);
    }
    CB::phase_finish_row(tid, acc, lds);
    __builtin_amdgcn_sched_barrier(0);
    inv_middle_passes<F, false>(opaque(tid), lds, mid_table);
    __syncthreads();
}

// One pair of output blocks: mid channel, then side channel + epilogue.
// (Issuing the NEXT pair's frame loads before the epilogue's stores -- software pipelining -- was
// built and measured: the 48-96 registers in flight make the 8192-point kernel spill at the 256 a
// wave has here, and a spilling kernel is far slower than an unpipelined one, 294 vs 153 us.)
template <int LOG2N, bool MULTI>
__device__ __forceinline__ float conv_pair(int tid, long long pair, const Conv2Args& a,
                                           const typename Conv2Block<LOG2N>::Persist& ps, float2* lds,
                                           const float2* mid_table) {
    using CB = Conv2Block<LOG2N>;
    const bool edge = !CB::interior(pair, a.n, a.parts);
    typename CB::Kept kept;
    if constexpr (MULTI) {
        conv_channel_partitioned<LOG2N, false>(tid, pair, edge, a, ps, lds, mid_table);
        CB::phase_keep_mid(tid, ps, lds, kept);
        __syncthreads();
        conv_channel_partitioned<LOG2N, true>(tid, pair, edge, a, ps, lds, mid_table);
    } else {
        typename CB::Raw raw;
        typename CB::Held held;
        CB::fetch_frames(tid, pair, a, 0, raw);
        conv_channel<LOG2N, false>(
            tid, a, lds, mid_table, [&]() { CB::phase_pass0_mid(tid, raw, ps, lds, held); });
        CB::phase_keep_mid(tid, ps, lds, kept);
        __syncthreads();
        conv_channel<LOG2N, true>(
            tid, a, lds, mid_table, [&]() { CB::phase_pass0_side(tid, held, ps, lds); });
    }
    const float pk = CB::phase_store(tid, pair, edge, a, ps, lds, kept);
    return pk;
}

// Persistent workgroups.  gridDim.x is a multiple of 8; workgroup w is (observed to be) placed on
// XCD w % 8, so XCD x walks its own contiguous eighth of the track and the workgroups resident on
// it work on neighbouring pairs: the overlap between neighbours is re-read from that XCD's L2,
// not from HBM.  Placement only affects speed, never results.
// After its first pair a workgroup takes the next pair of its XCD's range from a counter (asked for at
// the start of a pair, needed at its end) instead of a fixed stride: an 8-minute track is 5.05 pairs
// per workgroup, and with fixed strides the kernel lasted six pair-times for it.
// Two workgroups per CU (LDS): the second launch bound is waves per SIMD, i.e. the register budget.
// MULTI = more than one filter partition (its own instantiation: the accumulator row costs registers
// the plain kernel should not pay for)
template <int LOG2N, bool MULTI>
__global__ __launch_bounds__((Fft2<LOG2N>::T), (conv_waves_per_simd<LOG2N>())) void k_conv(Conv2Args a) {
    warm_code(CODE_CONV, LOG2N);
    using CB = Conv2Block<LOG2N>;
    using F = Fft2<LOG2N>;
    MGX_LDS;
    float2* lds = reinterpret_cast<float2*>(mgx_smem);
    float2* mid_table = lds + F::LDS_ELEMS;
    float* scratch = reinterpret_cast<float*>(mid_table + F::MID_TABLE);
    const int tid = threadIdx.x;
    typename CB::Persist ps;
    CB::load_persist(tid, a.tw, mid_table, ps);
    __syncthreads();
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, slots = gridDim.x >> 3;
    const long long per = (a.npairs + 7) >> 3;
    const long long end = min(a.npairs, (xcd + 1) * per);
    const long long first = xcd * per + slot;
    int* next_slot = reinterpret_cast<int*>(scratch + 16);
    long long pair = first;
    while (pair < end) {
        unsigned ticket = 0;
        if (tid == 0) ticket = atomicAdd(a.queue + xcd, 1u);
        // The pass-0 twiddles stay in registers across pairs, but nothing derived from them (or
        // from the thread id) should: hoisted out of this loop it would sit in VGPRs it does
        // not have.  An empty asm makes the values opaque per iteration.
#pragma unroll
        for (int q = 0; q < F::LB0; ++q) asm volatile("" : "+v"(ps.tw0.b[q].x), "+v"(ps.tw0.b[q].y));
        const float pk = conv_pair<LOG2N, MULTI>(tid, pair, a, ps, lds, mid_table);
        const float bp = block_max<F::T>(pk, scratch);
        if (tid == 0) {
            if (a.pair_peak) a.pair_peak[pair] = bp;
            *next_slot = (int)ticket;
        }
        __syncthreads();
        pair = xcd * per + slots + *next_slot;
    }
    // the last workgroup to run out of pairs leaves the counters at zero for the next launch
    if (tid == 0 && atomicAdd(a.queue + 8, 1u) == gridDim.x - 1) {
        for (int i = 0; i < 9; ++i) a.queue[i] = 0;
    }
}

#ifdef MGX_DEV_CONV_PHASES         // development builds only: where a block's time goes (tools/conv_delay_phases.py)
constexpr int DEV_CONV_BLOCKS = 16384;
__device__ unsigned mgx_dev_conv_ticks[DEV_CONV_BLOCKS][8];          // [block][mark]: ticks since the previous mark; [7] = start
#define DEV_CONV_MARK(k)                                                                             \
    do {                                                                                             \
        if (threadIdx.x == 0 && b >= 0 && b < DEV_CONV_BLOCKS) {                                     \
            const long long now = wall_clock64();                                                    \
            mgx_dev_conv_ticks[b][k] = (unsigned)(now - dev_last);                                   \
            dev_last = now;                                                                          \
        }                                                                                            \
    } while (0)
#else
#define DEV_CONV_MARK(k)
#endif
// A filter of two partitions as a frequency-domain delay line (conv_delay_kernel.h): workgroup w takes blocks
// [w * run, (w + 1) * run) one after the other, the partition-1 product of a block carried to the next in registers;
// it starts with the forward transform of block w * run - 1 (carry only).  a.npairs counts BLOCKS here and
// pair_peak has one entry per block.
template <int LOG2N>
__global__ __launch_bounds__((Fft2<LOG2N>::T), (conv_waves_per_simd<LOG2N>())) void k_conv_delay(Conv2Args a) {
    warm_code(CODE_CONV, CODE_VARIANT_CONV_DELAY);
    using CD = ConvDelay<LOG2N>;
    using CB = Conv2Block<LOG2N>;
    using F = Fft2<LOG2N>;
    MGX_LDS;
    float2* lds = reinterpret_cast<float2*>(mgx_smem);
    float2* mid_table = lds + F::LDS_ELEMS;
    float* scratch = reinterpret_cast<float*>(mid_table + F::MID_TABLE);
    const int tid = threadIdx.x;
    typename CB::Persist ps;
    CB::load_persist(tid, a.tw, mid_table, ps);
    __syncthreads();
    const long long first = (long long)blockIdx.x * a.run;
    const long long end = min(a.npairs, first + a.run);
    typename CD::Carry carry;
    CD::clear(carry);
    // the older half of a block's window is the newer half of the block before: kept in registers (as mid / side),
    // and the newer half is asked for a block ahead -- every frame is fetched once per run and its latency lies under
    // the end of the block before (275 us with the whole window loaded at the top of a block, 262 with the older half
    // kept, 243 with the newer half asked for ahead: profiles/r04_v_conv_delay_pairs.txt)
    typename CD::HeldFrames held;
    typename CD::HalfFrames newer;
    CD::prime(tid, first - 1, a, held);
    CD::template fetch_half<CD::R0 / 2>(tid, first - 1, a, newer);
    for (long long b = first - 1; b < end; ++b) {
        // (as in k_conv: nothing derived from the pass-0 twiddles or the thread id may be hoisted out of the loop)
#pragma unroll
        for (int q = 0; q < F::LB0; ++q) asm volatile("" : "+v"(ps.tw0.b[q].x), "+v"(ps.tw0.b[q].y));
#ifdef MGX_DEV_CONV_PHASES
        long long dev_last = wall_clock64();
        if (threadIdx.x == 0 && b >= 0 && b < DEV_CONV_BLOCKS) mgx_dev_conv_ticks[b][7] = (unsigned)dev_last;
#endif
        CD::phase_pass0_held(opaque(tid), ps, held, newer, lds);       // (the newer half was asked for a block ago)
        lds_barrier();
        DEV_CONV_MARK(0);                   // frames, pass 0, barrier
        fwd_middle_passes<F>(opaque(tid), lds, mid_table);
        __builtin_amdgcn_sched_barrier(0);
        DEV_CONV_MARK(1);                   // middle passes
        CD::phase_row(opaque(tid), lds);
        lds_barrier();
        DEV_CONV_MARK(2);                   // row forward, barrier
        CD::phase_multiply(opaque(tid), a, carry, lds);
        lds_barrier();                    // every mirror row has been read: the rows may be written again
        __builtin_amdgcn_sched_barrier(0);
        DEV_CONV_MARK(3);                   // multiply, barrier
        if (b < first) {                    // (uniform) the block in front of the run: its carry only
            CD::template fetch_half<CD::R0 / 2>(opaque(tid), b + 1, a, newer);
            continue;
        }
        CD::phase_row_back(opaque(tid), lds);
        inv_middle_passes<F>(opaque(tid), lds, mid_table);
        // the newer half of the next block's window: asked for here, its latency under the last inverse pass and the
        // stores (asked for a phase earlier, behind the multiply, it costs 24 B more scratch and 11 us)
        CD::template fetch_half<CD::R0 / 2>(opaque(tid), b + 1, a, newer);
        lds_barrier();                      // (every barrier of the loop orders LDS traffic only: a __syncthreads() would
                                            // wait for these loads, and for the stores below, which nobody here reads)
        DEV_CONV_MARK(4);                   // row back, inverse middle passes, barrier
        const float pk = CD::phase_store(opaque(tid), b, a, ps, lds);
        const float bp = block_max_lds<F::T>(pk, scratch);      // (a barrier inside: the LDS is free for the next block)
        if (tid == 0 && a.pair_peak) a.pair_peak[b] = bp;
        DEV_CONV_MARK(5);                   // inverse pass 0, stores, peak
    }
}

// F taps on N = 4F blocks (conv_wide_kernel.h): every workgroup takes one block per round of the grid and asks for the
// frames of its next block while the current one is in its inverse transform.  a.npairs counts BLOCKS of 3N/4 frames
// here and pair_peak has one entry per block.
// Which block: workgroup w is (observed to be) placed on XCD w % 8.  Round i covers blocks [i G, (i + 1) G) in eight runs
// of G / 8 consecutive blocks, one run per XCD, so that a block and its neighbour -- whose windows share N / 4 frames --
// are fetched through the same L2 (until round 6: blocks w, w + G, ... -- neighbours on different XCDs, the shared quarter
// fetched from HBM twice: FETCH_SIZE 112 MiB x 2 for 169 MB of frames).  Placement affects speed only.
__device__ __forceinline__ long long conv_wide_block(unsigned w, unsigned round, unsigned grid) {
    if ((grid & 7u) == 0) return ((long long)round * 8 + (w & 7u)) * (grid >> 3) + (w >> 3);
    return (long long)round * grid + w;
}
// Which forms of the loop the kernel runs (conv_wide_kernel.h; the earlier form of each stays there as the CPU emulation's
// reference, and an A/B build clears a bit in a copy of this line): the block peak combined behind the NEXT block's
// first barrier, the end-of-track mask behind a last-block branch.  (Two more lost their A/B and are gone, DESIGN.md
// section 3.4: 16-byte global accesses with an exchange between neighbouring lanes, filter tables that hold P and Q.)
constexpr unsigned CONV_WIDE_LATE_PEAK = 2, CONV_WIDE_END_BRANCH = 8;
constexpr unsigned CONV_WIDE_FORMS = CONV_WIDE_LATE_PEAK | CONV_WIDE_END_BRANCH;
// the block peak from the waves' maxima (thread 0; behind a barrier that follows the waves' writes)
template <int THREADS>
__device__ __forceinline__ float combine_wave_peaks(const float* scratch) {
    float r = 0.f;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) r = fmaxf(r, scratch[w]);
    return r;
}
template <int LOG2N>
__global__ __launch_bounds__((Fft2<LOG2N>::T), (conv_waves_per_simd<LOG2N>())) void k_conv_wide(Conv2Args a) {
    warm_code(CODE_CONV, CODE_VARIANT_CONV_WIDE);
    using CW = ConvWide<LOG2N>;
    using CB = Conv2Block<LOG2N>;
    using F = Fft2<LOG2N>;
    constexpr bool LATE_PEAK = (CONV_WIDE_FORMS & CONV_WIDE_LATE_PEAK) != 0, END_BRANCH = (CONV_WIDE_FORMS & CONV_WIDE_END_BRANCH) != 0;
    MGX_LDS;
    float2* lds = reinterpret_cast<float2*>(mgx_smem);
    float2* mid_table = lds + F::LDS_ELEMS;
    float* scratch = reinterpret_cast<float*>(mid_table + F::MID_TABLE);
    const int tid = threadIdx.x;
    typename CB::Persist ps;
    CB::load_persist(tid, a.tw, mid_table, ps);
    typename CW::Frames frames;
    CW::fetch(tid, conv_wide_block(blockIdx.x, 0, gridDim.x), a, frames);
    __syncthreads();
    long long pending = -1;                               // LATE_PEAK: the block whose waves' maxima wait in `scratch`
    for (unsigned round = 0;; ++round) {
        const long long b = conv_wide_block(blockIdx.x, round, gridDim.x);
        if (b >= a.npairs) break;
        // (as in k_conv: nothing derived from the pass-0 twiddles or the thread id may be hoisted out of the loop)
#pragma unroll
        for (int q = 0; q < F::LB0; ++q) asm volatile("" : "+v"(ps.tw0.b[q].x), "+v"(ps.tw0.b[q].y));
#ifdef MGX_DEV_CONV_PHASES
        long long dev_last = wall_clock64();
        if (threadIdx.x == 0 && b < DEV_CONV_BLOCKS) mgx_dev_conv_ticks[b][7] = (unsigned)dev_last;
#endif
        CW::phase_pass0(opaque(tid), ps, frames, lds);
        lds_barrier();
        if (LATE_PEAK && tid == 0 && pending >= 0 && a.pair_peak) a.pair_peak[pending] = combine_wave_peaks<F::T>(scratch);
        DEV_CONV_MARK(0);                   // pass 0, barrier
        fwd_middle_passes<F>(opaque(tid), lds, mid_table);
        __builtin_amdgcn_sched_barrier(0);
        DEV_CONV_MARK(1);                   // middle passes
        typename CW::Filters filt;
        CW::fetch_filters(opaque(tid), a, filt);          // needed behind the next barrier
        typename CW::Kept kept;                           // the own half of the row stays in registers (conv_wide_kernel.h)
        CW::phase_row_keep(opaque(tid), kept, lds);
        lds_barrier();
        DEV_CONV_MARK(2);                   // row forward, barrier
        CW::phase_multiply_keep(opaque(tid), filt, kept, lds);
        lds_barrier();                    // the partner has written this row's upper half
        __builtin_amdgcn_sched_barrier(0);
        DEV_CONV_MARK(3);                   // multiply, barrier
        CW::phase_row_back_keep(opaque(tid), kept, lds);
        inv_middle_passes<F>(opaque(tid), lds, mid_table);
        // the next block's window: its latency under the last inverse pass and the stores -- the barriers from here
        // to the top of the loop order LDS traffic only (a __syncthreads() would wait for these loads)
        CW::fetch(opaque(tid), conv_wide_block(blockIdx.x, round + 1, gridDim.x), a, frames);
        lds_barrier();
        DEV_CONV_MARK(4);                   // row back, inverse middle passes, barrier
        const float pk = CW::template phase_store<END_BRANCH>(opaque(tid), b, a, ps, lds);
        if constexpr (LATE_PEAK) {
            // No barrier between this phase and the next block's pass 0.  None is needed for the transform: the
            // inverse pass 0 above read LDS positions base<0>(tid) + off<0>(q), and the forward pass 0 of the next
            // block writes exactly those -- the thread's own (one pass-0 butterfly per thread).  The barrier that
            // stood here served the peak alone and kept sixteen waves in lock step across two phases that mix memory,
            // VALU and LDS work.  The waves' maxima wait in `scratch`; thread 0 combines them behind the barrier that
            // follows the next pass 0 (or the loop), and the waves write the next block's only behind three more.
            static_assert(F::CNT(0) == 1, "a thread's inverse pass 0 reads what its own forward pass 0 writes, nothing else");
            const float wave_peak = wave_max(pk);
            if ((tid & 63) == 0) scratch[tid >> 6] = wave_peak;
            pending = b;
        } else {
            const float bp = block_max_lds<F::T>(pk, scratch);      // (a barrier inside: the LDS is free for the next block)
            if (tid == 0 && a.pair_peak) a.pair_peak[b] = bp;
        }
        DEV_CONV_MARK(5);                   // inverse pass 0, stores, peak
    }
    if (LATE_PEAK && pending >= 0) {                      // (uniform) the last block's peak
        lds_barrier();
        if (tid == 0 && a.pair_peak) a.pair_peak[pending] = combine_wave_peaks<F::T>(scratch);
    }
}
// its filter spectra: grid = 2 (mid, side); taps = [2][N/4] float
template <int LOG2N>
__global__ __launch_bounds__((Fft2<LOG2N>::T)) void k_conv_wide_prep(const float* taps, const float2* tw, float2* tables,
                                                                   const double* gain_ptr, double gain) {
    warm_code(CODE_CONV_PREP, CODE_VARIANT_CONV_WIDE);
    using CW = ConvWide<LOG2N>;
    using CB = Conv2Block<LOG2N>;
    using F = Fft2<LOG2N>;
    MGX_LDS;
    float2* lds = reinterpret_cast<float2*>(mgx_smem);
    float2* mid_table = lds + F::LDS_ELEMS;
    const int tid = threadIdx.x, ch = blockIdx.x;
    const double g = gain_ptr ? *gain_ptr * gain : gain;
    typename CB::Persist ps;
    CB::load_persist(tid, tw, mid_table, ps);
    CW::phase_load_taps(tid, taps + (size_t)ch * CW::TAPS, ps, lds);
    __syncthreads();
    fwd_middle_passes<F>(tid, lds, mid_table);
    CB::phase_write_filter(tid, lds, (float)(g / (double)F::N), tables + (size_t)ch * F::N);
}

// filter spectra: grid = 2 * parts; taps = [2][parts * N/2] float (mid then side), tables =
// [2][parts][N] float2.  Workgroup (ch, k) transforms partition k of channel ch.
template <int LOG2N>
__global__ __launch_bounds__((Fft2<LOG2N>::T)) void k_conv_prep(const float* taps, const float2* tw, float2* tables,
                                                              int parts, const double* gain_ptr, double gain) {
    warm_code(CODE_CONV_PREP, LOG2N);
    using CB = Conv2Block<LOG2N>;
    using F = Fft2<LOG2N>;
    MGX_LDS;
    float2* lds = reinterpret_cast<float2*>(mgx_smem);
    float2* mid_table = lds + F::LDS_ELEMS;
    const int tid = threadIdx.x, ch = blockIdx.x / parts, k = blockIdx.x % parts;
    const double g = gain_ptr ? *gain_ptr * gain : gain;      // asked for first: nothing below should wait for it
    typename CB::Persist ps;
    CB::load_persist(tid, tw, mid_table, ps);
    CB::phase_load_taps(tid, taps + ((size_t)ch * parts + k) * CB::TAPS, ps, lds);
    __syncthreads();
    fwd_middle_passes<F>(tid, lds, mid_table);
    CB::phase_write_filter(tid, lds, (float)(g / (double)F::N), tables + ((size_t)ch * parts + k) * F::N);
}

// ---------------------------------------------------------------------------
// analysis
// ---------------------------------------------------------------------------
template <int LOG2N>
constexpr size_t analysis_lds_bytes() {
    // (+ a double and a float of reduction scratch per wave of the workgroup)
    return ((size_t)Fft2<LOG2N>::LDS_ELEMS + Fft2<LOG2N>::MID_TABLE) * sizeof(float2) + (Fft2<LOG2N>::T / 64) * 12;
}

// waves per SIMD the LDS footprint admits (4 SIMDs per CU): the register budget follows from it
constexpr int ANALYZE_MAX_WGS = 8;      // workgroups per CU at most (host: analysis_workgroups_per_cu)
template <int LOG2N>
constexpr int analysis_waves_per_simd() {
    constexpr int fit = workgroups_per_cu(Fft2<LOG2N>::T, analysis_lds_bytes<LOG2N>());
    constexpr int wgs = fit < ANALYZE_MAX_WGS ? fit : ANALYZE_MAX_WGS;
    constexpr int w = wgs * (Fft2<LOG2N>::T / 64) / 4;
    return w < 1 ? 1 : (w > 8 ? 8 : w);
}

// One grid for one or two tracks: workgroups [0, nwg0) belong to `a0`, the rest to `a1` (target and
// reference of a pair in ONE launch: no boundary and no half-empty chip between the two passes).
template <int LOG2N>
__global__ __launch_bounds__(Fft2<LOG2N>::T, analysis_waves_per_simd<LOG2N>()) void k_analyze(AnalysisArgs a0, AnalysisArgs a1,
                                                                                             int nwg0) {
    warm_code(CODE_ANALYZE, LOG2N);
    using AB = Analysis2Block<LOG2N>;
    using F = Fft2<LOG2N>;
    MGX_LDS;
    float2* lds = reinterpret_cast<float2*>(mgx_smem);
    float2* mid_table = lds + F::LDS_ELEMS;
    double* dscratch = reinterpret_cast<double*>(mid_table + F::MID_TABLE);
    float* fscratch = reinterpret_cast<float*>(dscratch + F::T / 64);   // (one slot per wave each)
    const bool second = (int)blockIdx.x >= nwg0;                 // uniform
    const AnalysisArgs& a = second ? a1 : a0;
    const int tid = threadIdx.x, wg = second ? blockIdx.x - nwg0 : blockIdx.x;
    const int d = wg / a.chunks_per_piece, ch = wg % a.chunks_per_piece;
    typename AB::Thread th;
    AB::init(th);
    typename AB::Persist ps;
    AB::load_persist(tid, a.tw, mid_table, ps);
    __syncthreads();
    int s0, s1;
    AB::chunk_segments(a, ch, s0, s1);
    constexpr bool AHEAD = LOG2N == 14;
    typename AB::Raw raw;
    if (AHEAD) AB::fetch(tid, (long long)d * a.piece + (long long)s0 * F::N, a, raw);
    for (int s = s0; s < s1; ++s) {
        // (A software prefetch of the next segment, round 4: asked for after pass 0, after the middle pass or after
        // the row pass, with the thread id opaque per iteration so that nothing is hoisted -- at 128 VGPRs every
        // variant spills (116 - 172 B: the kernel sits at 124 registers without it) and the spilling kernel ran 152 us;
        // at three workgroups per CU and 168 VGPRs it fits without scratch and changes nothing: 100 us with and
        // without it, against 92 us for four workgroups without.  Hiding the loads is worth exactly the fourth
        // workgroup it costs.  profiles/r04_b_ab_variants.txt.  Round 5: one word of each 128-byte line of the next
        // segment asked for behind this segment's loads (one register, no scratch at 16384 points) so that the L2
        // holds it -- 149 -> 173 us at 16384 points, 88 -> 126 us at 4096: profiles/r05_p_analysis_touch_next_segment.txt)
        // (Round 6, 16384 points only -- one workgroup per CU, nobody else to cover a segment's load latency: the next
        // segment's frames are asked for behind the row pass, so that they travel under the magnitudes phase; the registers
        // they wait in are live across that phase only: k_analyze<14> 149.6 -> 130.2 us, profiles/r06_f_*.  One `raw`, no branches around it -- the form k_conv_wide
        // prefetches in: behind the last segment of the chunk the loads run into the next chunk's frames, or past the
        // track where the buffer's range check answers zeros, and are dropped.)
        if (!AHEAD) AB::fetch(tid, (long long)d * a.piece + (long long)s * F::N, a, raw);
        AB::phase_load(tid, raw, ps, th, lds);
        lds_barrier();
        fwd_middle_passes<F>(tid, lds, mid_table);
        typename AB::Row own;
        AB::phase_row(tid, own, lds);
        if (AHEAD) {
            __builtin_amdgcn_sched_barrier(0);          // (not above the row pass: its butterflies need the registers)
            AB::fetch(mgx_opaque(tid), (long long)d * a.piece + (long long)(s + 1) * F::N, a, raw);
            __builtin_amdgcn_sched_barrier(0);
        }
        lds_barrier();
        AB::phase_magnitudes(tid, own, th, lds);
        lds_barrier();
    }
    if (ch == a.chunks_per_piece - 1) {
        AB::phase_loose_frames(tid, (long long)d * a.piece + (long long)a.segs_per_piece * F::N,
                               (long long)(d + 1) * a.piece, true, a, th);
        if (d == a.divisions - 1)
            AB::phase_loose_frames(tid, (long long)a.divisions * a.piece, a.n, false, a, th);
    }
    AB::phase_write_spectrum(tid, wg, a, th);
    const double ss = block_sum<F::T>(th.sumsq, dscratch);
    const float pk = block_max<F::T>(th.peak, fscratch);
    if (tid == 0) {
        a.wg_sumsq[wg] = ss;
        a.wg_peak[wg] = pk;
    }
}

// fft_size = 2 * Fft2<LOG2H>::N (analysis2_kernel.h, AnalysisDouble): the same grid layout and outputs, two
// transforms per segment
template <int LOG2H>
__global__ __launch_bounds__(Fft2<LOG2H>::T, analysis_waves_per_simd<LOG2H>()) void k_analyze_double(AnalysisArgs a0,
                                                                                                    AnalysisArgs a1,
                                                                                                    int nwg0) {
    using AD = AnalysisDouble<LOG2H>;
    using F = Fft2<LOG2H>;
    MGX_LDS;
    float2* lds = reinterpret_cast<float2*>(mgx_smem);
    float2* mid_table = lds + F::LDS_ELEMS;
    double* dscratch = reinterpret_cast<double*>(mid_table + F::MID_TABLE);
    float* fscratch = reinterpret_cast<float*>(dscratch + F::T / 64);   // (one slot per wave each)
    const bool second = (int)blockIdx.x >= nwg0;                 // uniform
    const AnalysisArgs& a = second ? a1 : a0;
    const int tid = threadIdx.x, wg = second ? blockIdx.x - nwg0 : blockIdx.x;
    const int d = wg / a.chunks_per_piece, ch = wg % a.chunks_per_piece;
    typename AD::Thread th;
    AD::init(th);
    typename AD::Persist ps;
    AD::AB::load_persist(tid, a.tw, mid_table, ps);
    __syncthreads();
    int s0, s1;
    AD::AB::chunk_segments(a, ch, s0, s1);
    for (int s = s0; s < s1; ++s) {
        const long long start = (long long)d * a.piece + (long long)s * 2 * F::N;
        AD::template phase_load<false>(tid, start, a, ps, th, lds);
        lds_barrier();
        fwd_middle_passes<F, false>(tid, lds, mid_table);
        AD::phase_row(tid, lds);
        lds_barrier();
        AD::template phase_magnitudes<false>(tid, th, lds);
        lds_barrier();
        AD::template phase_load<true>(tid, start, a, ps, th, lds);
        lds_barrier();
        fwd_middle_passes<F, false>(tid, lds, mid_table);
        AD::phase_row(tid, lds);
        lds_barrier();
        AD::template phase_magnitudes<true>(tid, th, lds);
        lds_barrier();
    }
    if (ch == a.chunks_per_piece - 1) {
        AD::phase_loose_frames(tid, (long long)d * a.piece + (long long)a.segs_per_piece * 2 * F::N,
                               (long long)(d + 1) * a.piece, true, a, th);
        if (d == a.divisions - 1)
            AD::phase_loose_frames(tid, (long long)a.divisions * a.piece, a.n, false, a, th);
    }
    AD::phase_write_spectrum(tid, wg, a, th);
    const double ss = block_sum<F::T>(th.sumsq, dscratch);
    const float pk = block_max<F::T>(th.peak, fscratch);
    if (tid == 0) {
        a.wg_sumsq[wg] = ss;
        a.wg_peak[wg] = pk;
    }
}

// fft_size = 4 * Fft2<LOG2H>::N (analysis2_kernel.h, AnalysisQuad): the same grid layout and outputs, four transforms
// per segment; the spectrum sums live in the workgroup's slice of a.wg_pack until the end
template <int LOG2H>
__global__ __launch_bounds__(Fft2<LOG2H>::T, analysis_waves_per_simd<LOG2H>()) void k_analyze_quad(AnalysisArgs a0,
                                                                                                  AnalysisArgs a1,
                                                                                                  int nwg0) {
    using AQ = AnalysisQuad<LOG2H>;
    using F = Fft2<LOG2H>;
    MGX_LDS;
    float2* lds = reinterpret_cast<float2*>(mgx_smem);
    float2* mid_table = lds + F::LDS_ELEMS;
    double* dscratch = reinterpret_cast<double*>(mid_table + F::MID_TABLE);
    float* fscratch = reinterpret_cast<float*>(dscratch + F::T / 64);   // (one slot per wave each)
    const bool second = (int)blockIdx.x >= nwg0;                 // uniform
    const AnalysisArgs& a = second ? a1 : a0;
    const int tid = threadIdx.x, wg = second ? blockIdx.x - nwg0 : blockIdx.x;
    const int d = wg / a.chunks_per_piece, ch = wg % a.chunks_per_piece;
    typename AQ::Thread th;
    AQ::init(th);
    typename AQ::Persist ps;
    AQ::AB::load_persist(tid, a.tw, mid_table, ps);
    AQ::phase_clear(tid, wg, a);
    __syncthreads();
    int s0, s1;
    AQ::AB::chunk_segments(a, ch, s0, s1);
    auto transform = [&]() {
        lds_barrier();
        fwd_middle_passes<F, false>(opaque(tid), lds, mid_table);
        AQ::phase_row(opaque(tid), lds);
        lds_barrier();
    };
    for (int s = s0; s < s1; ++s) {
        const long long start = (long long)d * a.piece + (long long)s * 4 * F::N;
        typename AQ::Pairs u;
        AQ::template phase_load<false, 0>(opaque(tid), start, a, ps, th, lds);
        transform();
        AQ::phase_unmix(opaque(tid), u, lds);
        AQ::phase_keep(opaque(tid), wg, a, u);
        lds_barrier();
        AQ::template phase_load<false, 1>(opaque(tid), start, a, ps, th, lds);
        transform();
        AQ::phase_unmix(opaque(tid), u, lds);
        AQ::template phase_magnitudes<false>(opaque(tid), wg, a, u);
        lds_barrier();
        AQ::template phase_load<true, 0>(opaque(tid), start, a, ps, th, lds);
        transform();
        AQ::phase_unmix(opaque(tid), u, lds);
        AQ::phase_keep(opaque(tid), wg, a, u);
        lds_barrier();
        AQ::template phase_load<true, 1>(opaque(tid), start, a, ps, th, lds);
        transform();
        AQ::phase_unmix(opaque(tid), u, lds);
        AQ::template phase_magnitudes<true>(opaque(tid), wg, a, u);
        lds_barrier();
    }
    if (ch == a.chunks_per_piece - 1) {
        AQ::phase_loose_frames(tid, (long long)d * a.piece + (long long)a.segs_per_piece * 4 * F::N,
                               (long long)(d + 1) * a.piece, true, a, th);
        if (d == a.divisions - 1)
            AQ::phase_loose_frames(tid, (long long)a.divisions * a.piece, a.n, false, a, th);
    }
    AQ::phase_write_spectrum(tid, wg, a);
    const double ss = block_sum<F::T>(th.sumsq, dscratch);
    const float pk = block_max<F::T>(th.peak, fscratch);
    if (tid == 0) {
        a.wg_sumsq[wg] = ss;
        a.wg_peak[wg] = pk;
    }
}

}  // namespace mgx

// (after the kernels above: the order in which kernels are first defined is the order of the device code object)
#include "levels_kernels.h"
#include "fir_kernels.h"
#include "correction_kernels.h"
#include "io_kernels.h"
#include "limiter_kernels.h"
#include "profile_kernels.h"       // (off the pair route's chain: last, so that it moves none of the kernels above)
#include "eq_shape_kernels.h"      // (likewise: only a call with an mgx_eq_shape launches them)
