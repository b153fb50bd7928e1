// What every device-only header of the library shares (gfx950, wave64; not part of the CPU emulation):
//   * MGX_LDS, the LDS-only barrier and the barrier-free middle passes of the LDS transforms (fft2.h, fft2_lanes.h),
//   * wave and workgroup reductions by shuffles and DPP, and `opaque` (a thread id the compiler may not hoist),
//   * the handle's device-error words (DEVICE_ERROR_*),
//   * code warming: the CODE_* table of kernel sizes and warm_code.
// The *_kernel.h headers hold the phase functions the emulation drives; the *_kernels.h headers hold __global__
// kernels and device-only helpers and build on this file.
#pragma once

#include <hip/hip_runtime.h>

#include "fft2_lanes.h"

namespace mgx {

#define MGX_LDS extern __shared__ __attribute__((aligned(16))) char mgx_smem[]

// Workgroup barrier that orders LDS traffic only: global loads issued before it stay in flight
// (__syncthreads() would drain vmcnt as well and serialise a software prefetch).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Between two phases of a transform that lie between pass 0 and the inverse of pass 0.  In a plan with
// Fft2::WAVE_LOCAL every wave reads there only what it wrote itself, and the LDS executes one wave's instructions in
// program order: all that is needed is that the COMPILER keeps the order (a memory clobber), no s_barrier.  With
// sixteen waves per workgroup and one workgroup per CU (the 16384-point kernels) a barrier idles the whole CU
// until the last wave arrives; this takes them from ten per block to five.  Other plans get the barrier.
template <class F>
__device__ __forceinline__ void pass_sync() {
    if constexpr (F::WAVE_LOCAL) asm volatile("" ::: "memory");
    else lds_barrier();
}

// The middle passes of a transform, forward and inverse, as the kernels below call them (each followed / preceded by
// the pass_sync the separate passes had).  A four-pass plan (16384 points) runs its two radix-8 passes as ONE phase
// with the exchange between them in the wave's lanes (fft2_lanes.h: bit-identical results, one LDS round trip and one
// wait fewer per direction: k_conv_wide<14> 144.3 -> 139.4 us, k_conv_delay<14> 238.5 -> 232.7, profiles/r06_b_*).
// LANES = false: kernels that hold an accumulator row
// or a second transform's registers across the middle passes (k_conv<14>, the two- and four-transform analysis) keep
// the two-phase form -- both butterflies of a thread alive at once is 16 registers they do not have.
template <class F, bool LANES = true>
__device__ __forceinline__ void fwd_middle_passes(int tid, float2* lds, const float2* mid_table) {
    if constexpr (F::P == 4 && LANES) {
        Fft2Lanes<ilog2(F::N)>::fwd_mid_fused(tid, lds, mid_table);
        pass_sync<F>();
        return;
    }
    if constexpr (F::P >= 3) {
        F::fwd_mid(tid, lds, mid_table);
        pass_sync<F>();
    }
    if constexpr (F::P == 4) {
        F::fwd_mid2(mgx_opaque(tid), lds, mid_table);
        pass_sync<F>();
    }
}
template <class F, bool LANES = true>
__device__ __forceinline__ void inv_middle_passes(int tid, float2* lds, const float2* mid_table) {
    if constexpr (F::P == 4 && LANES) {
        pass_sync<F>();
        Fft2Lanes<ilog2(F::N)>::inv_mid_fused(tid, lds, mid_table);
        return;
    }
    if constexpr (F::P == 4) {
        pass_sync<F>();
        F::inv_mid2(tid, lds, mid_table);
    }
    if constexpr (F::P >= 3) {
        pass_sync<F>();
        F::inv_mid(mgx_opaque(tid), lds, mid_table);
    }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// inclusive prefix sum over the 64 lanes: four steps inside each row of 16 (row_shr 1, 2, 4, 8; lanes
// without a source add 0), then lane 15 of rows 0 and 2 into rows 1 and 3, then lane 31 into rows 2 and 3
__device__ __forceinline__ int wave_inclusive_sum(int x) {
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);    // row_bcast:15
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);    // row_bcast:31
    return x;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
// scratch: at least (threads/64) floats / doubles of LDS; result valid on thread 0
template <int THREADS>
__device__ __forceinline__ float block_max(float v, float* scratch) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = 0.f;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) r = fmaxf(r, scratch[w]);
    }
    return r;
}
// the same behind an LDS-only barrier: global loads asked for earlier (a software prefetch) stay in flight
template <int THREADS>
__device__ __forceinline__ float block_max_lds(float v, float* scratch) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    lds_barrier();
    float r = 0.f;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) r = fmaxf(r, scratch[w]);
    }
    return r;
}
template <int THREADS>
__device__ __forceinline__ double block_sum(double v, double* scratch) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) r += scratch[w];
    }
    return r;
}

// The phases of a kernel share index arithmetic (LDS addresses derived from the thread id).  Left
// alone, the compiler computes it once and keeps dozens of addresses alive across the whole
// kernel -- in scratch memory once the registers run out.  An empty asm makes the id opaque so
// that each phase re-derives its few addresses instead (the same goes for loop-invariant LDS
// table reads: hoisted out of a persistent loop they would live in scratch).
__device__ __forceinline__ int opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

// The handle's error words: ONE int per kind of failure (error[0] look-back, error[1] tail, error[2] input), each set by
// a plain store of 1 -- kernels of different kinds never write the same word, so a later tail expiry cannot erase an
// earlier lost look-back word; the host folds them into the DEVICE_ERROR_* bits below.
// A limiter look-back that expires (limiter_kernel.h) means a lost word: the
// audio is wrong and the call fails.  An expired wait of k_correction_tail means its workgroups were not resident
// together (another process's kernels held the compute units): the host then runs the rounds again as one launch
// each, which wait for nobody (device_errors.h, check_device_error).  DEVICE_ERROR_INPUT is not a wait at all: the level
// analysis met a NaN or an infinity (k_match_curve), where the reference raises.  Nor is DEVICE_ERROR_PROFILE: a reference
// profile whose header does not fit the call's Config (profile_kernels.h); its word holds WHICH field, not a 1.
constexpr int DEVICE_ERROR_LOOKBACK = 1, DEVICE_ERROR_TAIL = 2, DEVICE_ERROR_INPUT = 4, DEVICE_ERROR_PROFILE = 8;
constexpr int DEVICE_ERROR_SLOT_LOOKBACK = 0, DEVICE_ERROR_SLOT_TAIL = 1, DEVICE_ERROR_SLOT_INPUT = 2, DEVICE_ERROR_SLOT_PROFILE = 3,
              DEVICE_ERROR_SLOTS = 4;

// ---------------------------------------------------------------------------
// code warming
// ---------------------------------------------------------------------------
// The kernels of this library are long stretches of straight-line code (a fully unrolled 8192-point
// transform is 38 KB, the limiter 105 KB), and every launch finds them evicted from the L2s by the hundreds of
// megabytes the previous kernel streamed.  The instruction cache then pulls them in line by line behind the
// first wave: ~32 ns per 64-byte line on some boxes of the pool and ~170 ns on others (same clocks, same
// memory latencies; tools/probe, profiles/r03_*_box_class.json) -- the whole difference between a
// "fast" and a "slow" box.  So the first eight workgroups of a launch -- one per XCD: the L2s are per XCD --
// read their own kernel's code AS DATA, 4 KB per load instruction and all of it in flight at once, which puts it
// into the XCD's L2; instruction fetch then finds it there.  (Every workgroup of the first generation doing so was
// measured: the limiter lost 14 us to the wait; so was warming again every 16th or 64th workgroup of an XCD, in
// case the streamed audio pushes the code out of the L2 again: +6 / +13 us.)  Sizes come from the code object's
// symbol table (code_sizes.h, code_sizes_from_library; uploaded by mgx_create); zero = no warming.
enum { CODE_ANALYZE = 0, CODE_MATCH_CURVE, CODE_CONV_PREP, CODE_CONV, CODE_ROUND, CODE_TAIL, CODE_LIMIT, CODE_KERNELS };
constexpr int CODE_VARIANTS = 16;                                  // second index: log2 of the transform; 0 / 1 = 256 / 1024-block limiter
constexpr int CODE_VARIANT_CONV_DELAY = 15;                        // [CODE_CONV][15]: k_conv_delay<14>
constexpr int CODE_VARIANT_CONV_WIDE = 6;                          // [CODE_CONV][6]: k_conv_wide<14> (there is no k_conv<6>)
__device__ int g_code_bytes[CODE_KERNELS][CODE_VARIANTS];
__device__ __forceinline__ void warm_code(int which, int variant = 0) {
    if (blockIdx.x >= 8 || threadIdx.x >= 64) return;             // workgroup b runs on XCD b % 8: one wave per L2
    const int bytes = g_code_bytes[which][variant];
    // Where this kernel's code starts: dispatch packet -> kernel descriptor -> entry offset (the AMDHSA code object
    // ABI: hsa_kernel_dispatch_packet_t::kernel_object at byte 32 points at the 64-byte descriptor, whose
    // kernel_code_entry_byte_offset at byte 16 is relative to the descriptor).  The window read is then exactly
    // [entry, entry + symbol size): it cannot run past the kernel whatever the compiler did with the block that
    // holds these loads (the program counter of this block is not the entry point).
    const char* packet = (const char*)__builtin_amdgcn_dispatch_ptr();      // (constant address space -> generic)
    const char* descriptor = *reinterpret_cast<const char* const*>(packet + 32);
    const char* entry = descriptor + *reinterpret_cast<const long long*>(descriptor + 16);
    int acc = 0;
    for (int off = (int)threadIdx.x * 64; off < bytes; off += 4096) acc += *reinterpret_cast<const volatile int*>(entry + off);
    if (acc == 0x7ffffff1) asm volatile("s_nop 0");                // (the sum is needed: the loads are waited for here)
}

}  // namespace mgx
