// Noise-shaped deliveries (include/mgx.h, mgx_deliver_shaped): k_deliver's gain, TPDF dither, quantiser and packing with
// the quantiser's error fed back through a short filter -- tests/deliver_shaped_oracle.py is the numpy form.
//
//     a = ((double)x[s] * gain) * top,  d = U(s, 0) + U(s, 1)          (deliver_kernel.h's values, its Philox, its U)
//     t = 0.0;  for k = 1..K:  t = t + c[k] * e_k                      (one product and one sum per tap, in this order)
//     w = a - t;  r = rint(w + d);  e_new = r - w;  (e_K, .., e_1) <- (e_{K-1}, .., e_1, e_new)
//     out = clip(r, -top - 1, top)
//
// The recurrence is not linear (rint), so no scan removes it; the chains are made short and many instead.  Segment j is
// the frames [jB, min(n, (j+1)B)); each channel of each segment is one chain, which starts W frames early (at frame
// max(0, jB - W)) with e = 0 and writes nothing before jB.  One lane owns one chain; a workgroup owns SHAPED_SEGMENTS
// consecutive segments -- 64 chains, the lanes of its first wave -- no workgroup waits for another and there is no
// grid-stride loop.  The other three waves own no chain: the chains are too few to fill the chip (646 waves' worth on the
// 8-minute track for 1024 SIMDs) and most of the work is the dither's Philox blocks, which any lane can compute.
//
// A lane's frames are a contiguous stretch B * 8 bytes from its neighbour's, so the workgroup works in steps of
// SHAPED_STEP frames, each of three phases between barriers (the bodies are MGX_HD: tests/emu/emu_deliver_shaped.cpp runs
// them):
//   fill    every thread of the four waves takes frame PAIRS -- 16 bytes, the four samples of exactly one Philox block
//           per stream -- lanes consecutive along a segment (256 contiguous bytes per segment and step), computes a and d and puts them into
//           the LDS transposed: slot(frame, chain) = frame * (CHAINS + 1) + chain, 16 bytes {a, d} each.
//   run     first wave only, lane = chain: SHAPED_STEP serial steps; lane c reads slot(f, c) -- consecutive lanes,
//           consecutive 16-byte slots: no bank conflict, and no address depends on e, so the reads run ahead of the chain -- and leaves r, as
//           an int, in the slot's first word.
//   store   the fill's mapping again, all four waves: four values per thread, packed as k_deliver packs them, 8 bytes
//           (16 bit) or three words (24 bit) per pair, lanes consecutive along a segment.
// The one pad slot per frame row spreads the fill's writes (lanes a frame pair apart) over the banks: 2-way instead of
// 16-way.  The taps are a template argument of the serial loop (0 .. 16, chosen once per launch by a uniform switch), so
// that the products and sums on the chain are exactly the K the definition names and e lives in registers.
// Frame pairs before the track (segment 0's warm-up) and behind its end are filled with a = d = 0 (the frame behind an
// odd last frame with a = 0 and its Philox d), so the serial loop has no branch: before the track w = r = e = 0 exactly,
// which is the chain starting at frame 0 with e = 0; behind the end nothing is written and no stored frame follows.
#pragma once

#include "deliver_kernel.h"

namespace mgx {

constexpr int SHAPED_TAPS_MAX = 16;              // MGX_SHAPER_TAPS_MAX
constexpr int SHAPED_CHAINS = 64;                // chains of a workgroup: one wave's lanes
constexpr int SHAPED_THREADS = 256;              // ... and its threads: every wave fills and stores, the first runs the chains
constexpr int SHAPED_SEGMENTS = SHAPED_CHAINS / 2;    // segments of a workgroup's tile (two channels each)
constexpr int SHAPED_STEP = 32;                  // frames of a step; divides the segment and the warm-up, even
constexpr int SHAPED_ROW = SHAPED_CHAINS + 1;    // slots of a frame row, one of them padding
constexpr int SHAPED_PAIRS = SHAPED_SEGMENTS * (SHAPED_STEP / 2);      // frame pairs of a step
constexpr size_t SHAPED_LDS_BYTES = (size_t)SHAPED_STEP * SHAPED_ROW * 16;

struct DeliverShapedArgs {
    const float* x;             // [frames][2] float32
    long long frames;
    double gain;
    int bits;                   // 16 or 24
    int taps;                   // K, 0 .. 16
    int segment, warmup;        // B and W in frames: multiples of SHAPED_STEP (the library: MGX_SHAPER_SEGMENT / _WARMUP)
    unsigned key0, key1;        // seed low / high word
    void* out;
    double c[SHAPED_TAPS_MAX];  // c[k - 1] = the definition's c[k]
};

// a and d on the way in; the run leaves r, as an int, where a was
struct alignas(16) ShapedSlot {
    union { double a; int r; };
    double d;
};
struct ShapedThread { double e[SHAPED_TAPS_MAX]; };

// ---- what the host decides (mgx_deliver_shaped and the emulation alike) -------------------------------------------------
MGX_HD long long shaped_segments(long long frames, int segment) { return (frames + segment - 1) / segment; }
MGX_HD long long shaped_grid(long long frames, int segment) {
    return (shaped_segments(frames, segment) + SHAPED_SEGMENTS - 1) / SHAPED_SEGMENTS;
}
MGX_HD int shaped_steps(int segment, int warmup) { return (segment + warmup) / SHAPED_STEP; }
// everything of the arguments but the pointers
inline void deliver_shaped_launch(DeliverShapedArgs& a, long long frames, double gain, int bits, int taps, const double* c,
                                  int segment, int warmup, unsigned long long seed) {
    a.frames = frames, a.gain = gain;
    a.bits = bits, a.taps = taps;
    a.segment = segment, a.warmup = warmup;
    a.key0 = (unsigned)seed, a.key1 = (unsigned)(seed >> 32);
    for (int k = 0; k < SHAPED_TAPS_MAX; ++k) a.c[k] = k < taps ? c[k] : 0.0;
}

// the first frame of segment `seg` of tile `tile` in step `step` (negative in segment 0's warm-up)
MGX_HD long long shaped_first(const DeliverShapedArgs& a, long long tile, int seg, int step) {
    return (tile * SHAPED_SEGMENTS + seg) * (long long)a.segment - a.warmup + (long long)step * SHAPED_STEP;
}

MGX_HD void shaped_put(ShapedSlot* lds, int frame, int chain, float x, double gain, double top, unsigned w0, unsigned w1) {
    ShapedSlot s;
    s.a = ((double)x * gain) * top;
    s.d = deliver_uniform(w0) + deliver_uniform(w1);
    lds[frame * SHAPED_ROW + chain] = s;
}

// ---- fill: a and d of the step's frames, transposed into the LDS ---------------------------------------------------------
MGX_HD void shaped_fill(const DeliverShapedArgs& a, long long tile, int step, ShapedSlot* lds, int thread) {
    const double top = (double)((1ll << (a.bits - 1)) - 1);
    for (int item = thread; item < SHAPED_PAIRS; item += SHAPED_THREADS) {
        const int seg = item / (SHAPED_STEP / 2), pair = item % (SHAPED_STEP / 2);
        const long long m = shaped_first(a, tile, seg, step) + 2 * pair;          // even: frames m, m + 1 are quad m / 2
        if (m < 0 || m >= a.frames) {                                             // outside the track: a = d = 0 (below)
            ShapedSlot zero;
            zero.a = 0.0, zero.d = 0.0;
            lds[2 * pair * SHAPED_ROW + 2 * seg] = lds[2 * pair * SHAPED_ROW + 2 * seg + 1] = zero;
            lds[(2 * pair + 1) * SHAPED_ROW + 2 * seg] = lds[(2 * pair + 1) * SHAPED_ROW + 2 * seg + 1] = zero;
            continue;
        }
        float4 v;
        if (m + 1 < a.frames) {
            v = *reinterpret_cast<const float4*>(a.x + 2 * m);
        } else {                                                                  // the track's last frame, alone
            const float2 last = *reinterpret_cast<const float2*>(a.x + 2 * m);
            v = make_float4(last.x, last.y, 0.f, 0.f);
        }
        const long long q = m >> 1;
        unsigned w[4], u[4];
        philox4x32_10((unsigned)q, (unsigned)((unsigned long long)q >> 32), 0u, 0u, a.key0, a.key1, w);
        philox4x32_10((unsigned)q, (unsigned)((unsigned long long)q >> 32), 1u, 0u, a.key0, a.key1, u);
        shaped_put(lds, 2 * pair, 2 * seg, v.x, a.gain, top, w[0], u[0]);
        shaped_put(lds, 2 * pair, 2 * seg + 1, v.y, a.gain, top, w[1], u[1]);
        shaped_put(lds, 2 * pair + 1, 2 * seg, v.z, a.gain, top, w[2], u[2]);
        shaped_put(lds, 2 * pair + 1, 2 * seg + 1, v.w, a.gain, top, w[3], u[3]);
    }
}

// ---- run: the chain's SHAPED_STEP serial steps ---------------------------------------------------------------------------
template <int K>
MGX_HD void shaped_run_taps(const DeliverShapedArgs& a, ShapedSlot* lds, int chain, ShapedThread& th) {
    const double top = (double)((1ll << (a.bits - 1)) - 1);
    double e[K > 0 ? K : 1];
    MGX_UNROLL
    for (int k = 0; k < K; ++k) e[k] = th.e[k];
#if defined(__HIP_DEVICE_COMPILE__) && !defined(MGX_HOST_EMU)
#pragma unroll 8
#endif
    for (int f = 0; f < SHAPED_STEP; ++f) {
        ShapedSlot* slot = lds + f * SHAPED_ROW + chain;
        const ShapedSlot s = *slot;
        double t = 0.0;
        MGX_UNROLL
        for (int k = 0; k < K; ++k) t = t + a.c[k] * e[k];
        const double w = s.a - t;
        const double r = rint(w + s.d);
        MGX_UNROLL
        for (int k = K - 1; k > 0; --k) e[k] = e[k - 1];
        if (K > 0) e[0] = r - w;                                                  // (before the clip: |e| stays about 3/2)
        slot->r = (int)fmin(fmax(r, -top - 1.0), top);
    }
    MGX_UNROLL
    for (int k = 0; k < K; ++k) th.e[k] = e[k];
}

MGX_HD void shaped_start(ShapedThread& th) {
    MGX_UNROLL
    for (int k = 0; k < SHAPED_TAPS_MAX; ++k) th.e[k] = 0.0;
}

MGX_HD void shaped_run(const DeliverShapedArgs& a, ShapedSlot* lds, int thread, ShapedThread& th) {
    if (thread >= SHAPED_CHAINS) return;                                          // (wave-uniform: the helper waves own no chain)
    switch (a.taps) {                                                             // (uniform: one branch per launch)
#define MGX_SHAPED_CASE(K) case K: shaped_run_taps<K>(a, lds, thread, th); break;
        MGX_SHAPED_CASE(0) MGX_SHAPED_CASE(1) MGX_SHAPED_CASE(2) MGX_SHAPED_CASE(3) MGX_SHAPED_CASE(4) MGX_SHAPED_CASE(5)
        MGX_SHAPED_CASE(6) MGX_SHAPED_CASE(7) MGX_SHAPED_CASE(8) MGX_SHAPED_CASE(9) MGX_SHAPED_CASE(10) MGX_SHAPED_CASE(11)
        MGX_SHAPED_CASE(12) MGX_SHAPED_CASE(13) MGX_SHAPED_CASE(14) MGX_SHAPED_CASE(15) MGX_SHAPED_CASE(16)
#undef MGX_SHAPED_CASE
        default: break;
    }
}

// ---- store: pack and write the step's frames that lie inside their segment -----------------------------------------------
MGX_HD int shaped_value(const ShapedSlot* lds, int frame, int chain) {
    return lds[frame * SHAPED_ROW + chain].r;
}

// frame m alone (the track's last frame where the count is odd)
MGX_HD void shaped_store_frame(const DeliverShapedArgs& a, long long m, int v0, int v1) {
    if (a.bits == 16) {
        static_cast<unsigned*>(a.out)[m] = ((unsigned)v0 & 0xFFFFu) | ((unsigned)v1 << 16);
    } else {
        unsigned char* bytes = static_cast<unsigned char*>(a.out) + 6 * m;
        bytes[0] = (unsigned char)v0;
        bytes[1] = (unsigned char)((unsigned)v0 >> 8);
        bytes[2] = (unsigned char)((unsigned)v0 >> 16);
        bytes[3] = (unsigned char)v1;
        bytes[4] = (unsigned char)((unsigned)v1 >> 8);
        bytes[5] = (unsigned char)((unsigned)v1 >> 16);
    }
}

MGX_HD void shaped_store(const DeliverShapedArgs& a, long long tile, int step, const ShapedSlot* lds, int thread) {
    if (step * SHAPED_STEP < a.warmup) return;                                    // a warm-up step: computed, not written
    for (int item = thread; item < SHAPED_PAIRS; item += SHAPED_THREADS) {
        const int seg = item / (SHAPED_STEP / 2), pair = item % (SHAPED_STEP / 2);
        const long long m = shaped_first(a, tile, seg, step) + 2 * pair;
        if (m >= a.frames) continue;
        const int i0 = shaped_value(lds, 2 * pair, 2 * seg), i1 = shaped_value(lds, 2 * pair, 2 * seg + 1);
        if (m + 1 >= a.frames) {
            shaped_store_frame(a, m, i0, i1);
            continue;
        }
        const int i2 = shaped_value(lds, 2 * pair + 1, 2 * seg), i3 = shaped_value(lds, 2 * pair + 1, 2 * seg + 1);
        const long long q = m >> 1;
        if (a.bits == 16) {
            DeliverWords2 o;
            o.x = ((unsigned)i0 & 0xFFFFu) | ((unsigned)i1 << 16);
            o.y = ((unsigned)i2 & 0xFFFFu) | ((unsigned)i3 << 16);
            static_cast<DeliverWords2*>(a.out)[q] = o;
        } else {
            const unsigned b0 = (unsigned)i0 & 0xFFFFFFu, b1 = (unsigned)i1 & 0xFFFFFFu;
            const unsigned b2 = (unsigned)i2 & 0xFFFFFFu, b3 = (unsigned)i3 & 0xFFFFFFu;
            unsigned* out = static_cast<unsigned*>(a.out);
            out[3 * q] = b0 | (b1 << 24);
            out[3 * q + 1] = (b1 >> 8) | (b2 << 16);
            out[3 * q + 2] = (b2 >> 16) | (b3 << 8);
        }
    }
}

#if defined(__HIPCC__) && !defined(MGX_HOST_EMU)
__global__ __launch_bounds__(SHAPED_THREADS) void k_deliver_shaped(DeliverShapedArgs a) {
    __shared__ ShapedSlot lds[SHAPED_STEP * SHAPED_ROW];
    const long long tile = blockIdx.x;
    const int thread = threadIdx.x, steps = shaped_steps(a.segment, a.warmup);
    ShapedThread th;
    shaped_start(th);
    for (int step = 0; step < steps; ++step) {
        shaped_fill(a, tile, step, lds, thread);
        __syncthreads();
        shaped_run(a, lds, thread, th);
        __syncthreads();
        shaped_store(a, tile, step, lds, thread);
        __syncthreads();
    }
}
#endif

}  // namespace mgx
