// Delivery renditions (include/mgx.h, mgx_deliver): gain, dither, quantise and pack in one pass over frames in HBM --
// tests/delivery_oracle.py is the numpy form.
//
//     a = ((double)x[s] * gain) * top,  top = 2^(bits-1) - 1        (two float64 products, in this order)
//     v = clip(rint(a + d(s)), -top - 1, top)                       (bits == 0: out[s] = (float)((double)x[s] * gain))
//
// d(s) comes from Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), a counter-based
// generator: block q = s >> 2 of stream t is philox(counter = (q lo, q hi, t, 0), key = (seed lo, seed hi)), its word
// s & 3 is sample s's, U = ((W >> 8) + 0.5) 2^-24 - 0.5 lies inside (-1/2, 1/2) and is exact in float64.
//     TPDF:               d(s) = U(s, 0) + U(s, 1)
//     high-passed TPDF:   d(s) = U(s, 0) - U(s - 2, 0)              (s - 2: the same channel one frame earlier; U = 0 before
//                                                                    the track).  Triangular density, first-differenced
//                                                                    spectrum, no error feedback.
// Both sums are exact in float64 (multiples of 2^-25 below 1), so a + d rounds once and every value is defined bit for
// bit.  A thread owns quad q -- samples 4q .. 4q+3, exactly one Philox block per stream; the high-passed form takes the
// two words it needs from block q - 1 by a second call, nothing sequential, no neighbour -- loads it with one 16-byte
// access and stores 8 bytes (16 bit), three words (24 bit, packed little-endian as k_pcm_encode packs them) or 16 bytes.
// The samples % 4 behind the last quad go one each to the first threads of workgroup 0, as in k_pcm_encode's 24-bit path.
// No LDS, no barrier, nobody waits for anybody.  The bodies are MGX_HD so that tests/emu/emu_deliver.cpp runs them; what
// the host decides of a launch -- the arguments but the pointers, and the grid -- is deliver_launch and deliver_grid,
// for mgx_deliver and the emulation alike.
#pragma once

#include "mgx_hd.h"

namespace mgx {

constexpr int DELIVER_THREADS = 256;
constexpr int DELIVER_GRID_MAX = 2048;          // workgroups of a launch: 8 per CU; longer tracks wrap (grid-stride)

struct DeliverArgs {
    const float* x;             // [samples] float32, interleaved
    long long samples;
    double gain;
    int bits;                   // 0 (float32 out), 16, 24, 32
    int dither;                 // 0 none, 1 TPDF, 2 high-passed TPDF
    unsigned key0, key1;        // seed low / high word
    void* out;
};

// ---- what the host decides (mgx_deliver and the emulation alike) -------------------------------------------------------
MGX_HD long long deliver_grid(long long samples) {
    const long long blocks = (samples / 4 + DELIVER_THREADS - 1) / DELIVER_THREADS;
    return blocks < 1 ? 1 : (blocks > DELIVER_GRID_MAX ? DELIVER_GRID_MAX : blocks);
}
// everything of the arguments but the pointers
inline void deliver_launch(DeliverArgs& a, long long samples, double gain, int bits, int dither, unsigned long long seed) {
    a.samples = samples, a.gain = gain;
    a.bits = bits, a.dither = dither;
    a.key0 = (unsigned)seed, a.key1 = (unsigned)(seed >> 32);
}

struct alignas(16) DeliverWords4 { unsigned x, y, z, w; };
struct alignas(8) DeliverWords2 { unsigned x, y; };

MGX_HD unsigned deliver_mulhi(unsigned a, unsigned b) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(MGX_HOST_EMU)
    return __umulhi(a, b);
#else
    return (unsigned)(((unsigned long long)a * b) >> 32);
#endif
}

// Philox4x32-10: w = the four output words of (c0, c1, c2, c3) under key (k0, k1)
MGX_HD void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned* w) {
    MGX_UNROLL
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = deliver_mulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = deliver_mulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

MGX_HD double deliver_uniform(unsigned w) { return ((double)(w >> 8) + 0.5) * (1.0 / 16777216.0) - 0.5; }

// d(4q) .. d(4q + 3)
MGX_HD void deliver_dither_quad(const DeliverArgs& a, long long q, double* d) {
    d[0] = d[1] = d[2] = d[3] = 0.0;
    if (a.dither == 0) return;
    unsigned w[4], v[4];
    philox4x32_10((unsigned)q, (unsigned)((unsigned long long)q >> 32), 0u, 0u, a.key0, a.key1, w);
    if (a.dither == 1) {
        philox4x32_10((unsigned)q, (unsigned)((unsigned long long)q >> 32), 1u, 0u, a.key0, a.key1, v);
        MGX_UNROLL
        for (int i = 0; i < 4; ++i) d[i] = deliver_uniform(w[i]) + deliver_uniform(v[i]);
    } else {
        const long long p = q - 1;
        philox4x32_10((unsigned)p, (unsigned)((unsigned long long)p >> 32), 0u, 0u, a.key0, a.key1, v);
        const double u0 = deliver_uniform(w[0]), u1 = deliver_uniform(w[1]);
        d[0] = u0 - (q > 0 ? deliver_uniform(v[2]) : 0.0);
        d[1] = u1 - (q > 0 ? deliver_uniform(v[3]) : 0.0);
        d[2] = deliver_uniform(w[2]) - u0;
        d[3] = deliver_uniform(w[3]) - u1;
    }
}

// U(s, stream), 0 before the track; d(s) of one sample, straight from the definition (the ragged tail)
MGX_HD double deliver_uniform_at(const DeliverArgs& a, long long s, unsigned stream) {
    if (s < 0) return 0.0;
    const long long q = s >> 2;
    unsigned w[4];
    philox4x32_10((unsigned)q, (unsigned)((unsigned long long)q >> 32), stream, 0u, a.key0, a.key1, w);
    const int i = (int)(s & 3);
    return deliver_uniform(i == 0 ? w[0] : i == 1 ? w[1] : i == 2 ? w[2] : w[3]);
}
MGX_HD double deliver_dither_one(const DeliverArgs& a, long long s) {
    if (a.dither == 1) return deliver_uniform_at(a, s, 0u) + deliver_uniform_at(a, s, 1u);
    if (a.dither == 2) return deliver_uniform_at(a, s, 0u) - deliver_uniform_at(a, s - 2, 0u);
    return 0.0;
}

MGX_HD int deliver_quantise(float x, double gain, double top, double d) {
    const double scaled = ((double)x * gain) * top;
    const double q = rint(scaled + d);
    return (int)fmin(fmax(q, -top - 1.0), top);
}

// quad q: samples 4q .. 4q+3, all inside the track
MGX_HD void deliver_quad(const DeliverArgs& a, long long q) {
    const float4 v = *reinterpret_cast<const float4*>(a.x + 4 * q);
    if (a.bits == 0) {
        float4 o;
        o.x = (float)((double)v.x * a.gain); o.y = (float)((double)v.y * a.gain);
        o.z = (float)((double)v.z * a.gain); o.w = (float)((double)v.w * a.gain);
        *reinterpret_cast<float4*>(static_cast<float*>(a.out) + 4 * q) = o;
        return;
    }
    const double top = (double)((1ll << (a.bits - 1)) - 1);
    double d[4];
    deliver_dither_quad(a, q, d);
    const int i0 = deliver_quantise(v.x, a.gain, top, d[0]), i1 = deliver_quantise(v.y, a.gain, top, d[1]);
    const int i2 = deliver_quantise(v.z, a.gain, top, d[2]), i3 = deliver_quantise(v.w, a.gain, top, d[3]);
    if (a.bits == 16) {
        DeliverWords2 o;
        o.x = ((unsigned)i0 & 0xFFFFu) | ((unsigned)i1 << 16);
        o.y = ((unsigned)i2 & 0xFFFFu) | ((unsigned)i3 << 16);
        static_cast<DeliverWords2*>(a.out)[q] = o;
    } else if (a.bits == 32) {
        DeliverWords4 o;
        o.x = (unsigned)i0; o.y = (unsigned)i1; o.z = (unsigned)i2; o.w = (unsigned)i3;
        static_cast<DeliverWords4*>(a.out)[q] = o;
    } else {
        const unsigned b0 = (unsigned)i0 & 0xFFFFFFu, b1 = (unsigned)i1 & 0xFFFFFFu;
        const unsigned b2 = (unsigned)i2 & 0xFFFFFFu, b3 = (unsigned)i3 & 0xFFFFFFu;
        unsigned* out = static_cast<unsigned*>(a.out);
        out[3 * q] = b0 | (b1 << 24);
        out[3 * q + 1] = (b1 >> 8) | (b2 << 16);
        out[3 * q + 2] = (b2 >> 16) | (b3 << 8);
    }
}

// sample s of the ragged tail, alone
MGX_HD void deliver_one(const DeliverArgs& a, long long s) {
    if (a.bits == 0) {
        static_cast<float*>(a.out)[s] = (float)((double)a.x[s] * a.gain);
        return;
    }
    const double top = (double)((1ll << (a.bits - 1)) - 1);
    const int v = deliver_quantise(a.x[s], a.gain, top, deliver_dither_one(a, s));
    if (a.bits == 16) {
        static_cast<short*>(a.out)[s] = (short)v;
    } else if (a.bits == 32) {
        static_cast<int*>(a.out)[s] = v;
    } else {
        unsigned char* bytes = static_cast<unsigned char*>(a.out);
        bytes[3 * s] = (unsigned char)v;
        bytes[3 * s + 1] = (unsigned char)((unsigned)v >> 8);
        bytes[3 * s + 2] = (unsigned char)((unsigned)v >> 16);
    }
}

// everything thread `thread` of workgroup `block` does in a launch of `grid` workgroups
MGX_HD void deliver_thread(const DeliverArgs& a, long long block, int thread, long long grid) {
    const long long quads = a.samples / 4, stride = grid * DELIVER_THREADS;
    for (long long q = block * DELIVER_THREADS + thread; q < quads; q += stride) deliver_quad(a, q);
    if (block == 0 && thread < (int)(a.samples - 4 * quads)) deliver_one(a, 4 * quads + thread);
}

#if defined(__HIPCC__) && !defined(MGX_HOST_EMU)
__global__ __launch_bounds__(DELIVER_THREADS) void k_deliver(DeliverArgs a) {
    deliver_thread(a, blockIdx.x, threadIdx.x, gridDim.x);
}
#endif

}  // namespace mgx
