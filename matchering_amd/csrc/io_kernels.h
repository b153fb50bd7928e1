// The small streaming kernels around the master chain: the scaled outputs (k_scale_outputs), window energies and the
// preview cut, per-block frame peaks, PCM decode / encode at the file boundary, and the peak count (k_peak_max,
// k_peak_count).  The kernels are device only.  The launch geometry of the grid-stride ones stands first and compiles
// under a plain host compiler as well (-DMGX_HOST_EMU: tests/emu/emu.cpp exports it, so that the lengths at which
// the tests make a grid wrap follow these numbers).
#pragma once

#include "mgx_hd.h"

namespace mgx {

constexpr int PCM_GRID_MAX = 8192;              // workgroups of k_pcm_decode / k_pcm_encode: longer files wrap (grid-stride)
constexpr int PEAK_GRID_MAX = 4096;             // ... of k_peak_max / k_peak_count
constexpr int PREVIEW_CUT_GRID_MAX = 4096;      // ... of k_preview_cut
constexpr int WINDOW_ENERGY_ROWS_MAX = 65535;   // windows of one k_window_energy launch (a grid's y extent is 16 bits)
constexpr int WINDOW_ENERGY_CHUNK_FRAMES = 16384, WINDOW_ENERGY_CHUNKS_MAX = 64;    // a window's workgroups: size / 16384, 1 .. 64

// four samples per thread, and one workgroup more for the ragged end
inline long long quad_grid(long long samples, int cap) {
    const long long blocks = (samples / 4 + 255) / 256 + 1;
    return blocks < cap ? blocks : cap;
}
inline long long pcm_grid(long long samples) { return quad_grid(samples, PCM_GRID_MAX); }
inline long long peak_grid(long long samples) { return quad_grid(samples, PEAK_GRID_MAX); }
inline long long preview_cut_grid(long long size) {
    const long long blocks = (size + 255) / 256;
    return blocks < PREVIEW_CUT_GRID_MAX ? blocks : PREVIEW_CUT_GRID_MAX;
}
inline int window_energy_chunks(long long size) {
    const long long chunks = size / WINDOW_ENERGY_CHUNK_FRAMES;
    return (int)(chunks < 1 ? 1 : (chunks > WINDOW_ENERGY_CHUNKS_MAX ? WINDOW_ENERGY_CHUNKS_MAX : chunks));
}

}  // namespace mgx

#if defined(__HIPCC__) && !defined(MGX_HOST_EMU)
#include "wave_util.h"

namespace mgx {

// result_no_limiter = y*gain (dsp.py:89-90) and/or the normalised variant
__global__ __launch_bounds__(256) void k_scale_outputs(const float2* y, long long n, const double* gain_ptr,
                                                       double gain_mul, const double* normalize_ptr,
                                                       float2* out_plain, float2* out_normalized) {
    const double g = (gain_ptr ? *gain_ptr : 1.0) * gain_mul;
    const double inv = normalize_ptr ? *normalize_ptr : 1.0;
    // two frames (16 bytes) per access where every buffer allows it; the odd last frame, if any, goes alone
    const bool wide = (((size_t)y | (size_t)out_plain | (size_t)out_normalized) & 15) == 0;
    if (!wide) {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
            const float2 v = y[i];
            const double l = (double)v.x * g, r = (double)v.y * g;
            if (out_plain) out_plain[i] = make_float2((float)l, (float)r);
            if (out_normalized) out_normalized[i] = make_float2((float)(l / inv), (float)(r / inv));
        }
        return;
    }
    const long long pairs = n >> 1;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < pairs; i += (long long)gridDim.x * 256) {
        const float4 v = reinterpret_cast<const float4*>(y)[i];
        const double a = (double)v.x * g, b = (double)v.y * g, c = (double)v.z * g, d = (double)v.w * g;
        // (plain stores: non-temporal ones measured 58 vs 54 us here)
        if (out_plain) reinterpret_cast<float4*>(out_plain)[i] = make_float4((float)a, (float)b, (float)c, (float)d);
        if (out_normalized)
            reinterpret_cast<float4*>(out_normalized)[i] =
                make_float4((float)(a / inv), (float)(b / inv), (float)(c / inv), (float)(d / inv));
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const float2 v = y[n - 1];
        const double l = (double)v.x * g, r = (double)v.y * g;
        if (out_plain) out_plain[n - 1] = make_float2((float)l, (float)r);
        if (out_normalized) out_normalized[n - 1] = make_float2((float)(l / inv), (float)(r / inv));
    }
}

// ---- A/B previews (preview_creator.py:30-94) --------------------------------------------------------
// dsp.py:128-143 strided_app_2d + batch_rms_2d: windows of `size` frames every `step` frames; the loudest one
// is argmax of sqrt(mean(x^2)) over both channels = argmax of the plain sum of squares.  grid = (chunks,
// windows): workgroup (c, w) sums chunk c of window w in float64 (float32 products are exact in float64);
// the host adds a window's chunks in order and takes the argmax of a few hundred numbers.
__global__ __launch_bounds__(256) void k_window_energy(const float2* x, long long size, long long step, int chunks,
                                                       double* partial /* [windows][chunks] */, long long first_window) {
    __shared__ double scratch[4];
    partial += (size_t)first_window * chunks;                   // (grids of at most 65535 windows each)
    const long long begin = (first_window + (long long)blockIdx.y) * step;
    const long long len = (size + chunks - 1) / chunks;
    const long long b = begin + (long long)blockIdx.x * len, e = min(begin + size, b + len);
    double acc = 0.0;
    for (long long i = b + threadIdx.x; i < e; i += 256) {
        const float2 v = x[i];
        acc = fma((double)v.x, (double)v.x, acc);
        acc = fma((double)v.y, (double)v.y, acc);
    }
    const double s = block_sum<256>(acc, scratch);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * chunks + blockIdx.x] = s;
}
// the cut: out[i] = fade(i) * clip(x[begin + i], -limit, limit) for i < size (dsp.py:109-110 clip -- limit <= 0:
// none --, dsp.py:146-152 fade: numpy.linspace(0, 1, fade) over the first `fade` frames, its mirror over the
// last `fade`; both factors where the two ramps overlap, as the reference's two in-place products give)
__global__ __launch_bounds__(256) void k_preview_cut(const float2* x, long long begin, long long size, long long fade,
                                                     double limit, float2* out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < size; i += (long long)gridDim.x * 256) {
        const float2 v = x[begin + i];
        double l = v.x, r = v.y;
        if (limit > 0.0) {
            l = fmin(fmax(l, -limit), limit);
            r = fmin(fmax(r, -limit), limit);
        }
        double g = 1.0;
        if (fade > 0) {
            const double denom = fade > 1 ? (double)(fade - 1) : 1.0;         // linspace(0, 1, 1) = [0]
            if (i < fade) g *= (double)i / denom;
            if (i >= size - fade) g *= (double)(size - 1 - i) / denom;
        }
        out[i] = make_float2((float)(l * g), (float)(r * g));
    }
}

// per-block max(|L|,|R|) of interleaved frames (4096 frames per block)
__global__ __launch_bounds__(256) void k_frame_peaks(const float2* x, long long n, float* block_peak) {
    __shared__ float scratch[4];
    const long long b = (long long)blockIdx.x * 4096;
    float m = 0.f;
    for (int i = threadIdx.x; i < 4096; i += 256) {
        const long long f = b + i;
        if (f < n) {
            const float2 v = x[f];
            m = fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y)));
        }
    }
    const float r = block_max<256>(m, scratch);
    if (threadIdx.x == 0) block_peak[blockIdx.x] = r;
}

// ---- PCM at the boundary (loader.py:35 / saver.py:27-33: what soundfile does on the host) ------------
// Files hold integer samples; moving those over PCIe instead of float32 halves (16 bit) the bytes either
// way.  Scaling follows libsndfile: read x = v / 2^(bits-1) (exact in float32 up to 24 bits), write
// v = rint(x * (2^(bits-1) - 1)) clipped to the integer range, computed in float64 so that the result is
// the one the host codec (audio_io.write_wav) produces from the same float32 sample.  24-bit samples are
// packed little-endian, three bytes each: a thread moves four of them as three 32-bit words.
__global__ __launch_bounds__(256) void k_pcm_decode(const void* pcm, long long samples, int bits, float* out) {
    const long long stride = (long long)gridDim.x * 256;
    if (bits == 16) {
        const short* in = static_cast<const short*>(pcm);
        for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < samples; i += stride * 4) {
            if (i + 4 <= samples) {
                const short4 v = *reinterpret_cast<const short4*>(in + i);
                *reinterpret_cast<float4*>(out + i) = make_float4(v.x * (1.f / 32768.f), v.y * (1.f / 32768.f),
                                                                  v.z * (1.f / 32768.f), v.w * (1.f / 32768.f));
            } else {
                for (long long k = i; k < samples; ++k) out[k] = in[k] * (1.f / 32768.f);
            }
        }
    } else if (bits == 32) {
        const int* in = static_cast<const int*>(pcm);
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < samples; i += stride)
            out[i] = (float)((double)in[i] * (1.0 / 2147483648.0));
    } else {                                     // 24 bits packed: samples 4q .. 4q+3 = bytes 12q .. 12q+11
        const unsigned* in = static_cast<const unsigned*>(pcm);
        const unsigned char* bytes = static_cast<const unsigned char*>(pcm);
        const long long quads = samples / 4;
        for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < quads; q += stride) {
            const unsigned w0 = in[3 * q], w1 = in[3 * q + 1], w2 = in[3 * q + 2];
            const int v0 = (int)(w0 << 8) >> 8;
            const int v1 = (int)(((w0 >> 24) | (w1 << 8)) << 8) >> 8;
            const int v2 = (int)(((w1 >> 16) | (w2 << 16)) << 8) >> 8;
            const int v3 = (int)w2 >> 8;
            *reinterpret_cast<float4*>(out + 4 * q) = make_float4(v0 * (1.f / 8388608.f), v1 * (1.f / 8388608.f),
                                                                  v2 * (1.f / 8388608.f), v3 * (1.f / 8388608.f));
        }
        if (blockIdx.x == 0 && threadIdx.x < (int)(samples - 4 * quads)) {
            const long long k = 4 * quads + threadIdx.x;
            const int v = (int)(((unsigned)bytes[3 * k] | ((unsigned)bytes[3 * k + 1] << 8) | ((unsigned)bytes[3 * k + 2] << 16)) << 8) >> 8;
            out[k] = v * (1.f / 8388608.f);
        }
    }
}
__device__ __forceinline__ int pcm_quantise(float x, double top) {
    const double q = rint((double)x * top);
    return (int)fmin(fmax(q, -top - 1.0), top);
}
__global__ __launch_bounds__(256) void k_pcm_encode(const float* x, long long samples, int bits, void* pcm) {
    const long long stride = (long long)gridDim.x * 256;
    const double top = (double)((1ll << (bits - 1)) - 1);
    if (bits == 16) {
        short* out = static_cast<short*>(pcm);
        for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < samples; i += stride * 4) {
            if (i + 4 <= samples) {
                const float4 v = *reinterpret_cast<const float4*>(x + i);
                short4 o;
                o.x = (short)pcm_quantise(v.x, top); o.y = (short)pcm_quantise(v.y, top);
                o.z = (short)pcm_quantise(v.z, top); o.w = (short)pcm_quantise(v.w, top);
                *reinterpret_cast<short4*>(out + i) = o;
            } else {
                for (long long k = i; k < samples; ++k) out[k] = (short)pcm_quantise(x[k], top);
            }
        }
    } else if (bits == 32) {
        int* out = static_cast<int*>(pcm);
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < samples; i += stride)
            out[i] = pcm_quantise(x[i], top);
    } else {
        unsigned* out = static_cast<unsigned*>(pcm);
        unsigned char* bytes = static_cast<unsigned char*>(pcm);
        const long long quads = samples / 4;
        for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < quads; q += stride) {
            const float4 v = *reinterpret_cast<const float4*>(x + 4 * q);
            const unsigned a = (unsigned)pcm_quantise(v.x, top) & 0xFFFFFFu, b = (unsigned)pcm_quantise(v.y, top) & 0xFFFFFFu;
            const unsigned c = (unsigned)pcm_quantise(v.z, top) & 0xFFFFFFu, d = (unsigned)pcm_quantise(v.w, top) & 0xFFFFFFu;
            out[3 * q] = a | (b << 24);
            out[3 * q + 1] = (b >> 8) | (c << 16);
            out[3 * q + 2] = (c >> 16) | (d << 8);
        }
        if (blockIdx.x == 0 && threadIdx.x < (int)(samples - 4 * quads)) {
            const long long k = 4 * quads + threadIdx.x;
            const unsigned v = (unsigned)pcm_quantise(x[k], top);
            bytes[3 * k] = (unsigned char)v; bytes[3 * k + 1] = (unsigned char)(v >> 8); bytes[3 * k + 2] = (unsigned char)(v >> 16);
        }
    }
}

// dsp.py:49-54 count_max_peaks on frames in HBM: the largest magnitude, then how many samples numpy.isclose
// would put on it (|x - m| <= 1e-8 + 1e-5 m, either sign), evaluated in float64 like numpy does on the
// float32 values.  out[0] = bits of the maximum (a non-negative float orders like its bit pattern),
// out[1] = the count; both zeroed by the caller.
__global__ __launch_bounds__(256) void k_peak_max(const float* x, long long samples, unsigned long long* out) {
    __shared__ float red[4];
    float m = 0.f;
    for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < samples; i += (long long)gridDim.x * 1024) {
        if (i + 4 <= samples) {
            const float4 v = *reinterpret_cast<const float4*>(x + i);
            m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        } else {
            for (long long k = i; k < samples; ++k) m = fmaxf(m, fabsf(x[k]));
        }
    }
    const float b = block_max<256>(m, red);
    if (threadIdx.x == 0) atomicMax(out, (unsigned long long)__float_as_uint(b));
}
__global__ __launch_bounds__(256) void k_peak_count(const float* x, long long samples, unsigned long long* out) {
    __shared__ double red[4];
    const double peak = (double)__uint_as_float((unsigned)out[0]);
    const double tol = 1e-8 + 1e-5 * peak;
    int c = 0;
    for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < samples; i += (long long)gridDim.x * 1024) {
        if (i + 4 <= samples) {
            const float4 v = *reinterpret_cast<const float4*>(x + i);
            c += (fabs(fabs((double)v.x) - peak) <= tol) + (fabs(fabs((double)v.y) - peak) <= tol) +
                 (fabs(fabs((double)v.z) - peak) <= tol) + (fabs(fabs((double)v.w) - peak) <= tol);
        } else {
            for (long long k = i; k < samples; ++k) c += fabs(fabs((double)x[k]) - peak) <= tol;
        }
    }
    const double total = block_sum<256>((double)c, red);
    if (threadIdx.x == 0 && total > 0.0) atomicAdd(out + 1, (unsigned long long)total);
}

}  // namespace mgx
#endif
