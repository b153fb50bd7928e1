// CPU emulation of the noise-shaped delivery kernel -- TEST INFRASTRUCTURE (tests/test_deliver_shaped_host.py).
//
// Compiled through tests/emu/build.py (the unit tests/deliver_shaped_emu.py registers) with a plain host compiler and
// -DMGX_HOST_EMU: the launch as mgx_deliver_shaped fills it (deliver_shaped_launch, shaped_grid) and the SAME per-thread
// phase functions k_deliver_shaped inlines (matchering_amd/csrc/deliver_shaped_kernel.h), driven by a loop over
// workgroups and thread ids, a plain sequence point where the GPU has a barrier.  Not part of the product.
#include <cstring>
#include <vector>

#include "../../include/mgx.h"
#include "../../matchering_amd/csrc/deliver_shaped_kernel.h"

using namespace mgx;

// out = {B, W, tile segments, step frames, threads, LDS bytes, chains of a workgroup}
extern "C" void emu_deliver_shaped_constants(long long* out) {
    out[0] = MGX_SHAPER_SEGMENT;
    out[1] = MGX_SHAPER_WARMUP;
    out[2] = SHAPED_SEGMENTS;
    out[3] = SHAPED_STEP;
    out[4] = SHAPED_THREADS;
    out[5] = (long long)SHAPED_LDS_BYTES;
    out[6] = SHAPED_CHAINS;
}

// The launch of mgx_deliver_shaped on the CPU.  `segment` <= 0: the library's B and W; otherwise that segment and
// warm-up (multiples of the step: a test runs one chain over the whole track to have the sequential filter).  out holds
// exactly 2 n samples.  Returns the grid, -1 for a geometry the kernel does not take.
extern "C" long long emu_deliver_shaped(const float* x, long long frames, double gain, int bits, int taps, const double* c,
                                        unsigned long long seed, void* out, int segment, int warmup) {
    if (segment <= 0) segment = MGX_SHAPER_SEGMENT, warmup = MGX_SHAPER_WARMUP;
    if (segment % SHAPED_STEP || warmup % SHAPED_STEP || warmup < 0 || taps < 0 || taps > SHAPED_TAPS_MAX) return -1;
    if (frames <= 0) return 0;
    DeliverShapedArgs a;
    deliver_shaped_launch(a, frames, gain, bits, taps, c, segment, warmup, seed);
    a.x = x;
    a.out = out;
    const long long grid = shaped_grid(frames, segment);
    const int steps = shaped_steps(segment, warmup);
    std::vector<ShapedSlot> lds(SHAPED_LDS_BYTES / sizeof(ShapedSlot));
    std::vector<ShapedThread> th(SHAPED_THREADS);
    for (long long tile = 0; tile < grid; ++tile) {
        std::memset(lds.data(), 0x7f, SHAPED_LDS_BYTES);                 // (what a previous workgroup left behind must not matter)
        for (int t = 0; t < SHAPED_THREADS; ++t) shaped_start(th[t]);
        for (int step = 0; step < steps; ++step) {
            for (int t = 0; t < SHAPED_THREADS; ++t) shaped_fill(a, tile, step, lds.data(), t);
            for (int t = 0; t < SHAPED_THREADS; ++t) shaped_run(a, lds.data(), t, th[t]);
            for (int t = 0; t < SHAPED_THREADS; ++t) shaped_store(a, tile, step, lds.data(), t);
        }
    }
    return grid;
}

#ifdef EMU_DELIVER_SHAPED_MAIN
// A stand-alone run of the emulation under the sanitizers (tests/test_deliver_shaped_driver_host.py; build.py
// build_driver): both widths, every tap count's edge, the sizes around a warm-up, a segment and a tile, exactly sized
// buffers.
#include <cstdio>
int main() {
    const long long B = MGX_SHAPER_SEGMENT, W = MGX_SHAPER_WARMUP;
    const long long sizes[] = {1, 2, 3, W - 1, W, W + 1, B - 1, B, B + 1, B + W + 1, 3 * B + 7, SHAPED_SEGMENTS * B + B + 1};
    const int widths[] = {16, 24};
    const int tapses[] = {0, 1, 5, 9, 16};
    double c[SHAPED_TAPS_MAX];
    for (int k = 0; k < SHAPED_TAPS_MAX; ++k) c[k] = (k % 2 ? -0.9 : 1.1) / (k + 1);
    for (long long n : sizes)
        for (int bits : widths)
            for (int taps : tapses) {
                std::vector<float> x((size_t)n * 2);                             // exactly sized: one byte past either end is found
                std::vector<unsigned char> exact((size_t)n * 2 * (bits / 8));
                for (long long i = 0; i < 2 * n; ++i) x[i] = (float)((i * 37 % 201) - 100) / 90.0f;
                if (emu_deliver_shaped(x.data(), n, 0.3701, bits, taps, c, (1ull << 40) + 3, exact.data(), 0, 0) < 1) return 1;
            }
    std::puts("ok");
    return 0;
}
#endif
