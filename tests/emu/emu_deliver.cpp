// CPU emulation of the delivery kernel -- TEST INFRASTRUCTURE (tests/test_delivery_host.py).
//
// Compiled by tests/emu/build.py ("deliver") with a plain host compiler and -DMGX_HOST_EMU: the launch as mgx_deliver
// fills it (deliver_launch, deliver_grid) and the SAME per-thread body k_deliver inlines
// (matchering_amd/csrc/deliver_kernel.h), driven by a loop over workgroups and thread ids.  Not part of the product.
#include "../../matchering_amd/csrc/deliver_kernel.h"

using namespace mgx;

extern "C" void emu_philox(const unsigned* counter, const unsigned* key, unsigned* out) {
    philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1], out);
}

// the grid mgx_deliver launches for `samples` samples
extern "C" long long emu_deliver_grid(long long samples) { return deliver_grid(samples); }

// The launch of mgx_deliver on the CPU with `grid` workgroups (0: the grid the library launches).  x and out must be
// 16-byte aligned, as on the device.  Returns the grid.
extern "C" long long emu_deliver(const float* x, long long samples, double gain, int bits, int dither,
                                 unsigned long long seed, void* out, long long grid) {
    DeliverArgs a;
    deliver_launch(a, samples, gain, bits, dither, seed);
    a.x = x;
    a.out = out;
    if (grid <= 0) grid = deliver_grid(samples);
    for (long long b = 0; b < grid; ++b)
        for (int t = 0; t < DELIVER_THREADS; ++t) deliver_thread(a, b, t, grid);
    return grid;
}

#ifdef EMU_DELIVER_MAIN
// A stand-alone run of the emulation under the sanitizers (tests/test_emu_drivers_host.py; build.py build_driver):
// every width and dither at a few ragged sizes, exactly sized buffers.
#include <cstdio>
#include <cstdlib>
int main() {
    const long long sizes[] = {1, 2, 3, 4, 6, 1022, 1024, 1026, 200006};
    const int widths[] = {0, 16, 24, 32};
    for (long long n : sizes)
        for (int bits : widths)
            for (int dither = 0; dither < 3; ++dither) {
                if (dither && (bits == 0 || bits == 32)) continue;
                const size_t bytes = (size_t)n * (bits ? bits / 8 : 4);
                float* x = (float*)aligned_alloc(16, ((size_t)n * 4 + 15) / 16 * 16);
                void* out = aligned_alloc(16, (bytes + 15) / 16 * 16);
                for (long long i = 0; i < n; ++i) x[i] = (float)((i * 37 % 201) - 100) / 90.0f;
                emu_deliver(x, n, 0.3701, bits, dither, (1ull << 40) + 3, out, n > 4096 ? 3 : 0);
                free(x);
                free(out);
            }
    std::puts("ok");
    return 0;
}
#endif
