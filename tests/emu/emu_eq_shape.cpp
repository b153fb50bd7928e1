// CPU emulation of the matching EQ's device stages -- TEST INFRASTRUCTURE (tests/test_eq_emu.py, tests/test_eq_host.py).
//
// Compiled through tests/emu/build.py (the unit tests/eq_shape_emu.py registers) with a plain host compiler and
// -DMGX_HOST_EMU: the SAME per-thread phase functions k_eq_shape, k_minphase_sub and k_minphase_combine inline
// (matchering_amd/csrc/eq_shape_kernels.h), driven by loops over workgroups and thread ids in the order of the eight
// launches, a plain sequence point where the GPU has a barrier.  Not part of the product.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mgx.h"
#include "../../matchering_amd/csrc/eq_shape_kernels.h"

using namespace mgx;

// k_eq_shape on one smooth plane of `bins` values, in place
extern "C" void emu_eq_shape(double* smooth, int bins, double amount, double max_boost_db, double max_cut_db, double min_value) {
    const EqShapeArgs a{amount, max_boost_db, max_cut_db, min_value};
    for (int k = 0; k < bins; ++k) eq_shape_phase(k, smooth, a);
}

// out = {log2 M, R, threads of a sub-transform, its LDS bytes, the call's scratch bytes}
extern "C" void emu_eq_geometry(int fft, long long* out) {
    int log2m, r;
    minphase_geometry(fft, log2m, r);
    out[0] = log2m;
    out[1] = r;
    out[2] = minphase_threads(log2m);
    out[3] = (long long)minphase_lds_bytes(log2m);
    out[4] = (long long)minphase_work_bytes(fft);
}

// run_minimum_phase's eight launches on the CPU: taps [2][fft] float32, in place.  Returns R, -1 for a size outside
// [64, 16384] or not a power of two.
extern "C" int emu_eq_minphase(float* taps, int fft) {
    if (fft < 64 || fft > 16384 || (fft & (fft - 1))) return -1;
    MinPhaseArgs a;
    a.fft = fft;
    a.n = fft * MINPHASE_OVERSAMPLE;
    minphase_geometry(fft, a.log2m, a.r);
    std::vector<double2> tw(a.n);
    const double pi = 3.14159265358979323846;
    for (int j = 0; j < a.n; ++j) {
        tw[j].x = std::cos(2.0 * pi * j / a.n);
        tw[j].y = std::sin(2.0 * pi * j / a.n);
    }
    // exactly the call's scratch, carved as run_minimum_phase carves it; 0xff bytes: what an earlier call left must not matter
    std::vector<unsigned char> work(minphase_work_bytes(fft), 0xff);
    a.tw = tw.data();
    a.taps = taps;
    a.a = reinterpret_cast<double2*>(work.data());
    a.b = a.a + (size_t)2 * a.n;
    a.hmax = reinterpret_cast<unsigned long long*>(a.b + (size_t)2 * a.n);
    const int M = 1 << a.log2m, threads = minphase_threads(a.log2m);
    std::vector<unsigned char> lds(minphase_lds_bytes(a.log2m));
    double2* z = reinterpret_cast<double2*>(lds.data());
    double2* q = z + M + 64;
    for (int step = 0; step < 4; ++step) {
        for (int plane = 0; plane < 2; ++plane)
            for (int rho = 0; rho < a.r; ++rho) {
                std::memset(lds.data(), 0x7f, lds.size());
                if (step == 0 && rho == 0) a.hmax[plane] = 0ull;
                for (int t = 0; t < threads; ++t) minphase_sub_load(t, threads, plane, rho, step, a, z, q);
                int h = 1;
                if (a.log2m & 1) {
                    for (int t = 0; t < threads; ++t) minphase_sub_first(t, threads, a.log2m, z);
                    h = 2;
                }
                for (; h < M; h <<= 2)
                    for (int t = 0; t < threads; ++t) minphase_sub_pass(t, threads, a.log2m, h, z, q);
                for (int t = 0; t < threads; ++t) minphase_sub_store(t, threads, plane, rho, a, z);
            }
        for (int plane = 0; plane < 2; ++plane) {
            double top = 0.0;
            const int count = minphase_combine_count(a, step);
            for (int n = 0; n < count; ++n) top = std::max(top, minphase_combine(n, plane, step, a));
            if (step == 0) {                                   // (the kernel's atomic maximum of the bit patterns)
                unsigned long long bits;
                std::memcpy(&bits, &top, 8);
                a.hmax[plane] = std::max(a.hmax[plane], bits);
            }
        }
    }
    return a.r;
}

#ifdef EMU_EQ_SHAPE_MAIN
// A stand-alone run under the sanitizers (tests/test_eq_host.py; build.py build_driver): mgx_shape_fir, the library's
// host function, over exactly sized buffers at sizes from 8 to 4096, both phases, with and without the curve stage --
// and the emulated device chain on exactly sized taps at a size of one workgroup per channel and at a split one.
#include <cstdio>
int main() {
    mgx_config cfg;
    if (mgx_config_default(&cfg) != 0) return 1;
    const double nan = std::nan("");
    for (int fft : {8, 32, 64, 512, 4096}) {
        cfg.fft_size = fft;
        std::vector<double> smooth((size_t)fft / 2 + 1), taps((size_t)fft);          // exactly sized
        for (int k = 0; k <= fft / 2; ++k) smooth[k] = k == 0 ? 0.0 : (k % 7 == 0 ? -0.5 : 0.2 + 3.0 * std::fabs(std::sin(0.37 * k)));
        for (int phase : {0, 1})
            for (double amount : {1.0, 0.5}) {
                const mgx_eq_shape shape{amount, amount == 1.0 ? nan : 6.0, amount == 1.0 ? nan : 3.0, phase, 0};
                const int rc = mgx_shape_fir(&cfg, &shape, smooth.data(), taps.data());
                const int want = phase == 1 && fft < 64 ? MGX_ERR_UNSUPPORTED : 0;
                if (rc != want) {
                    std::printf("mgx_shape_fir(%d, %d): %d %s\n", fft, phase, rc, mgx_last_error());
                    return 1;
                }
                if (rc == 0 && !std::isfinite(taps[fft - 1])) return 1;
            }
    }
    for (int fft : {64, 1024, 2048}) {
        std::vector<float> taps((size_t)2 * fft);                                    // exactly sized
        for (int i = 0; i < 2 * fft; ++i) taps[i] = (float)std::exp(-0.01 * std::abs(i % fft - fft / 2)) * ((i & 1) ? 0.5f : 1.0f);
        if (emu_eq_minphase(taps.data(), fft) < 1) return 1;
        for (int plane = 0; plane < 2; ++plane)
            if (taps[(size_t)plane * fft] != 0.f || !(std::fabs(taps[(size_t)plane * fft + fft / 2]) > 0.f)) return 1;
    }
    std::puts("ok");
    return 0;
}
#endif
