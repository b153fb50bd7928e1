// CPU emulation of the matching EQ's tone stage -- TEST INFRASTRUCTURE (tests/test_eq_tone_emu.py, tests/test_eq_tone_host.py).
//
// Compiled through tests/emu/build.py (the unit tests/eq_tone_emu.py registers) with a plain host compiler and
// -DMGX_HOST_EMU: the SAME per-thread phase function k_eq_tone inlines (matchering_amd/csrc/eq_tone.h), driven by a loop
// over the launch's grid, (ceil(bins / 256), 2) workgroups of 256 threads.  Not part of the product.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/mgx.h"
#include "../../matchering_amd/csrc/eq_tone.h"

using namespace mgx;

// k_eq_tone on the two smooth planes ([2][bins], bins = fft / 2 + 1), in place, as run_fir_design launches it.
// shape NULL: amount 1, no caps.
extern "C" void emu_eq_tone(double* planes, int fft, double sample_rate, double min_value, const mgx_eq_shape* shape,
                            const mgx_eq_tone* tone) {
    const int bins = fft / 2 + 1;
    const double nan = std::nan("");
    const EqToneArgs a{shape ? shape->amount : 1.0, shape ? shape->max_boost_db : nan, shape ? shape->max_cut_db : nan,
                       min_value, *tone, sample_rate, fft};
    for (int plane = 0; plane < 2; ++plane)
        for (int block = 0; block < (bins + 255) / 256; ++block)
            for (int thread = 0; thread < 256; ++thread) {
                const int k = block * 256 + thread;
                if (k >= bins) continue;
                eq_tone_phase(k, plane, planes + (size_t)plane * bins, a);
            }
}

extern "C" int emu_eq_tone_sizeof(void) { return (int)sizeof(mgx_eq_tone); }

#ifdef EMU_EQ_TONE_MAIN
// A stand-alone run under the sanitizers (tests/test_eq_tone_host.py; build.py build_driver): the library's host entry
// points mgx_eq_tone_check, mgx_eq_tone_curve and mgx_tone_fir (csrc/mgx_policy.cpp) over exactly sized buffers, sizes
// 8 to 4096, both channels and phases, every control set -- and the emulated stage on exactly sized planes.
static int fail_at(const char* what, int fft, int rc) {
    std::printf("%s(%d): %d %s\n", what, fft, rc, mgx_last_error());
    return 1;
}
int main() {
    mgx_config cfg;
    if (mgx_config_default(&cfg) != 0) return 1;
    mgx_eq_tone tone;
    if (mgx_eq_tone_default(&tone) != 0) return 1;
    const double nan = std::nan("");
    if (mgx_eq_tone_check(&cfg, nullptr, &tone) != 0) return fail_at("mgx_eq_tone_check", cfg.fft_size, -1);
    tone.low_hz = 60.0;
    tone.high_hz = 12000.0;
    tone.side_amount = 0.25;
    tone.mono_below_hz = 120.0;
    tone.tilt_db_per_octave = -0.5;
    tone.band_count = MGX_EQ_BANDS_MAX;
    for (int i = 0; i < MGX_EQ_BANDS_MAX; ++i)
        tone.bands[i] = mgx_eq_band{i % 3, 1 + i % 3, 40.0 * std::pow(2.2, i), i % 2 ? 3.0 : -4.5, 0.3 + 0.6 * i};
    for (int fft : {8, 32, 64, 512, 4096}) {
        cfg.fft_size = fft;
        const size_t bins = (size_t)fft / 2 + 1;
        std::vector<double> smooth(bins), taps((size_t)fft), w(bins), t(bins), g(bins);             // exactly sized
        for (size_t k = 0; k < bins; ++k) smooth[k] = k == 0 ? 0.0 : (k % 7 == 0 ? -0.5 : 0.2 + 3.0 * std::fabs(std::sin(0.37 * k)));
        for (int phase : {0, 1}) {
            const mgx_eq_shape shape{0.5, 6.0, nan, phase, 0};
            const int unsupported = phase == 1 && fft < 64;
            int rc = mgx_eq_tone_check(&cfg, &shape, &tone);
            if (rc != (unsupported ? MGX_ERR_UNSUPPORTED : 0)) return fail_at("mgx_eq_tone_check", fft, rc);
            for (int channel : {0, 1}) {
                rc = mgx_eq_tone_curve(&cfg, &shape, &tone, channel, w.data(), t.data(), g.data());
                if (rc != 0) return fail_at("mgx_eq_tone_curve", fft, rc);
                if (w[0] != 0.0 || !std::isfinite(t[bins - 1]) || !(g[bins - 1] == 1.0)) return fail_at("terms", fft, 0);
                rc = mgx_tone_fir(&cfg, &shape, &tone, channel, smooth.data(), taps.data());
                if (rc != (unsupported ? MGX_ERR_UNSUPPORTED : 0)) return fail_at("mgx_tone_fir", fft, rc);
                if (rc == 0 && !std::isfinite(taps[(size_t)fft - 1])) return fail_at("taps", fft, 0);
            }
        }
        std::vector<double> planes(2 * bins);                                                      // exactly sized
        for (size_t k = 0; k < 2 * bins; ++k) planes[k] = 0.5 + (double)(k % 5);
        emu_eq_tone(planes.data(), fft, cfg.internal_sample_rate, cfg.min_value, nullptr, &tone);
        if (planes[0] != 0.0 || planes[bins] != 0.0 || !std::isfinite(planes[2 * bins - 1])) return fail_at("emu_eq_tone", fft, 0);
    }
    tone.bands[3].q = 0.01;
    if (mgx_eq_tone_check(&cfg, nullptr, &tone) != MGX_ERR_ARGUMENT) return fail_at("bands[3].q accepted", cfg.fft_size, 0);
    std::puts("ok");
    return 0;
}
#endif
