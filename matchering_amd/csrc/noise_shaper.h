// The noise shapers of the deliveries (include/mgx.h, mgx_noise_shaper): the one table of presets and what the policy
// needs of a shaper's coefficients.  Host only, plain C++: mgx_policy.cpp uses it, mgx.hip through mgx_policy.h.
#pragma once

#include <cmath>

#include "../../include/mgx.h"

namespace mgx {

struct ShaperPreset {
    int id;
    const char* name;
    int taps;
    double c[MGX_SHAPER_TAPS_MAX];
};

// Published error-feedback coefficients for 44.1 kHz, H(z) = 1 - sum c[k] z^-k:
//   1  S. Lipshitz, J. Vanderkooy, R. Wannamaker, "Minimally audible noise shaping", JAES 39 (1991), 5 taps
//   2  R. Wannamaker, "Psychoacoustically optimal noise shaping", JAES 40 (1992), F-weighted, 9 taps
constexpr ShaperPreset SHAPER_PRESETS[] = {
    {1, "lipshitz5", 5, {2.033, -2.165, 1.959, -1.590, 0.6149}},
    {2, "wannamaker9", 9, {2.412, -3.370, 3.937, -4.174, 3.353, -2.205, 1.281, -0.569, 0.0847}},
};
constexpr int SHAPER_PRESET_RATE_MIN = 44100, SHAPER_PRESET_RATE_MAX = 48000;

// the factor over (3/2)(1 + sum |c|) that covers the recurrence's float64 roundings
constexpr double SHAPER_SLACK = 1.0 + 1.0 / 1048576.0;

// sum_k |c[k]| in tap order
inline double shaper_sum_abs(const mgx_noise_shaper& s) {
    double sum = 0.0;
    for (int k = 0; k < s.taps; ++k) sum += std::fabs(s.c[k]);
    return sum;
}

// e_shaped: the most the shaped quantiser moves a sample that does not clip, in LSB
inline double shaper_error_lsb(const mgx_noise_shaper& s) { return 1.5 * (1.0 + shaper_sum_abs(s)) * SHAPER_SLACK; }

}  // namespace mgx
