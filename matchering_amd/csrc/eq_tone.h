// Matching EQ tone controls (include/mgx.h, mgx_eq_tone): the definition's per-bin terms and the stage's per-thread phase
// function.  No kernel here: mgx_policy.cpp evaluates the same functions on the host (mgx_eq_tone_curve, mgx_tone_fir),
// eq_tone_kernels.h wraps them in k_eq_tone, tests/emu/emu_eq_tone.cpp drives them under -DMGX_HOST_EMU, and
// tests/eq_tone_oracle.py restates them in numpy.
#pragma once

#include "../../include/mgx.h"
#include "mgx_hd.h"

namespace mgx {

struct EqToneArgs {
    double amount;                           // the matching part's: EqShapeArgs' four (eq_shape_kernels.h)
    double max_boost_db, max_cut_db;         // NaN: no cap
    double min_value;
    mgx_eq_tone tone;                        // by value: no pointers
    double sample_rate;                      // fs
    int fft;                                 // F
};

struct EqToneTerms {
    double weight_times_amount;              // a * w
    double trim_db;                          // t
    double gate;                             // g
};

MGX_HD bool eq_tone_given(double v) { return v == v; }            // not NaN
MGX_HD double eq_tone_ramp(double x) {
    if (x <= 0.0) return 0.0;
    if (x >= 1.0) return 1.0;
    return 0.5 - 0.5 * cos(3.14159265358979323846 * x);
}
MGX_HD double eq_tone_edge(double f, double f0, double w) {
    if (w == 0.0) return f >= f0 ? 1.0 : 0.0;
    return eq_tone_ramp(log2(f / f0) / w + 0.5);
}
MGX_HD double eq_tone_band(const mgx_eq_band& b, double f) {
    if (b.kind == 0) {
        const double x = b.q * (f / b.hz - b.hz / f);
        return b.gain_db / (1.0 + x * x);
    }
    const double ratio = b.kind == 1 ? f / b.hz : b.hz / f;
    return b.gain_db / (1.0 + pow(ratio, 4.0 * b.q));
}

// the terms of bin k >= 1 of channel `plane` (0 mid, 1 side)
MGX_HD EqToneTerms eq_tone_terms(int k, int plane, const EqToneArgs& a) {
    const mgx_eq_tone& t = a.tone;
    const double f = ((double)k * a.sample_rate) / (double)a.fft;
    double w = 1.0;
    if (eq_tone_given(t.low_hz)) w = eq_tone_edge(f, t.low_hz, t.range_octaves);
    if (eq_tone_given(t.high_hz)) w = w * (1.0 - eq_tone_edge(f, t.high_hz, t.range_octaves));
    const double amount = plane == 1 && eq_tone_given(t.side_amount) ? t.side_amount : a.amount;
    EqToneTerms out;
    out.weight_times_amount = amount * w;
    double trim = t.tilt_db_per_octave * log2(f / t.tilt_pivot_hz);
    for (int i = 0; i < t.band_count && i < MGX_EQ_BANDS_MAX; ++i)
        if (t.bands[i].channels & (1 << plane)) trim += eq_tone_band(t.bands[i], f);
    out.trim_db = trim;
    out.gate = plane == 1 && eq_tone_given(t.mono_below_hz) ? eq_tone_edge(f, t.mono_below_hz, t.mono_octaves) : 1.0;
    return out;
}

// bin k of one smooth plane, in place; bin 0 stays 0.  With a tone that sets nothing but side_amount = amount the bits
// are eq_shape_phase's: a * 1, d + 0 and * 1 change none.
MGX_HD void eq_tone_phase(int k, int plane, double* smooth, const EqToneArgs& a) {
    if (k == 0) {
        smooth[0] = 0.0;
        return;
    }
    const EqToneTerms t = eq_tone_terms(k, plane, a);
    double d = t.weight_times_amount * (20.0 * log10(fmax(smooth[k], a.min_value)));
    if (a.max_boost_db == a.max_boost_db) d = fmin(d, a.max_boost_db);
    if (a.max_cut_db == a.max_cut_db) d = fmax(d, -a.max_cut_db);
    smooth[k] = pow(10.0, (d + t.trim_db) / 20.0) * t.gate;
}

}  // namespace mgx
