// csrc/mgx_policy.cpp -- the entry points of libmgx.so that touch no device -- in a program of its own, for sanitizer
// builds (tests/test_policy_host.py; tests/emu/build.py, unit "policy").  It walks the edges the Python tests
// name, states the value it expects at each, prints one line per group and exits non-zero when any differs.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../matchering_amd/csrc/mgx_policy.h"

using namespace mgx;

static int g_checks = 0, g_wrong = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        ++g_checks;                                                   \
        if (!(cond)) {                                                \
            ++g_wrong;                                                \
            std::printf("  line %d: %s\n", __LINE__, #cond);          \
        }                                                             \
    } while (0)

static bool close_to(double a, double b, double tol = 1e-12) { return std::fabs(a - b) <= tol * std::fmax(1.0, std::fabs(b)); }
static bool refused(int rc, const char* field) { return rc == MGX_ERR_ARGUMENT && std::strstr(mgx_last_error(), field); }

static int group_done(const char* name) {
    static int checks_before = 0, wrong_before = 0;
    const int checks = g_checks - checks_before, wrong = g_wrong - wrong_before;
    checks_before = g_checks;
    wrong_before = g_wrong;
    std::printf("%s: %d checks, %d wrong\n", name, checks, wrong);
    return wrong;
}

// ---- check_config at each bound --------------------------------------------------------------------------------------
static void config_bounds() {
    mgx_config c;
    EXPECT(mgx_config_default(nullptr) == MGX_ERR_ARGUMENT);
    EXPECT(mgx_config_default(&c) == 0 && c.fft_size == 4096 && c.internal_sample_rate == 44100 && c.reserved0 == 0);
    EXPECT(check_config(&c) == 0);
    EXPECT(check_config(nullptr) == MGX_ERR_ARGUMENT);
    EXPECT(mgx_version() == 106);
    auto with = [&](auto set) {
        mgx_config v;
        mgx_config_default(&v);
        set(v);
        return check_config(&v);
    };
    EXPECT(with([](mgx_config& v) { v.internal_sample_rate = 1; }) == 0);
    EXPECT(refused(with([](mgx_config& v) { v.internal_sample_rate = 0; }), "internal_sample_rate"));
    EXPECT(with([](mgx_config& v) { v.fft_size = 8; }) == 0);
    EXPECT(with([](mgx_config& v) { v.fft_size = 65536; v.max_piece_size = 65537.0; }) == 0);
    EXPECT(refused(with([](mgx_config& v) { v.fft_size = 4; }), "fft_size below 8"));
    EXPECT(refused(with([](mgx_config& v) { v.fft_size = 4095; }), "power of two"));
    EXPECT(refused(with([](mgx_config& v) { v.fft_size = 0; }), "power of two"));
    EXPECT(refused(with([](mgx_config& v) { v.fft_size = -8; }), "power of two"));
    EXPECT(with([](mgx_config& v) { v.fft_size = 131072; v.max_piece_size = 1e6; }) == MGX_ERR_UNSUPPORTED);
    EXPECT(std::strstr(mgx_last_error(), "fft_size above 65536"));
    EXPECT(with([](mgx_config& v) { v.rms_correction_steps = 0; }) == 0);
    EXPECT(with([](mgx_config& v) { v.rms_correction_steps = 4096; }) == 0);
    EXPECT(refused(with([](mgx_config& v) { v.rms_correction_steps = -1; }), "rms_correction_steps"));
    EXPECT(with([](mgx_config& v) { v.rms_correction_steps = 4097; }) == MGX_ERR_UNSUPPORTED);
    EXPECT(with([](mgx_config& v) { v.lowess_it = 64; }) == 0);
    EXPECT(refused(with([](mgx_config& v) { v.lowess_it = 65; }), "lowess_it"));
    EXPECT(refused(with([](mgx_config& v) { v.lowess_it = -1; }), "lowess_it"));
    EXPECT(refused(with([](mgx_config& v) { v.threshold = 1.0; }), "threshold"));
    EXPECT(refused(with([](mgx_config& v) { v.threshold = v.min_value; }), "threshold"));
    EXPECT(refused(with([](mgx_config& v) { v.min_value = 0.0; }), "min_value"));
    EXPECT(refused(with([](mgx_config& v) { v.threshold = NAN; }), "threshold"));
    EXPECT(with([](mgx_config& v) { v.max_piece_size = 4097.0; }) == 0);
    EXPECT(refused(with([](mgx_config& v) { v.max_piece_size = 4096.0; }), "max_piece_size"));
    // (536 million frames: (0xfffffff0 >> 3) - 65536 = 536870910 - 65536)
    EXPECT(check_length(536805374) == 0 && check_length(536805375) == MGX_ERR_UNSUPPORTED);
    size_t bytes = 0;
    mgx_config_default(&c);
    EXPECT(mgx_profile_bytes(&c, &bytes) == 0 && bytes == sizeof(mgx_profile_header) + 2 * 2049 * sizeof(double));
    c.fft_size = 131072;
    EXPECT(refused(mgx_profile_bytes(&c, &bytes), "[8, 65536]"));
    c.fft_size = 4;
    EXPECT(refused(mgx_profile_bytes(&c, &bytes), "[8, 65536]"));
    EXPECT(mgx_profile_bytes(nullptr, &bytes) == MGX_ERR_ARGUMENT && mgx_profile_bytes(&c, nullptr) == MGX_ERR_ARGUMENT);
}

// ---- mgx_delivery_gain -----------------------------------------------------------------------------------------------
static mgx_delivery delivery(double target, double ceiling, int bits, int dither) {
    mgx_delivery d;
    std::memset(&d, 0, sizeof d);
    d.target_lufs = target;
    d.ceiling_dbtp = ceiling;
    d.bits = bits;
    d.dither = dither;
    return d;
}
static mgx_loudness_report measured(double integrated, double true_peak) {
    mgx_loudness_report r;
    std::memset(&r, 0, sizeof r);
    r.integrated = integrated;
    r.true_peak = true_peak;
    return r;
}
static int gain(double target, double ceiling, int bits, int dither, double integrated, double peak, mgx_delivery_result* out) {
    const mgx_delivery d = delivery(target, ceiling, bits, dither);
    const mgx_loudness_report r = measured(integrated, peak);
    return mgx_delivery_gain(&d, &r, out);
}

static void delivery_gain() {
    mgx_delivery_result out;
    const mgx_delivery d = delivery(-14.0, -1.0, 16, 0);
    const mgx_loudness_report r = measured(-14.0, 0.5);
    EXPECT(mgx_delivery_gain(nullptr, &r, &out) == MGX_ERR_ARGUMENT && mgx_delivery_gain(&d, nullptr, &out) == MGX_ERR_ARGUMENT &&
           mgx_delivery_gain(&d, &r, nullptr) == MGX_ERR_ARGUMENT);
    // every refusal names its field
    EXPECT(refused(gain(NAN, 0.5, 16, 0, -14.0, 0.5, &out), "ceiling_dbtp"));             // above 0 dBTP
    EXPECT(refused(gain(NAN, -100.0, 16, 1, -14.0, 0.5, &out), "ceiling_dbtp"));          // under the quantiser's head-room
    EXPECT(refused(gain(NAN, -INFINITY, 16, 0, -14.0, 0.5, &out), "ceiling_dbtp"));
    EXPECT(refused(gain(NAN, INFINITY, 16, 0, -14.0, 0.5, &out), "ceiling_dbtp"));
    EXPECT(refused(gain(INFINITY, NAN, 16, 0, -14.0, 0.5, &out), "target_lufs"));
    EXPECT(refused(gain(-INFINITY, NAN, 16, 0, -14.0, 0.5, &out), "target_lufs"));
    for (int bits : {8, 20, -16, 64}) EXPECT(refused(gain(-14.0, NAN, bits, 0, -14.0, 0.5, &out), "bits"));
    EXPECT(refused(gain(-14.0, NAN, 0, 1, -14.0, 0.5, &out), "dither"));
    EXPECT(refused(gain(-14.0, NAN, 32, 2, -14.0, 0.5, &out), "dither"));
    EXPECT(refused(gain(-14.0, NAN, 16, 3, -14.0, 0.5, &out), "dither"));
    EXPECT(refused(gain(-14.0, NAN, 16, -1, -14.0, 0.5, &out), "dither"));
    EXPECT(refused(gain(-14.0, NAN, 16, 0, -14.0, INFINITY, &out), "true_peak"));
    EXPECT(refused(gain(-14.0, NAN, 16, 0, -14.0, NAN, &out), "true_peak"));
    EXPECT(refused(gain(-14.0, NAN, 16, 0, -14.0, -0.5, &out), "true_peak"));
    EXPECT(refused(gain(-14.0, NAN, 16, 0, NAN, 0.5, &out), "integrated"));
    EXPECT(refused(gain(-14.0, NAN, 16, 0, INFINITY, 0.5, &out), "integrated"));
    // every format that is accepted
    for (int bits : {0, 16, 24, 32})
        for (int dither : {0, 1, 2})
            if (dither == 0 || bits == 16 || bits == 24) EXPECT(gain(-14.0, -1.0, bits, dither, -20.0, 0.1, &out) == 0);
    // target only: +6 dB to -14 LUFS
    EXPECT(gain(-14.0, NAN, 24, 0, -20.0, 0.5, &out) == 0 && close_to(out.gain, std::pow(10.0, 0.3)) && out.limited_by == 1 &&
           out.shortfall_lu == 0.0 && close_to(out.achieved_lufs, -14.0) && close_to(out.achieved_true_peak, 0.5 * std::pow(10.0, 0.3)));
    // float output has no quantiser: the ceiling itself
    EXPECT(gain(NAN, -2.0, 0, 0, -14.0, 1.0, &out) == 0 && close_to(out.gain, std::pow(10.0, -0.1)) && out.limited_by == 2);
    // the ceiling does not bind; nothing asked for; silence
    EXPECT(gain(NAN, -1.0, 16, 1, -9.0, 0.3, &out) == 0 && out.gain == 1.0 && out.limited_by == 0 && out.achieved_lufs == -9.0);
    EXPECT(gain(NAN, NAN, 16, 0, -14.0, 0.5, &out) == 0 && out.gain == 1.0 && out.limited_by == 0);
    EXPECT(gain(-14.0, -1.0, 16, 0, -INFINITY, 0.0, &out) == 0 && out.gain == 1.0 && out.achieved_lufs == -INFINITY &&
           out.limited_by == 0 && out.shortfall_lu == 0.0);
    // both, the ceiling binding: the shortfall is what is missing to the target
    EXPECT(gain(-9.0, -1.0, 24, 0, -14.0, 0.8, &out) == 0 && out.limited_by == 2 && out.gain < std::pow(10.0, -0.05) / 0.8 &&
           close_to(out.shortfall_lu, -9.0 - out.achieved_lufs) && out.shortfall_lu > 3.0);
}

// ---- mgx_delivery_limit_step -----------------------------------------------------------------------------------------
static int step(double target, double ceiling, int bits, double integrated0, double peak0, int passes, const double* pre,
                const double* loud, int max_passes, double tolerance, mgx_delivery_limit_plan* plan) {
    const mgx_delivery d = delivery(target, ceiling, bits, 0);
    const mgx_loudness_report r = measured(integrated0, peak0);
    return mgx_delivery_limit_step(&d, &r, passes, pre, loud, max_passes, tolerance, plan);
}

static void delivery_limit_step() {
    mgx_delivery_limit_plan plan;
    const double room = std::pow(10.0, -0.05);                   // -1 dBTP, float output: no head-room
    EXPECT(mgx_delivery_limit_step(nullptr, nullptr, 0, nullptr, nullptr, 4, 0.1, nullptr) == MGX_ERR_ARGUMENT);
    // the refusals
    EXPECT(refused(step(-9.0, NAN, 0, -14.0, 1.0, 0, nullptr, nullptr, 4, 0.1, &plan), "ceiling_dbtp"));
    EXPECT(refused(step(-9.0, -1.0, 0, -14.0, 1.0, 0, nullptr, nullptr, 0, 0.1, &plan), "max_passes"));
    EXPECT(refused(step(-9.0, -1.0, 0, -14.0, 1.0, 0, nullptr, nullptr, MGX_LIMIT_PASSES_MAX + 1, 0.1, &plan), "max_passes"));
    EXPECT(refused(step(-9.0, -1.0, 0, -14.0, 1.0, 0, nullptr, nullptr, 4, -0.1, &plan), "tolerance_lu"));
    EXPECT(refused(step(-9.0, -1.0, 0, -14.0, 1.0, 0, nullptr, nullptr, 4, NAN, &plan), "tolerance_lu"));
    EXPECT(refused(step(-9.0, -1.0, 0, -14.0, 1.0, 0, nullptr, nullptr, 4, INFINITY, &plan), "tolerance_lu"));
    EXPECT(refused(step(-9.0, -1.0, 0, -14.0, 1.0, -1, nullptr, nullptr, 4, 0.1, &plan), "passes"));
    EXPECT(refused(step(-9.0, -1.0, 0, -14.0, 1.0, 1, nullptr, nullptr, 4, 0.1, &plan), "null with passes run"));
    {
        // arrays of exactly `passes` entries: a read past them is the sanitizer's to find
        const std::vector<double> five(5, 1.0), loud5(5, -10.0);
        EXPECT(refused(step(-9.0, -1.0, 0, -14.0, 1.0, 5, five.data(), loud5.data(), 4, 0.1, &plan), "passes"));
        const std::vector<double> nan1(1, NAN), inf1(1, INFINITY), one(1, 1.0), loud1(1, -10.0);
        EXPECT(refused(step(-9.0, -1.0, 0, -14.0, 1.0, 1, nan1.data(), loud1.data(), 4, 0.1, &plan), "NaN or +infinity"));
        EXPECT(refused(step(-9.0, -1.0, 0, -14.0, 1.0, 1, one.data(), inf1.data(), 4, 0.1, &plan), "NaN or +infinity"));
        EXPECT(refused(step(-9.0, -1.0, 0, -14.0, 1.0, 1, one.data(), nan1.data(), 4, 0.1, &plan), "NaN or +infinity"));
    }
    // mgx_delivery_gain's own, through the step
    EXPECT(refused(step(-9.0, -1.0, 20, -14.0, 1.0, 0, nullptr, nullptr, 4, 0.1, &plan), "bits"));
    EXPECT(refused(step(-9.0, 1.0, 0, -14.0, 1.0, 0, nullptr, nullptr, 4, 0.1, &plan), "ceiling_dbtp"));
    EXPECT(refused(step(INFINITY, -1.0, 0, -14.0, 1.0, 0, nullptr, nullptr, 4, 0.1, &plan), "target_lufs"));
    EXPECT(refused(step(-9.0, -1.0, 0, NAN, 1.0, 0, nullptr, nullptr, 4, 0.1, &plan), "integrated"));
    // passes == 0: the ceiling does not bind -> no pass; it binds -> p1 = T - I0; no target -> 0
    EXPECT(step(-14.0, -1.0, 0, -10.0, 0.5, 0, nullptr, nullptr, 4, 0.1, &plan) == 0 && plan.run == 0 && plan.pre_gain_db == 0.0 &&
           close_to(plan.ceiling, room));
    EXPECT(step(-9.0, -1.0, 0, -14.0, 1.0, 0, nullptr, nullptr, 4, 0.1, &plan) == 0 && plan.run == 1 && plan.pre_gain_db == 5.0 &&
           close_to(plan.ceiling, room));
    EXPECT(step(NAN, -1.0, 0, -12.0, 1.2, 0, nullptr, nullptr, 4, 0.1, &plan) == 0 && plan.run == 1 && plan.pre_gain_db == 0.0);
    // passes == 1: slope 1 -> p2 = p1 + (T - L1); within the tolerance -> done, the last pre-gain kept
    {
        const std::vector<double> pre{5.0}, loud{-10.5}, near{-9.08}, gone{-INFINITY};
        EXPECT(step(-9.0, -1.0, 0, -14.0, 1.0, 1, pre.data(), loud.data(), 4, 0.1, &plan) == 0 && plan.run == 1 && plan.pre_gain_db == 6.5);
        EXPECT(step(-9.0, -1.0, 0, -14.0, 1.0, 1, pre.data(), near.data(), 4, 0.1, &plan) == 0 && plan.run == 0 && plan.pre_gain_db == 5.0);
        EXPECT(step(-9.0, -1.0, 0, -14.0, 1.0, 1, pre.data(), gone.data(), 4, 0.1, &plan) == 0 && plan.run == 0);
        EXPECT(step(-9.0, -1.0, 0, -14.0, 1.0, 1, pre.data(), loud.data(), 1, 0.1, &plan) == 0 && plan.run == 0);       // passes == max_passes
    }
    // passes == 2: slope 0.6 / 1.5 = 0.4 -> p3 = 6.5 + 0.9 / 0.4; a zero and a negative slope end it; so does dp == 0
    {
        const std::vector<double> pre{5.0, 6.5}, loud{-10.5, -9.9}, flat{-10.5, -10.5}, down{-10.5, -10.8}, same{5.0, 5.0};
        EXPECT(step(-9.0, -1.0, 0, -14.0, 1.0, 2, pre.data(), loud.data(), 4, 0.1, &plan) == 0 && plan.run == 1 &&
               close_to(plan.pre_gain_db, 8.75));
        EXPECT(step(-9.0, -1.0, 0, -14.0, 1.0, 2, pre.data(), flat.data(), 4, 0.1, &plan) == 0 && plan.run == 0 && plan.pre_gain_db == 6.5);
        EXPECT(step(-9.0, -1.0, 0, -14.0, 1.0, 2, pre.data(), down.data(), 4, 0.1, &plan) == 0 && plan.run == 0 && plan.pre_gain_db == 6.5);
        EXPECT(step(-9.0, -1.0, 0, -14.0, 1.0, 2, same.data(), loud.data(), 4, 0.1, &plan) == 0 && plan.run == 0);
        EXPECT(step(-9.0, -1.0, 0, -14.0, 1.0, 2, pre.data(), loud.data(), 2, 0.1, &plan) == 0 && plan.run == 0);      // passes == max_passes
    }
    // passes == max_passes at the most the library takes, with arrays of exactly that many entries
    {
        std::vector<double> pre(MGX_LIMIT_PASSES_MAX), loud(MGX_LIMIT_PASSES_MAX);
        for (int i = 0; i < MGX_LIMIT_PASSES_MAX; ++i) {
            pre[i] = 5.0 + 0.1 * i;
            loud[i] = -12.0 + 0.05 * i;
        }
        EXPECT(step(-9.0, -1.0, 0, -14.0, 1.0, MGX_LIMIT_PASSES_MAX, pre.data(), loud.data(), MGX_LIMIT_PASSES_MAX, 0.1, &plan) == 0 &&
               plan.run == 0 && plan.pre_gain_db == pre.back());
        // one short of it: slope 0.5 -> the last pre-gain + (T - L) / 0.5
        EXPECT(step(-9.0, -1.0, 0, -14.0, 1.0, MGX_LIMIT_PASSES_MAX - 1, pre.data(), loud.data(), MGX_LIMIT_PASSES_MAX, 0.1, &plan) == 0 &&
               plan.run == 1 && close_to(plan.pre_gain_db, pre[MGX_LIMIT_PASSES_MAX - 2] + (-9.0 - loud[MGX_LIMIT_PASSES_MAX - 2]) / 0.5, 1e-9));
    }
}

// ---- mgx_loudness_gate -----------------------------------------------------------------------------------------------
static void loudness_gate_edges() {
    mgx_loudness_report r;
    const int rate = 44100, S = 4410;
    auto empty = [&](const mgx_loudness_report& v, int64_t count) {
        return v.integrated == -INFINITY && v.momentary_max == -INFINITY && v.short_term_max == -INFINITY && v.range == 0.0 &&
               v.sub_blocks == count && v.sub_block_frames == S && v.reserved == 0;
    };
    std::memset(&r, 0xff, sizeof r);
    EXPECT(mgx_loudness_gate(nullptr, 0, rate, &r) == 0 && empty(r, 0));
    EXPECT(mgx_loudness_gate(nullptr, 3, rate, &r) == MGX_ERR_ARGUMENT && mgx_loudness_gate(nullptr, -1, rate, &r) == MGX_ERR_ARGUMENT);
    EXPECT(refused(mgx_loudness_gate(nullptr, 0, 7999, &r), "8000 Hz"));
    EXPECT(mgx_loudness_gate(nullptr, 0, 8000, &r) == 0 && r.sub_block_frames == 800);
    // energies in arrays of exactly [count][2]: one sub-block, then fewer than a momentary window (4) -- no block at all
    for (int count : {1, 3}) {
        const std::vector<double> e((size_t)count * 2, 0.25 * S);
        EXPECT(mgx_loudness_gate(e.data(), count, rate, nullptr) == MGX_ERR_ARGUMENT);
        EXPECT(mgx_loudness_gate(e.data(), count, rate, &r) == 0 && empty(r, count));
    }
    // exactly one momentary window, mean square 0.25 per channel: -0.691 + 10 log10(0.5); no short-term block (3 s) yet
    {
        const std::vector<double> e(8, 0.25 * S);
        const double want = -0.691 + 10.0 * std::log10(0.5);
        EXPECT(mgx_loudness_gate(e.data(), 4, rate, &r) == 0 && close_to(r.integrated, want) && close_to(r.momentary_max, want) &&
               r.short_term_max == -INFINITY && r.range == 0.0 && r.sub_blocks == 4);
    }
    // 30 sub-blocks: one short-term block; a constant level has no range
    {
        const std::vector<double> e(60, 0.25 * S);
        const double want = -0.691 + 10.0 * std::log10(0.5);
        EXPECT(mgx_loudness_gate(e.data(), 30, rate, &r) == 0 && close_to(r.integrated, want) && close_to(r.short_term_max, want) &&
               r.range == 0.0);
    }
}

// ---- mgx_design_fir --------------------------------------------------------------------------------------------------
static void design_fir_sizes() {
    mgx_config c;
    mgx_config_default(&c);
    std::vector<double> one(1, 1.0);
    EXPECT(mgx_design_fir(nullptr, one.data(), one.data(), one.data(), nullptr, nullptr) == MGX_ERR_ARGUMENT);
    EXPECT(mgx_design_fir(&c, one.data(), one.data(), nullptr, nullptr, nullptr) == MGX_ERR_ARGUMENT);
    c.fft_size = 4;
    EXPECT(refused(mgx_design_fir(&c, one.data(), one.data(), one.data(), nullptr, nullptr), "bad fft_size"));
    c.fft_size = 4097;
    EXPECT(refused(mgx_design_fir(&c, one.data(), one.data(), one.data(), nullptr, nullptr), "bad fft_size"));
    c.fft_size = 8;
    c.lowess_it = 65;
    EXPECT(refused(mgx_design_fir(&c, one.data(), one.data(), one.data(), nullptr, nullptr), "lowess_it"));
    for (int fft : {8, 4096}) {
        mgx_config_default(&c);
        c.fft_size = fft;
        const int bins = fft / 2 + 1;
        // buffers of exactly the documented sizes, on the heap: F/2 + 1 per spectrum and curve, F taps
        std::vector<double> target(bins), reference(bins), taps(fft), raw(bins), smooth(bins), taps_direct(fft), raw_direct(bins),
            smooth_direct(bins), taps_only(fft);
        for (int k = 0; k < bins; ++k) {
            target[k] = 1.0 + 0.5 * std::sin(0.37 * k);
            reference[k] = 2.0 * target[k];                      // the matching curve is 2 at every bin
        }
        EXPECT(mgx_design_fir(&c, target.data(), reference.data(), taps.data(), raw.data(), smooth.data()) == 0);
        EXPECT(mgx_design_fir(&c, target.data(), reference.data(), taps_only.data(), nullptr, nullptr) == 0);
        EXPECT(taps_only == taps);
        bool flat = true, finite = true;
        for (int k = 0; k < bins; ++k) flat = flat && close_to(raw[k], 2.0);
        for (double v : taps) finite = finite && std::isfinite(v);
        for (double v : smooth) finite = finite && std::isfinite(v);
        EXPECT(flat && finite);
        // the plan against the design written out step by step (fir_design.h): equal to float64 rounding
        design_fir_direct(target.data(), reference.data(), fir_design_params(c), taps_direct.data(), raw_direct.data(),
                          smooth_direct.data());
        double worst = 0.0, scale = 0.0;
        for (int i = 0; i < fft; ++i) {
            worst = std::fmax(worst, std::fabs(taps[i] - taps_direct[i]));
            scale = std::fmax(scale, std::fabs(taps_direct[i]));
        }
        EXPECT(worst <= 1e-9 * scale && scale > 0.0);
    }
}

// ---- resample_request: what mgx_resample and mgx_convert_rate settle before they look at their handle ----------------
static bool unsupported(int rc, const char* fragment) { return rc == MGX_ERR_UNSUPPORTED && std::strstr(mgx_last_error(), fragment); }

static void resample_request_bounds() {
    ResampleGeometry g;
    int64_t n_out = -7;
    auto track = [&](int32_t channels, int64_t n, int32_t in, int32_t out) {
        return resample_request("mgx_resample", "the track is", &channels, n, in, out, &g, &n_out);
    };
    auto frames = [&](int64_t n, int32_t in, int32_t out) {
        return resample_request("mgx_convert_rate", "the frames are", nullptr, n, in, out, &g, &n_out);
    };
    EXPECT(refused(resample_request("mgx_resample", "the track is", nullptr, 1000, 48000, 44100, &g, nullptr), "null argument"));
    // channels: one or two, and no argument of mgx_convert_rate
    EXPECT(refused(track(0, 1000, 48000, 44100), "one or two channels") && refused(track(3, 1000, 48000, 44100), "one or two channels"));
    EXPECT(track(1, 1000, 48000, 44100) == 0 && n_out == 918 && track(2, 1000, 48000, 44100) == 0 && n_out == 918);
    EXPECT(g.L == 147 && g.M == 160 && g.W == 140);
    // the channels are looked at first, then the rates, then the frame count
    n_out = -7;
    EXPECT(refused(track(3, -1, 0, 0), "one or two channels") && refused(track(2, -1, 0, 0), "must be positive"));
    EXPECT(refused(track(2, -1, 44100, 44100), "the track is at the requested rate already"));
    EXPECT(refused(frames(-1, 44100, 44100), "the frames are at the requested rate already"));
    // rates: positive
    EXPECT(refused(frames(1000, 0, 44100), "must be positive") && refused(frames(1000, 48000, 0), "must be positive"));
    EXPECT(refused(frames(1000, -48000, 44100), "must be positive") && refused(frames(1000, 48000, -1), "must be positive"));
    EXPECT(n_out == -7);                                            // nothing reported so far
    EXPECT(frames(1000, 1, 2) == 0 && n_out == 2000 && frames(1000, 2, 1) == 0 && n_out == 500);
    // the frame count: not negative
    EXPECT(refused(frames(-1, 48000, 44100), "negative frame count"));
    EXPECT(frames(0, 48000, 44100) == 0 && n_out == 0 && frames(1, 48000, 44100) == 0 && n_out == 0 && frames(2, 48000, 44100) == 0 && n_out == 1);
    // the plan's refusals name the entry and both rates: 4096 phases are the last accepted
    n_out = -7;
    EXPECT(unsupported(frames(1000, 4096, 4097), "mgx_convert_rate 4096 -> 4097 Hz: ") && std::strstr(mgx_last_error(), "more than 4096 phases"));
    EXPECT(unsupported(track(2, 1000, 4096, 4097), "mgx_resample 4096 -> 4097 Hz: ") && n_out == -7);
    EXPECT(frames(1000, 4097, 4096) == 0 && n_out == 999 && g.L == 4096 && g.M == 4097);
    // 500 million frames, in and out
    n_out = -7;
    EXPECT(frames(500000000, 48000, 44100) == 0 && n_out == 459375000);
    EXPECT(unsupported(frames(500000001, 48000, 44100), "mgx_convert_rate: tracks of more than 500 million frames"));
    EXPECT(frames(250000000, 1, 2) == 0 && n_out == 500000000);
    EXPECT(unsupported(track(1, 250000001, 1, 2), "mgx_resample: tracks of more than 500 million frames") && n_out == 500000000);
}

// ---- the ranges mgx_tp_limit, mgx_loudness, mgx_deliver and mgx_profile_merge check before their handle -----------------
static void stage_checks() {
    // mgx_tp_limit(n, pre_gain, ceiling, lookahead, release)
    const double big = 1.7976931348623157e308, tiny = 5e-324, above = std::nextafter(TP_LIMIT_RELEASE_MAX, INFINITY);
    const auto tp = tp_limit_check;
    EXPECT(tp(0, tiny, tiny, 1, 0.0) == 0 && tp(500000000, big, big, 2048, 4194304.0) == 0);
    EXPECT(refused(tp(-1, 0.0, 0.0, 0, -1.0), "n: negative"));
    EXPECT(refused(tp(1, 0.0, 0.5, 1, 0.0), "pre_gain") && refused(tp(1, INFINITY, 0.5, 1, 0.0), "pre_gain") && refused(tp(1, NAN, 0.5, 1, 0.0), "pre_gain"));
    EXPECT(refused(tp(1, 1.0, 0.0, 1, 0.0), "ceiling") && refused(tp(1, 1.0, INFINITY, 1, 0.0), "ceiling") && refused(tp(1, 1.0, NAN, 1, 0.0), "ceiling"));
    EXPECT(refused(tp(1, 1.0, 0.5, 0, 0.0), "lookahead: outside [1, 2048]") && refused(tp(1, 1.0, 0.5, 2049, 0.0), "lookahead: outside [1, 2048]"));
    EXPECT(refused(tp(1, 1.0, 0.5, 1, -tiny), "release: outside [0, 2^22]") && refused(tp(1, 1.0, 0.5, 1, above), "release: outside [0, 2^22]") &&
           refused(tp(1, 1.0, 0.5, 1, NAN), "release"));
    // (the length is looked at last, and is "not implemented", not a bad argument)
    EXPECT(unsupported(tp(500000001, 1.0, 0.5, 1, 0.0), "mgx_tp_limit: tracks of more than 500 million frames") &&
           refused(tp(500000001, 1.0, 0.5, 1, -1.0), "release"));

    // mgx_loudness(report, n, sample_rate, sub_energy, capacity, count) -> S
    mgx_loudness_report report;
    const double somewhere = 0.0;
    int64_t count = -7;
    int S = -7;
    auto loud = [&](int64_t n, int rate, const double* e = nullptr, int64_t capacity = 0) {
        return loudness_request(&report, n, rate, e, capacity, &count, &S);
    };
    EXPECT(refused(loudness_request(nullptr, 10, 44100, nullptr, 0, &count, &S), "null argument") && refused(loud(10, 7999), "8000 Hz") &&
           refused(loud(-1, 44100), "negative frame count") && count == -7 && S == -7);
    EXPECT(loud(10, 8000) == 0 && S == 800 && count == 0 && loudness_request(&report, 0, 44100, nullptr, 0, nullptr, &S) == 0 && S == 4410);
    EXPECT(loud(4409, 44100) == 0 && count == 0 && loud(4410, 44100) == 0 && count == 1);
    EXPECT(loud(44100, 44104) == 0 && S == 4410 && loud(44100, 44105) == 0 && S == 4411 && count == 9);
    EXPECT(loud(500000000, 44100) == 0 && count == 113378);
    EXPECT(unsupported(loud(500000001, 44100), "mgx_loudness: tracks of more than 500 million frames") && count == 113378);
    // an energy array that is too short is refused once the count has been reported; without an array no capacity is asked
    EXPECT(refused(loud(44100, 44100, &somewhere, 9), "fewer sub-blocks") && count == 10);
    EXPECT(loud(44100, 44100, &somewhere, 10) == 0 && loud(44100, 44100, nullptr, -1) == 0);

    // mgx_deliver(samples, gain, bits, dither): the format first
    EXPECT(deliver_check(0, 1.0, 16, 1) == 0 && deliver_check(1, -big, 0, 0) == 0 && deliver_check(7, 0.0, 32, 0) == 0);
    EXPECT(refused(deliver_check(-1, 1.0, 24, 2), "samples: negative") && refused(deliver_check(-1, NAN, 20, 0), "bits"));
    EXPECT(refused(deliver_check(-1, NAN, 16, 3), "dither") && refused(deliver_check(-1, NAN, 32, 1), "dither") && refused(deliver_check(-1, NAN, 16, 0), "samples"));
    EXPECT(refused(deliver_check(4, INFINITY, 16, 0), "gain: not a finite number") && refused(deliver_check(4, -INFINITY, 16, 0), "gain") &&
           refused(deliver_check(4, NAN, 16, 0), "gain"));

    // mgx_profile_merge(profiles, weights, count, cfg, profile): blocks of `bytes` inside one arena, never read
    mgx_config c;
    mgx_config_default(&c);
    size_t bytes = 0;
    EXPECT(mgx_profile_bytes(&c, &bytes) == 0 && bytes > 0);
    std::vector<char> arena(3 * bytes);
    const char* base = arena.data();
    // (arrays of exactly `count` entries: a read past them is the sanitizer's to find)
    auto merge = [&](const std::vector<const void*>& src, const std::vector<int32_t>& w, const char* out, const mgx_config* cfg = nullptr) {
        return profile_merge_check(src.data(), w.empty() ? nullptr : w.data(), (int32_t)src.size(), cfg ? cfg : &c, out);
    };
    const std::vector<const void*> one{base}, behind{base + bytes};
    EXPECT(refused(merge({}, {}, base + bytes), "takes 1 to 64 profiles, got 0"));
    EXPECT(merge(one, {}, base + bytes) == 0 && merge(one, {1}, base + bytes) == 0 && merge(one, {65536}, base + bytes) == 0);
    EXPECT(refused(merge(one, {0}, base + bytes), "weight 0 at position 0") && refused(merge(one, {65537}, base + bytes), "weight 65537 at position 0"));
    // the merged profile's block may touch a source's, not overlap it -- from either side
    EXPECT(refused(merge(one, {}, base + bytes - 1), "overlaps the source at position 0") && refused(merge(one, {}, base), "overlaps the source at position 0"));
    EXPECT(merge(behind, {}, base) == 0 && refused(merge(behind, {}, base + 1), "overlaps the source at position 0"));
    mgx_config bad = c;
    bad.fft_size = 4095;
    EXPECT(refused(merge(one, {}, base + bytes, &bad), "[8, 65536]"));
    std::vector<const void*> most(MGX_PROFILE_MERGE_MAX, base);
    std::vector<int32_t> weights(MGX_PROFILE_MERGE_MAX, 3);
    EXPECT(merge(most, weights, base + 2 * bytes) == 0);
    EXPECT(refused(merge(std::vector<const void*>(MGX_PROFILE_MERGE_MAX + 1, base), {}, base + 2 * bytes), "got 65"));
    most.back() = nullptr, weights.back() = 0;                  // (the null source is met before its weight)
    EXPECT(refused(merge(most, weights, base + 2 * bytes), "null profile at position 63"));
    most.back() = base + bytes + 1;
    EXPECT(refused(merge(most, {}, base + 2 * bytes), "overlaps the source at position 63"));
}

int main() {
    int wrong = 0;
    config_bounds();
    wrong += group_done("check_config");
    delivery_gain();
    wrong += group_done("mgx_delivery_gain");
    delivery_limit_step();
    wrong += group_done("mgx_delivery_limit_step");
    loudness_gate_edges();
    wrong += group_done("mgx_loudness_gate");
    design_fir_sizes();
    wrong += group_done("mgx_design_fir");
    resample_request_bounds();
    wrong += group_done("resample_request");
    stage_checks();
    wrong += group_done("stage_checks");
    return wrong ? 1 : 0;
}
