// libmgx.so's device-free part (mgx_policy.h): plain C++, no HIP.
#include "mgx_policy.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <complex>
#include <cstring>
#include <memory>
#include <vector>

#include "eq_tone.h"
#include "fir_plan.h"
#include "host_params.h"

namespace mgx {

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
thread_local std::string g_error;
int fail(int code, const std::string& msg) {
    g_error = msg;
    return code;
}

// The one range check of fft_size: a power of two in [8, max].  Each caller words its refusals itself, and says with
// `code_above` whether a size above `max` is a bad argument or not implemented.
static int check_fft_size(int fft_size, int max, const char* not_a_power, const char* below, int code_above,
                          const char* above) {
    if (ilog2_exact(fft_size) < 0) return fail(MGX_ERR_ARGUMENT, not_a_power);
    if (fft_size < 8) return fail(MGX_ERR_ARGUMENT, below);
    if (fft_size > max) return fail(code_above, above);
    return 0;
}

int check_config(const mgx_config* c) {
    if (!c) return fail(MGX_ERR_ARGUMENT, "config is null");
    if (c->internal_sample_rate <= 0) return fail(MGX_ERR_ARGUMENT, "internal_sample_rate must be positive");
    /* (below 8: defaults.py:110-112 lets 2 and 4 through; match_frequencies.py:45-58 then fails) */
    MGX_TRY(check_fft_size(c->fft_size, 65536, "fft_size must be a power of two",
                           "fft_size below 8: the reference's own cubic interpolation of the matching curve "
                           "needs at least four points per side and fails there",
                           MGX_ERR_UNSUPPORTED,
                           "fft_size above 65536 is not implemented "
                           "(an analysis segment is one, two or four transforms that fit one CU's LDS)"));
    if (c->rms_correction_steps < 0) return fail(MGX_ERR_ARGUMENT, "rms_correction_steps must not be negative");
    if (c->rms_correction_steps > 4096)      /* (a flag word per round and summing workgroup: 4 MB at 4096) */
        return fail(MGX_ERR_UNSUPPORTED, "more than 4096 rms_correction_steps are not implemented");
    if (c->lowess_it < 0 || c->lowess_it > 64) return fail(MGX_ERR_ARGUMENT, "lowess_it outside [0, 64]");
    if (!(c->threshold > c->min_value && c->threshold < 1.0 && c->min_value > 0.0))
        return fail(MGX_ERR_ARGUMENT, "threshold/min_value out of range (defaults.py:93-99)");
    if (!(c->max_piece_size > c->fft_size)) return fail(MGX_ERR_ARGUMENT, "max_piece_size must exceed fft_size samples");
    return 0;
}

// Kernels address a track through a buffer view with 32-bit byte offsets (mgx_hd.h MemView): 8 bytes
// per frame plus the look-ahead of a convolution block must stay below 4 GiB.  That is 3.3 hours at
// 44.1 kHz; the reference stops at max_length = 15 minutes by default (defaults.py, checker.py:58).
int check_length(long long n) {
    const long long max_frames = (0xfffffff0ll >> 3) - (1 << 16);
    if (n > max_frames) return fail(MGX_ERR_UNSUPPORTED, "tracks longer than 536 million frames are not implemented");
    return 0;
}

FirDesignParams fir_design_params(const mgx_config& c) {
    return FirDesignParams{c.fft_size, c.internal_sample_rate, c.lin_log_oversampling, c.lowess_frac,
                           c.lowess_it, c.lowess_delta, c.min_value};
}

void loudness_fill(const LoudnessGated& g, int64_t nsub, int S, mgx_loudness_report* report) {
    report->integrated = g.integrated;
    report->range = g.range;
    report->momentary_max = g.momentary_max;
    report->short_term_max = g.short_term_max;
    report->sub_blocks = nsub;
    report->sub_block_frames = S;
    report->reserved = 0;
}

// the arguments mgx_delivery_gain and mgx_deliver share
int deliver_format_check(int32_t bits, int32_t dither) {
    if (bits != 0 && bits != 16 && bits != 24 && bits != 32)
        return fail(MGX_ERR_ARGUMENT, "bits: a delivery is float32 (0) or 16, 24 or 32-bit PCM");
    if (dither < 0 || dither > 2) return fail(MGX_ERR_ARGUMENT, "dither: 0 (none), 1 (TPDF) or 2 (high-passed TPDF)");
    if (dither != 0 && (bits == 0 || bits == 32))
        return fail(MGX_ERR_ARGUMENT, "dither: only 16 and 24-bit deliveries are dithered");
    return 0;
}

int resample_request(const char* entry, const char* subject, const int32_t* channels, int64_t n, int32_t rate_in,
                     int32_t rate_out, ResampleGeometry* g, int64_t* n_out) {
    if (!n_out) return fail(MGX_ERR_ARGUMENT, "null argument");
    if (channels && *channels != 1 && *channels != 2) return fail(MGX_ERR_ARGUMENT, "a track to convert has one or two channels");
    if (rate_in <= 0 || rate_out <= 0) return fail(MGX_ERR_ARGUMENT, "sample rates must be positive");
    if (rate_in == rate_out) return fail(MGX_ERR_ARGUMENT, std::string(subject) + " at the requested rate already");
    if (n < 0) return fail(MGX_ERR_ARGUMENT, "negative frame count");
    std::string why;
    if (resample_geometry(rate_in, rate_out, g, &why) != 0)
        return fail(MGX_ERR_UNSUPPORTED, std::string(entry) + " " + std::to_string(rate_in) + " -> " + std::to_string(rate_out) + " Hz: " + why);
    const int64_t frames = resample_length(n, rate_in, rate_out);
    if (n > RESAMPLE_FRAMES_MAX || frames > RESAMPLE_FRAMES_MAX)
        return fail(MGX_ERR_UNSUPPORTED, std::string(entry) + ": tracks of more than 500 million frames are not converted here");
    *n_out = frames;
    return 0;
}

int loudness_request(const mgx_loudness_report* report, int64_t n, int32_t sample_rate, const double* sub_energy,
                     int64_t capacity, int64_t* count, int* S) {
    if (!report) return fail(MGX_ERR_ARGUMENT, "null argument");
    if (sample_rate < LOUD_MIN_RATE) return fail(MGX_ERR_ARGUMENT, "loudness is metered at sample rates of 8000 Hz and above");
    if (n < 0) return fail(MGX_ERR_ARGUMENT, "negative frame count");
    if (n > LOUD_FRAMES_MAX) return fail(MGX_ERR_UNSUPPORTED, "mgx_loudness: tracks of more than 500 million frames are not metered here");
    *S = (sample_rate + 5) / 10;
    const int64_t nsub = n / *S;
    if (count) *count = nsub;
    if (sub_energy && capacity < nsub) return fail(MGX_ERR_ARGUMENT, "the energy array holds fewer sub-blocks than the track has");
    return 0;
}

int audit_request(const mgx_audit_limits* limits, const mgx_audit_report* report, int64_t n_frames, int32_t bits,
                  int32_t sample_rate, const double* sub_sums, int64_t capacity, int64_t* count, int* B) {
    if (!limits) return fail(MGX_ERR_ARGUMENT, "limits: null");
    if (!report) return fail(MGX_ERR_ARGUMENT, "report: null");
    if (n_frames < 0) return fail(MGX_ERR_ARGUMENT, "n_frames: negative");
    if (bits != 0 && bits != 16 && bits != 24 && bits != 32)
        return fail(MGX_ERR_ARGUMENT, "bits: the audit reads float32 (0) or 16, 24 or 32-bit PCM");
    if (sample_rate < LOUD_MIN_RATE) return fail(MGX_ERR_ARGUMENT, "sample_rate: the audit's sub-blocks are the meter's, at 8000 Hz and above");
    if (!std::isfinite(limits->clip_level) || limits->clip_level <= 0.0)
        return fail(MGX_ERR_ARGUMENT, "clip_level: must be finite and positive");
    if (limits->clip_run < 1) return fail(MGX_ERR_ARGUMENT, "clip_run: must be at least 1");
    if (!std::isfinite(limits->silence_level) || limits->silence_level < 0.0)
        return fail(MGX_ERR_ARGUMENT, "silence_level: must be finite and not negative");
    if (n_frames > LOUD_FRAMES_MAX) return fail(MGX_ERR_UNSUPPORTED, "mgx_audit: tracks of more than 500 million frames are not audited here");
    *B = (sample_rate + 5) / 10;
    const int64_t subs = (n_frames + *B - 1) / *B;
    if (count) *count = subs;
    if (sub_sums && capacity < subs) return fail(MGX_ERR_ARGUMENT, "capacity: the array holds fewer sub-blocks than the track has");
    return 0;
}

void audit_clear(mgx_audit_report* report, int32_t bits) {
    std::memset(report, 0, sizeof(*report));
    report->bits = bits;
    report->clip_first[0] = report->clip_first[1] = -1;
    report->gap_at = -1;
    report->correlation_min_at = -1;
}

int audit_gate(const double* sub_sums, int64_t count, int64_t n_frames, int B, mgx_audit_report* report) {
    report->frames = n_frames;
    report->sub_blocks = count;
    report->sub_block_frames = B;
    const double n = (double)n_frames, ll = report->sumsq[0], rr = report->sumsq[1], lr = report->sum_lr;
    for (int c = 0; c < 2; ++c) {
        report->dc[c] = n_frames > 0 ? report->sum[c] / n : NAN;
        report->rms[c] = n_frames > 0 ? std::sqrt(report->sumsq[c] / n) : NAN;
    }
    report->balance_db = rr != 0.0 ? 10.0 * std::log10(ll / rr) : NAN;
    const double both = std::sqrt(ll * rr);
    report->correlation = both != 0.0 ? lr / both : NAN;
    const double power = 2.0 * (ll + rr), mono = ll + rr + 2.0 * lr;
    report->mono_loss_db = power != 0.0 ? 10.0 * std::log10(mono > 0.0 ? mono / power : 0.0) : NAN;
    // the correlation of every window of AUDIT_GATE_WINDOW sub-blocks; a shorter track is one window
    constexpr int64_t AUDIT_GATE_WINDOW = 30;
    const int64_t width = std::min(count, AUDIT_GATE_WINDOW), windows = count > 0 ? count - width + 1 : 0;
    double least = NAN;
    int64_t least_at = -1;
    for (int64_t k = 0; k < windows; ++k) {
        double s[3] = {0.0, 0.0, 0.0};
        for (int64_t j = 0; j < width; ++j)
            for (int c = 0; c < 3; ++c) s[c] += sub_sums[(k + j) * 3 + c];
        const int64_t frames = std::min(n_frames, (k + width) * (int64_t)B) - k * (int64_t)B;
        if (!((s[0] + s[1]) / (2.0 * (double)frames) >= 1e-7) || s[0] == 0.0 || s[1] == 0.0) continue;
        const double r = s[2] / std::sqrt(s[0] * s[1]);
        if (least_at < 0 ? !std::isnan(r) : r < least) least = r, least_at = k;
    }
    report->correlation_min = least;
    report->correlation_min_at = least_at;
    return 0;
}

int spectrogram_request(int64_t n_frames, const mgx_spectrogram_spec* spec, const int32_t* edges, SpectroPlan* plan) {
    const auto num = [](long long v) { return std::to_string(v); };
    if (!spec) return fail(MGX_ERR_ARGUMENT, "spec: null");
    if (!edges) return fail(MGX_ERR_ARGUMENT, "edges: null");
    if (n_frames < 0) return fail(MGX_ERR_ARGUMENT, "n_frames: " + num(n_frames) + " is negative");
    if (spec->log2_fft < SPECTRO_LOG2_MIN || spec->log2_fft > SPECTRO_LOG2_MAX)
        return fail(MGX_ERR_ARGUMENT, "log2_fft: " + num(spec->log2_fft) + " is outside 8 .. 14");
    const int N = 1 << spec->log2_fft, half = N / 2;
    if (spec->hop < 1 || spec->hop > N)
        return fail(MGX_ERR_ARGUMENT, "hop: " + num(spec->hop) + " is outside 1 .. " + num(N));
    if (spec->channels != 0 && spec->channels != 1)
        return fail(MGX_ERR_ARGUMENT, "channels: " + num(spec->channels) + " is neither 0 (left / right) nor 1 (mid / side)");
    if (spec->bands < 1 || spec->bands > half + 1)
        return fail(MGX_ERR_ARGUMENT, "bands: " + num(spec->bands) + " is outside 1 .. " + num(half + 1));
    if (edges[0] < 0) return fail(MGX_ERR_ARGUMENT, "edges[0]: " + num(edges[0]) + " is negative");
    for (int b = 0; b < spec->bands; ++b)
        if (edges[b + 1] <= edges[b])
            return fail(MGX_ERR_ARGUMENT, "edges[" + num(b + 1) + "]: " + num(edges[b + 1]) + " does not exceed edges[" +
                                              num(b) + "] = " + num(edges[b]));
    if (edges[spec->bands] > half + 1)
        return fail(MGX_ERR_ARGUMENT, "edges[" + num(spec->bands) + "]: " + num(edges[spec->bands]) + " exceeds the " +
                                          num(half + 1) + " bins");
    if (spec->columns < 0) return fail(MGX_ERR_ARGUMENT, "columns: " + num(spec->columns) + " is negative");
    if (n_frames > VISUALS_FRAMES_MAX)
        return fail(MGX_ERR_UNSUPPORTED, "n_frames: " + num(n_frames) + " exceeds the 500 million frames a picture is made of");
    plan->hops = spectro_hops(n_frames, spec->hop);
    plan->columns = 0, plan->parts = 0;
    if (n_frames == 0) return 0;
    if (spec->columns > plan->hops)
        return fail(MGX_ERR_ARGUMENT, "columns: " + num(spec->columns) + " exceeds the " + num(plan->hops) + " hops");
    const long long W = spec->columns == 0 ? plan->hops : spec->columns;
    const long long parts = visuals_parts(plan->hops, (int)std::min<long long>(W, INT_MAX), SPECTRO_RUN_CAP);
    if (W * parts * (N + 2) * 4 > VISUALS_BYTES_MAX || W * 2 * spec->bands * 4 > VISUALS_BYTES_MAX)
        return fail(MGX_ERR_UNSUPPORTED, "columns: " + num(W) + " columns of " + num(spec->bands) + " bands at " + num(N) +
                                             " points exceed 2 GiB of spectra: ask for fewer columns");
    plan->columns = (int)W, plan->parts = (int)parts;
    return 0;
}

int overview_request(int64_t n_frames, int32_t columns, int* parts) {
    const auto num = [](long long v) { return std::to_string(v); };
    if (n_frames < 0) return fail(MGX_ERR_ARGUMENT, "n_frames: " + num(n_frames) + " is negative");
    if (n_frames > VISUALS_FRAMES_MAX)
        return fail(MGX_ERR_UNSUPPORTED, "n_frames: " + num(n_frames) + " exceeds the 500 million frames a picture is made of");
    *parts = 0;
    if (n_frames == 0) return 0;
    const long long most = std::min<long long>(n_frames, OVERVIEW_COLUMNS_MAX);
    if (columns < 1 || columns > most)
        return fail(MGX_ERR_ARGUMENT, "columns: " + num(columns) + " is outside 1 .. " + num(most));
    *parts = visuals_parts(n_frames, columns, OVERVIEW_SHARE);
    return 0;
}

int deliver_check(int64_t samples, double gain, int32_t bits, int32_t dither) {
    MGX_TRY(deliver_format_check(bits, dither));
    if (samples < 0) return fail(MGX_ERR_ARGUMENT, "samples: negative");
    if (!std::isfinite(gain)) return fail(MGX_ERR_ARGUMENT, "gain: not a finite number");
    return 0;
}

int shaper_check(const mgx_noise_shaper* shaper) {
    if (!shaper) return fail(MGX_ERR_ARGUMENT, "shaper: null");
    if (shaper->taps < 0 || shaper->taps > MGX_SHAPER_TAPS_MAX)
        return fail(MGX_ERR_ARGUMENT, "taps: outside [0, " + std::to_string(MGX_SHAPER_TAPS_MAX) + "]");
    for (int k = 0; k < shaper->taps; ++k)
        if (!std::isfinite(shaper->c[k])) return fail(MGX_ERR_ARGUMENT, "c[" + std::to_string(k + 1) + "]: not a finite number");
    return 0;
}

static int shaped_bits_check(int32_t bits) {
    if (bits != 16 && bits != 24) return fail(MGX_ERR_ARGUMENT, "bits: a noise-shaped delivery is 16 or 24-bit PCM");
    return 0;
}

int deliver_shaped_check(int64_t n_frames, double gain, int32_t bits, const mgx_noise_shaper* shaper) {
    MGX_TRY(shaped_bits_check(bits));
    MGX_TRY(shaper_check(shaper));
    if (n_frames < 0) return fail(MGX_ERR_ARGUMENT, "n_frames: negative");
    if (!std::isfinite(gain)) return fail(MGX_ERR_ARGUMENT, "gain: not a finite number");
    return check_length(n_frames);
}

// what the _shaped policy functions ask of their delivery and shaper
static int shaped_policy_check(const mgx_delivery* delivery, const mgx_noise_shaper* shaper) {
    MGX_TRY(shaper_check(shaper));
    MGX_TRY(shaped_bits_check(delivery->bits));
    if (delivery->dither != 1) return fail(MGX_ERR_ARGUMENT, "dither: a noise-shaped delivery is dithered with TPDF (1)");
    return 0;
}

int tp_limit_check(int64_t n, double pre_gain, double ceiling, int32_t lookahead, double release) {
    if (n < 0) return fail(MGX_ERR_ARGUMENT, "n: negative");
    if (!std::isfinite(pre_gain) || pre_gain <= 0.0) return fail(MGX_ERR_ARGUMENT, "pre_gain: must be finite and positive");
    if (!std::isfinite(ceiling) || ceiling <= 0.0) return fail(MGX_ERR_ARGUMENT, "ceiling: must be finite and positive");
    if (lookahead < 1 || lookahead > TP_LIMIT_LOOKAHEAD_MAX)
        return fail(MGX_ERR_ARGUMENT, "lookahead: outside [1, " + std::to_string(TP_LIMIT_LOOKAHEAD_MAX) + "] frames");
    if (!std::isfinite(release) || release < 0.0 || release > TP_LIMIT_RELEASE_MAX)
        return fail(MGX_ERR_ARGUMENT, "release: outside [0, 2^22] frames");
    if (n > LOUD_FRAMES_MAX) return fail(MGX_ERR_UNSUPPORTED, "mgx_tp_limit: tracks of more than 500 million frames are not limited here");
    return 0;
}

int profile_merge_check(const void* const* profiles_dev, const int32_t* weights, int32_t count, const mgx_config* cfg,
                        const void* profile_dev) {
    if (count < 1 || count > MGX_PROFILE_MERGE_MAX)
        return fail(MGX_ERR_ARGUMENT, "mgx_profile_merge takes 1 to " + std::to_string(MGX_PROFILE_MERGE_MAX) + " profiles, got " +
                                      std::to_string(count) + ": merge in groups, a merged profile is a source like any other");
    size_t bytes = 0;
    MGX_TRY(mgx_profile_bytes(cfg, &bytes));
    const uintptr_t out = (uintptr_t)profile_dev;
    for (int i = 0; i < count; ++i) {
        const int32_t w = weights ? weights[i] : 1;
        if (!profiles_dev[i]) return fail(MGX_ERR_ARGUMENT, "null profile at position " + std::to_string(i));
        if (w < 1 || w > 65536)
            return fail(MGX_ERR_ARGUMENT, "weight " + std::to_string(w) + " at position " + std::to_string(i) + " is outside [1, 65536]");
        const uintptr_t src = (uintptr_t)profiles_dev[i];
        if (src < out + bytes && out < src + bytes)
            return fail(MGX_ERR_ARGUMENT, "profile_dev overlaps the source at position " + std::to_string(i) +
                                          ": the merged profile needs a block of its own");
    }
    return 0;
}

// the numerator of g_peak: the linear ceiling less the quantiser's head-room (mgx_delivery_limit_step's ceiling is the same number)
// `shaper`: null for the plain quantiser, else the error feedback's (include/mgx.h: e_shaped)
static int delivery_room(const mgx_delivery* delivery, const mgx_noise_shaper* shaper, double* room_out) {
    // A: the most the meter's interpolator makes of errors of magnitude 1 -- the largest per-phase sum of |taps|
    double taps[49], A = 0.0;
    loudness_true_peak_taps(taps);
    for (int p = 0; p < 4; ++p) {
        double sum = 0.0;
        for (int k = p; k < 49; k += 4) sum += std::fabs(taps[k]);
        A = std::max(A, sum);
    }
    const double e = delivery->bits == 0 ? 0.0 : shaper ? shaper_error_lsb(*shaper) : (delivery->dither ? 1.5 : 0.5);
    const double margin = delivery->bits == 0 ? 0.0 : A * e / std::ldexp(1.0, delivery->bits - 1);
    const double room = std::pow(10.0, delivery->ceiling_dbtp / 20.0) - margin;
    if (!(room > 0.0))
        return fail(MGX_ERR_ARGUMENT, "ceiling_dbtp: lower than the quantiser's own head-room at this width");
    *room_out = room;
    return 0;
}

bool eq_shape_curve_stage(const mgx_eq_shape* shape) {
    return shape && (shape->amount != 1.0 || !std::isnan(shape->max_boost_db) || !std::isnan(shape->max_cut_db));
}
bool eq_shape_minimum_phase(const mgx_eq_shape* shape) { return shape && shape->phase == 1; }
bool eq_tone_neutral(const mgx_eq_tone* tone) {
    return !tone || (std::isnan(tone->low_hz) && std::isnan(tone->high_hz) && std::isnan(tone->side_amount) &&
                     std::isnan(tone->mono_below_hz) && tone->tilt_db_per_octave == 0.0 && tone->band_count == 0);
}

// in-place radix-2 complex transform of n = 2^k points for mgx_shape_fir: sign -1 forward, +1 inverse, unnormalised.
// Every twiddle is its own cos / sin of an exactly representable fraction of the circle.
static void shape_fft(std::vector<std::complex<double>>& a, int sign) {
    const int n = (int)a.size();
    for (int i = 1, j = 0; i < n; ++i) {
        int bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(a[i], a[j]);
    }
    const double pi = 3.14159265358979323846;
    std::vector<std::complex<double>> w(n / 2);
    for (int k = 0; k < n / 2; ++k) w[k] = std::complex<double>(std::cos(2.0 * pi * k / n), sign * std::sin(2.0 * pi * k / n));
    for (int len = 2; len <= n; len <<= 1) {
        const int half = len / 2, stride = n / len;
        for (int i = 0; i < n; i += len)
            for (int k = 0; k < half; ++k) {
                const std::complex<double> u = a[i + k], v = a[i + k + half] * w[(size_t)k * stride];
                a[i + k] = u + v;
                a[i + k + half] = u - v;
            }
    }
}

}  // namespace mgx

using namespace mgx;

// ---------------------------------------------------------------------------
// C ABI: the entry points that need no device
// ---------------------------------------------------------------------------
extern "C" {

int mgx_version(void) { return 106; }
const char* mgx_last_error(void) { return g_error.c_str(); }

int mgx_config_default(mgx_config* c) {
    if (!c) return fail(MGX_ERR_ARGUMENT, "config is null");
    std::memset(c, 0, sizeof(*c));
    c->internal_sample_rate = 44100;
    c->fft_size = 4096;
    c->lin_log_oversampling = 4;
    c->rms_correction_steps = 4;
    c->max_piece_size = 15.0 * 44100;
    c->threshold = (32768.0 - 61.0) / 32768.0;
    c->min_value = 1e-6;
    c->lowess_frac = 0.0375;
    c->lowess_it = 0;
    c->lowess_delta = 0.001;
    c->attack_ms = 1.0;
    c->hold_ms = 1.0;
    c->release_ms = 3000.0;
    c->attack_filter_coefficient = -2.0;
    c->hold_filter_order = 1;
    c->release_filter_order = 1;
    c->hold_filter_coefficient = 7.0;
    c->release_filter_coefficient = 800.0;
    return 0;
}

int mgx_design_fir(const mgx_config* cfg, const double* avg_target, const double* avg_reference, double* taps,
                   double* curve_raw, double* curve_smooth) {
    if (!cfg || !avg_target || !avg_reference || !taps) return fail(MGX_ERR_ARGUMENT, "null argument");
    const char* const refusal = "bad fft_size";                 // (no upper bound: the host design has none)
    MGX_TRY(check_fft_size(cfg->fft_size, INT_MAX, refusal, refusal, MGX_ERR_ARGUMENT, refusal));
    if (cfg->lowess_it < 0 || cfg->lowess_it > 64) return fail(MGX_ERR_ARGUMENT, "lowess_it outside [0, 64]");
    design_fir(avg_target, avg_reference, fir_design_params(*cfg), taps, curve_raw, curve_smooth);
    return 0;
}

// ---- matching EQ controls ---------------------------------------------------------
// the values of a shape, whatever the size
static int eq_shape_values(const mgx_eq_shape* shape) {
    if (!std::isfinite(shape->amount) || shape->amount < 0.0 || shape->amount > 2.0)
        return fail(MGX_ERR_ARGUMENT, "amount: outside [0, 2]");
    if (!std::isnan(shape->max_boost_db) && (std::isinf(shape->max_boost_db) || shape->max_boost_db < 0.0))
        return fail(MGX_ERR_ARGUMENT, "max_boost_db: must be finite and not negative (NaN: no cap)");
    if (!std::isnan(shape->max_cut_db) && (std::isinf(shape->max_cut_db) || shape->max_cut_db < 0.0))
        return fail(MGX_ERR_ARGUMENT, "max_cut_db: must be finite and not negative (NaN: no cap)");
    if (shape->phase != 0 && shape->phase != 1) return fail(MGX_ERR_ARGUMENT, "phase: 0 (linear) or 1 (minimum)");
    if (shape->reserved != 0) return fail(MGX_ERR_ARGUMENT, "reserved: must be 0");
    return 0;
}

int mgx_eq_shape_check(const mgx_config* cfg, const mgx_eq_shape* shape) {
    if (!cfg || !shape) return fail(MGX_ERR_ARGUMENT, "null argument");
    MGX_TRY(eq_shape_values(shape));
    if (shape->phase == 1 && (cfg->fft_size < EQ_MINPHASE_FFT_MIN || cfg->fft_size > EQ_MINPHASE_FFT_MAX))
        return fail(MGX_ERR_UNSUPPORTED, "a minimum-phase matching EQ is implemented for fft_size " + std::to_string(EQ_MINPHASE_FFT_MIN) +
                                         " to " + std::to_string(EQ_MINPHASE_FFT_MAX) + ", not " + std::to_string(cfg->fft_size));
    return 0;
}

// steps 2 and 3 of the definition on a shaped curve s[0 .. F/2] (fft_size and the shape's values are the caller's to check)
static int fir_from_shaped_curve(const mgx_config* cfg, const mgx_eq_shape* shape, const std::vector<double>& s, double* taps) {
    const int f = cfg->fft_size, half = f / 2;
    // 2. linear-phase taps: the design's own synthesis
    {
        const std::shared_ptr<FirPlanHost> plan = FirPlanHost::get(fir_design_params(*cfg));
        const FirPlanView pl = plan->view(plan->blob());
        for (int tid = 0; tid < FirDesign::T; ++tid) FirDesign::phase_taps(tid, pl, s.data(), nullptr, taps);
    }
    if (shape->phase != 1) return 0;
    // 3. minimum phase by the folded cepstrum on N = 4F points
    const int n = 4 * f;
    std::vector<std::complex<double>> x(n);
    for (int k = 0; k < f; ++k) x[k] = taps[k];
    shape_fft(x, -1);
    double top = 0.0;
    for (int m = 0; m < n; ++m) top = std::max(top, std::abs(x[m]));
    for (int m = 0; m < n; ++m) x[m] = std::log(std::max(std::abs(x[m]), 1e-9 * top));
    shape_fft(x, +1);
    for (int m = 0; m < n; ++m) {
        const double c = x[m].real() / n;
        x[m] = m == 0 || m == n / 2 ? c : (m < n / 2 ? 2.0 * c : 0.0);
    }
    shape_fft(x, -1);
    for (int m = 0; m < n; ++m) x[m] = std::exp(x[m]);
    shape_fft(x, +1);
    const double pi = 3.14159265358979323846;
    for (int j = 0; j < half; ++j) {
        const double taper = j < f / 4 ? 1.0 : 0.5 * (1.0 + std::cos(pi * (j - f / 4) / (f / 4)));
        taps[j] = 0.0;
        taps[half + j] = x[j].real() / n * taper;
    }
    return 0;
}

int mgx_shape_fir(const mgx_config* cfg, const mgx_eq_shape* shape, const double* curve_smooth, double* taps) {
    if (!cfg || !shape || !curve_smooth || !taps) return fail(MGX_ERR_ARGUMENT, "null argument");
    const char* const refusal = "bad fft_size";                 // (no upper bound, as for mgx_design_fir)
    MGX_TRY(check_fft_size(cfg->fft_size, INT_MAX, refusal, refusal, MGX_ERR_ARGUMENT, refusal));
    MGX_TRY(eq_shape_values(shape));                            // (the upper end of the size range is the device's)
    const int f = cfg->fft_size, half = f / 2;
    if (shape->phase == 1 && f < EQ_MINPHASE_FFT_MIN)
        return fail(MGX_ERR_UNSUPPORTED, "a minimum-phase matching EQ needs fft_size 64 or more, not " + std::to_string(f));
    // 1. shape
    std::vector<double> s(curve_smooth, curve_smooth + half + 1);
    if (eq_shape_curve_stage(shape)) {
        s[0] = 0.0;
        for (int k = 1; k <= half; ++k) {
            double d = shape->amount * (20.0 * std::log10(std::max(s[k], cfg->min_value)));
            if (!std::isnan(shape->max_boost_db)) d = std::min(d, shape->max_boost_db);
            if (!std::isnan(shape->max_cut_db)) d = std::max(d, -shape->max_cut_db);
            s[k] = std::pow(10.0, d / 20.0);
        }
    }
    return fir_from_shaped_curve(cfg, shape, s, taps);
}

// ---- matching EQ tone controls ----------------------------------------------------
static const mgx_eq_shape EQ_SHAPE_DEFAULT = {1.0, std::nan(""), std::nan(""), 0, 0};      // a NULL shape with a tone

int mgx_eq_tone_default(mgx_eq_tone* tone) {
    if (!tone) return fail(MGX_ERR_ARGUMENT, "tone: null");
    std::memset(tone, 0, sizeof(*tone));
    tone->low_hz = tone->high_hz = tone->side_amount = tone->mono_below_hz = std::nan("");
    tone->range_octaves = tone->mono_octaves = 1.0;
    tone->tilt_pivot_hz = 1000.0;
    return 0;
}

// the values of a tone at a sample rate
static int eq_tone_values(const mgx_config* cfg, const mgx_eq_tone* tone) {
    if (cfg->internal_sample_rate <= 0) return fail(MGX_ERR_ARGUMENT, "internal_sample_rate must be positive");
    const double nyquist = 0.5 * cfg->internal_sample_rate;
    const std::string top = " at " + std::to_string(cfg->internal_sample_rate) + " Hz";
    auto inside = [](double v, double lo, double hi) { return std::isfinite(v) && v >= lo && v <= hi; };
    if (!std::isnan(tone->low_hz) && !(std::isfinite(tone->low_hz) && tone->low_hz > 0.0 && tone->low_hz < nyquist))
        return fail(MGX_ERR_ARGUMENT, "low_hz: outside (0, fs/2)" + top + " (NaN: open)");
    if (!std::isnan(tone->high_hz) && !(std::isfinite(tone->high_hz) && tone->high_hz > 0.0 && tone->high_hz <= nyquist))
        return fail(MGX_ERR_ARGUMENT, "high_hz: outside (0, fs/2]" + top + " (NaN: open)");
    if (!std::isnan(tone->low_hz) && !std::isnan(tone->high_hz) && !(tone->low_hz < tone->high_hz))
        return fail(MGX_ERR_ARGUMENT, "low_hz: must lie below high_hz");
    if (!inside(tone->range_octaves, 0.0, 4.0)) return fail(MGX_ERR_ARGUMENT, "range_octaves: outside [0, 4]");
    if (!std::isnan(tone->side_amount) && !inside(tone->side_amount, 0.0, 2.0))
        return fail(MGX_ERR_ARGUMENT, "side_amount: outside [0, 2] (NaN: the shape's amount)");
    if (!std::isnan(tone->mono_below_hz) &&
        !(std::isfinite(tone->mono_below_hz) && tone->mono_below_hz > 0.0 && tone->mono_below_hz < nyquist))
        return fail(MGX_ERR_ARGUMENT, "mono_below_hz: outside (0, fs/2)" + top + " (NaN: off)");
    if (!inside(tone->mono_octaves, 0.0, 4.0)) return fail(MGX_ERR_ARGUMENT, "mono_octaves: outside [0, 4]");
    if (!inside(tone->tilt_db_per_octave, -6.0, 6.0)) return fail(MGX_ERR_ARGUMENT, "tilt_db_per_octave: outside [-6, 6]");
    if (!(std::isfinite(tone->tilt_pivot_hz) && tone->tilt_pivot_hz > 0.0))
        return fail(MGX_ERR_ARGUMENT, "tilt_pivot_hz: must be positive and finite");
    if (tone->band_count < 0 || tone->band_count > MGX_EQ_BANDS_MAX)
        return fail(MGX_ERR_ARGUMENT, "band_count: outside [0, " + std::to_string(MGX_EQ_BANDS_MAX) + "]");
    for (int i = 0; i < tone->band_count; ++i) {
        const mgx_eq_band& b = tone->bands[i];
        const std::string name = "bands[" + std::to_string(i) + "].";
        if (b.kind < 0 || b.kind > 2) return fail(MGX_ERR_ARGUMENT, name + "kind: 0 (bell), 1 (low shelf) or 2 (high shelf)");
        if (b.channels < 1 || b.channels > 3) return fail(MGX_ERR_ARGUMENT, name + "channels: 1 (mid), 2 (side) or 3 (both)");
        if (!(std::isfinite(b.hz) && b.hz > 0.0 && b.hz <= nyquist)) return fail(MGX_ERR_ARGUMENT, name + "hz: outside (0, fs/2]" + top);
        if (!inside(b.gain_db, -24.0, 24.0)) return fail(MGX_ERR_ARGUMENT, name + "gain_db: outside [-24, 24]");
        if (!inside(b.q, 0.1, 20.0)) return fail(MGX_ERR_ARGUMENT, name + "q: outside [0.1, 20]");
    }
    if (tone->reserved != 0) return fail(MGX_ERR_ARGUMENT, "reserved: must be 0");
    return 0;
}

int mgx_eq_tone_check(const mgx_config* cfg, const mgx_eq_shape* shape, const mgx_eq_tone* tone) {
    if (!cfg || !tone) return fail(MGX_ERR_ARGUMENT, "null argument");
    MGX_TRY(eq_tone_values(cfg, tone));
    return shape ? mgx_eq_shape_check(cfg, shape) : 0;
}

static EqToneArgs eq_tone_args(const mgx_config* cfg, const mgx_eq_shape* shape, const mgx_eq_tone* tone) {
    return EqToneArgs{shape->amount, shape->max_boost_db, shape->max_cut_db, cfg->min_value, *tone,
                      (double)cfg->internal_sample_rate, cfg->fft_size};
}

int mgx_eq_tone_curve(const mgx_config* cfg, const mgx_eq_shape* shape, const mgx_eq_tone* tone, int32_t channel,
                      double* weight_times_amount, double* trim_db, double* gate) {
    if (!cfg || !tone) return fail(MGX_ERR_ARGUMENT, "null argument");
    if (channel != 0 && channel != 1) return fail(MGX_ERR_ARGUMENT, "channel: 0 (mid) or 1 (side)");
    const char* const refusal = "bad fft_size";
    MGX_TRY(check_fft_size(cfg->fft_size, INT_MAX, refusal, refusal, MGX_ERR_ARGUMENT, refusal));
    if (!shape) shape = &EQ_SHAPE_DEFAULT;
    MGX_TRY(eq_tone_values(cfg, tone));
    MGX_TRY(eq_shape_values(shape));
    const EqToneArgs a = eq_tone_args(cfg, shape, tone);
    for (int k = 0; k <= cfg->fft_size / 2; ++k) {
        const EqToneTerms t = k == 0 ? EqToneTerms{0.0, 0.0, 0.0} : eq_tone_terms(k, channel, a);
        if (weight_times_amount) weight_times_amount[k] = t.weight_times_amount;
        if (trim_db) trim_db[k] = t.trim_db;
        if (gate) gate[k] = t.gate;
    }
    return 0;
}

int mgx_tone_fir(const mgx_config* cfg, const mgx_eq_shape* shape, const mgx_eq_tone* tone, int32_t channel,
                 const double* curve_smooth, double* taps) {
    if (!cfg || !curve_smooth || !taps) return fail(MGX_ERR_ARGUMENT, "null argument");
    if (channel != 0 && channel != 1) return fail(MGX_ERR_ARGUMENT, "channel: 0 (mid) or 1 (side)");
    if (!shape) shape = &EQ_SHAPE_DEFAULT;
    if (tone) {
        const char* const refusal = "bad fft_size";
        MGX_TRY(check_fft_size(cfg->fft_size, INT_MAX, refusal, refusal, MGX_ERR_ARGUMENT, refusal));
        MGX_TRY(eq_tone_values(cfg, tone));
    }
    if (eq_tone_neutral(tone)) return mgx_shape_fir(cfg, shape, curve_smooth, taps);      // the route without a tone
    MGX_TRY(eq_shape_values(shape));
    const int f = cfg->fft_size, half = f / 2;
    if (shape->phase == 1 && f < EQ_MINPHASE_FFT_MIN)
        return fail(MGX_ERR_UNSUPPORTED, "a minimum-phase matching EQ needs fft_size 64 or more, not " + std::to_string(f));
    // 1. the tone stage in place of the shape stage
    std::vector<double> s(curve_smooth, curve_smooth + half + 1);
    const EqToneArgs a = eq_tone_args(cfg, shape, tone);
    for (int k = 0; k <= half; ++k) eq_tone_phase(k, channel, s.data(), a);
    return fir_from_shaped_curve(cfg, shape, s, taps);
}

int mgx_loudness_gate(const double* sub_energy, int64_t count, int32_t sample_rate, mgx_loudness_report* report) {
    if (!report || count < 0 || (count > 0 && !sub_energy)) return fail(MGX_ERR_ARGUMENT, "null argument or negative count");
    if (sample_rate < LOUD_MIN_RATE) return fail(MGX_ERR_ARGUMENT, "loudness is metered at sample rates of 8000 Hz and above");
    const int S = (sample_rate + 5) / 10;
    loudness_fill(loudness_gate(sub_energy, count, S), count, S, report);
    return 0;
}

int mgx_audit_gate(const double* sub_sums, int64_t count, int64_t n_frames, int32_t sample_rate, mgx_audit_report* report) {
    if (!report) return fail(MGX_ERR_ARGUMENT, "report: null");
    if (count < 0) return fail(MGX_ERR_ARGUMENT, "count: negative");
    if (n_frames < 0) return fail(MGX_ERR_ARGUMENT, "n_frames: negative");
    if (count > 0 && !sub_sums) return fail(MGX_ERR_ARGUMENT, "sub_sums: null");
    if (sample_rate < LOUD_MIN_RATE) return fail(MGX_ERR_ARGUMENT, "sample_rate: the audit's sub-blocks are the meter's, at 8000 Hz and above");
    const int B = (sample_rate + 5) / 10;
    if (count != (n_frames + B - 1) / B)
        return fail(MGX_ERR_ARGUMENT, "count: " + std::to_string(n_frames) + " frames are " + std::to_string((n_frames + B - 1) / B) +
                                      " sub-blocks of " + std::to_string(B) + ", not " + std::to_string(count));
    return audit_gate(sub_sums, count, n_frames, B, report);
}

int mgx_declip_check(const mgx_declip_params* params) {
    if (!params) return fail(MGX_ERR_ARGUMENT, "params: null");
    if (!std::isfinite(params->level) || params->level <= 0.0) return fail(MGX_ERR_ARGUMENT, "level: must be finite and positive");
    if (!std::isfinite(params->max_rise) || params->max_rise < 1.0) return fail(MGX_ERR_ARGUMENT, "max_rise: must be finite and at least 1");
    if (params->min_run < 1) return fail(MGX_ERR_ARGUMENT, "min_run: below 1");
    if (params->max_run < params->min_run || params->max_run > MGX_DECLIP_MAX_RUN)
        return fail(MGX_ERR_ARGUMENT, "max_run: outside [min_run, " + std::to_string(MGX_DECLIP_MAX_RUN) + "]");
    return 0;
}

int mgx_spectrogram_plan(int64_t n_frames, const mgx_spectrogram_spec* spec, const int32_t* edges, int64_t* hops,
                         int32_t* columns) {
    SpectroPlan plan;
    MGX_TRY(spectrogram_request(n_frames, spec, edges, &plan));
    if (hops) *hops = plan.hops;
    if (columns) *columns = plan.columns;
    return 0;
}

// mgx_delivery_gain (shaper null) and mgx_delivery_gain_shaped
static int delivery_gain(const mgx_delivery* delivery, const mgx_noise_shaper* shaper, const mgx_loudness_report* measured,
                         mgx_delivery_result* result) {
    if (!delivery || !measured || !result) return fail(MGX_ERR_ARGUMENT, "null argument");
    MGX_TRY(deliver_format_check(delivery->bits, delivery->dither));
    const double target = delivery->target_lufs, ceiling = delivery->ceiling_dbtp;
    const double integrated = measured->integrated, peak = measured->true_peak;
    if (std::isinf(target)) return fail(MGX_ERR_ARGUMENT, "target_lufs: must be finite (NaN: no target)");
    if (std::isinf(ceiling)) return fail(MGX_ERR_ARGUMENT, "ceiling_dbtp: must be finite (NaN: no ceiling)");
    if (ceiling > 0.0) return fail(MGX_ERR_ARGUMENT, "ceiling_dbtp: a ceiling above 0 dBTP would clip");
    if (!std::isfinite(peak) || peak < 0.0) return fail(MGX_ERR_ARGUMENT, "true_peak: the measured peak is negative or not finite");
    if (std::isnan(integrated) || integrated == INFINITY)
        return fail(MGX_ERR_ARGUMENT, "integrated: the measured loudness is NaN or +infinity");
    const bool has_loud = !std::isnan(target) && std::isfinite(integrated);
    const double g_loud = has_loud ? std::pow(10.0, (target - integrated) / 20.0) : 1.0;
    double g_peak = INFINITY;
    if (!std::isnan(ceiling)) {
        double room;
        MGX_TRY(delivery_room(delivery, shaper, &room));
        if (peak > 0.0) g_peak = room / peak;
    }
    const double gain = std::min(g_loud, g_peak);
    result->gain = gain;
    result->achieved_lufs = std::isfinite(integrated) ? integrated + 20.0 * std::log10(gain) : -INFINITY;
    result->achieved_true_peak = gain * peak;
    const bool by_peak = g_peak < g_loud;
    result->shortfall_lu = by_peak && has_loud ? 20.0 * std::log10(g_loud / gain) : 0.0;
    result->limited_by = by_peak ? 2 : (has_loud ? 1 : 0);
    result->reserved = 0;
    return 0;
}

// mgx_delivery_limit_step (shaper null) and mgx_delivery_limit_step_shaped
static int delivery_limit_step(const mgx_delivery* delivery, const mgx_noise_shaper* shaper, const mgx_loudness_report* rendering,
                               int32_t passes, const double* pre_gain_db, const double* integrated, int32_t max_passes,
                               double tolerance_lu, mgx_delivery_limit_plan* next) {
    if (!delivery || !rendering || !next) return fail(MGX_ERR_ARGUMENT, "null argument");
    if (max_passes < 1 || max_passes > MGX_LIMIT_PASSES_MAX)
        return fail(MGX_ERR_ARGUMENT, "max_passes: outside [1, " + std::to_string(MGX_LIMIT_PASSES_MAX) + "]");
    if (!(tolerance_lu >= 0.0) || std::isinf(tolerance_lu)) return fail(MGX_ERR_ARGUMENT, "tolerance_lu: negative or not finite");
    if (passes < 0 || passes > max_passes) return fail(MGX_ERR_ARGUMENT, "passes: outside [0, max_passes]");
    if (passes > 0 && (!pre_gain_db || !integrated)) return fail(MGX_ERR_ARGUMENT, "pre_gain_db / integrated: null with passes run");
    if (std::isnan(delivery->ceiling_dbtp)) return fail(MGX_ERR_ARGUMENT, "ceiling_dbtp: a limiter needs a ceiling");
    mgx_delivery_result linear;
    MGX_TRY(delivery_gain(delivery, shaper, rendering, &linear));
    next->run = 0;
    next->reserved = 0;
    next->pre_gain_db = passes > 0 ? pre_gain_db[passes - 1] : 0.0;
    MGX_TRY(delivery_room(delivery, shaper, &next->ceiling));
    const double target = delivery->target_lufs;
    const bool has_target = !std::isnan(target) && std::isfinite(rendering->integrated);
    if (passes == 0) {
        if (linear.limited_by != 2) return 0;                  // the linear policy reaches what was asked for
        next->run = 1;
        next->pre_gain_db = has_target ? target - rendering->integrated : 0.0;
        return 0;
    }
    const double p = pre_gain_db[passes - 1], loud = integrated[passes - 1];
    if (std::isnan(p) || std::isnan(loud) || loud == INFINITY)
        return fail(MGX_ERR_ARGUMENT, "pre_gain_db / integrated: NaN or +infinity in the passes run");
    if (!has_target || target - loud <= tolerance_lu || passes == max_passes || std::isinf(loud)) return 0;
    double slope = 1.0;
    if (passes >= 2) {
        const double dp = p - pre_gain_db[passes - 2], dl = loud - integrated[passes - 2];
        if (dp == 0.0 || !(dl / dp >= 0.1)) return 0;           // more pre-gain buys no loudness: a steady tone under a ceiling
        slope = std::min(dl / dp, 1.0);
    }
    next->run = 1;
    next->pre_gain_db = p + (target - loud) / slope;
    return 0;
}

int mgx_delivery_gain(const mgx_delivery* delivery, const mgx_loudness_report* measured, mgx_delivery_result* result) {
    return delivery_gain(delivery, nullptr, measured, result);
}

int mgx_delivery_limit_step(const mgx_delivery* delivery, const mgx_loudness_report* rendering, int32_t passes,
                            const double* pre_gain_db, const double* integrated, int32_t max_passes, double tolerance_lu,
                            mgx_delivery_limit_plan* next) {
    return delivery_limit_step(delivery, nullptr, rendering, passes, pre_gain_db, integrated, max_passes, tolerance_lu, next);
}

// ---- noise-shaped deliveries ----------------------------------------------------
int mgx_noise_shaper_preset(int32_t id, int32_t sample_rate, mgx_noise_shaper* out) {
    if (!out) return fail(MGX_ERR_ARGUMENT, "out: null");
    for (const ShaperPreset& preset : SHAPER_PRESETS) {
        if (preset.id != id) continue;
        if (sample_rate < SHAPER_PRESET_RATE_MIN || sample_rate > SHAPER_PRESET_RATE_MAX)
            return fail(MGX_ERR_UNSUPPORTED, "sample_rate: the noise shaper '" + std::string(preset.name) + "' is designed for 44100 Hz and is handed out for " +
                                             std::to_string(SHAPER_PRESET_RATE_MIN) + " to " + std::to_string(SHAPER_PRESET_RATE_MAX) +
                                             " Hz, not " + std::to_string(sample_rate) + " Hz (custom coefficients are taken at any rate)");
        std::memset(out, 0, sizeof(*out));
        out->taps = preset.taps;
        for (int k = 0; k < preset.taps; ++k) out->c[k] = preset.c[k];
        return 0;
    }
    return fail(MGX_ERR_ARGUMENT, "id: no such noise shaper preset (1: lipshitz5, 2: wannamaker9)");
}

int mgx_delivery_gain_shaped(const mgx_delivery* delivery, const mgx_noise_shaper* shaper, const mgx_loudness_report* measured,
                             mgx_delivery_result* result) {
    if (!delivery || !measured || !result) return fail(MGX_ERR_ARGUMENT, "null argument");
    MGX_TRY(shaped_policy_check(delivery, shaper));
    return delivery_gain(delivery, shaper, measured, result);
}

int mgx_delivery_limit_step_shaped(const mgx_delivery* delivery, const mgx_noise_shaper* shaper,
                                   const mgx_loudness_report* rendering, int32_t passes, const double* pre_gain_db,
                                   const double* integrated, int32_t max_passes, double tolerance_lu,
                                   mgx_delivery_limit_plan* next) {
    if (!delivery || !rendering || !next) return fail(MGX_ERR_ARGUMENT, "null argument");
    MGX_TRY(shaped_policy_check(delivery, shaper));
    return delivery_limit_step(delivery, shaper, rendering, passes, pre_gain_db, integrated, max_passes, tolerance_lu, next);
}

// ---- reference profiles -------------------------------------------------------
int mgx_profile_bytes(const mgx_config* cfg, size_t* bytes) {
    if (!cfg || !bytes) return fail(MGX_ERR_ARGUMENT, "null argument");
    const char* const refusal = "fft_size must be a power of two in [8, 65536]";
    MGX_TRY(check_fft_size(cfg->fft_size, 65536, refusal, refusal, MGX_ERR_ARGUMENT, refusal));
    *bytes = sizeof(mgx_profile_header) + (size_t)2 * (cfg->fft_size / 2 + 1) * sizeof(double);
    return 0;
}

}  // extern "C"
