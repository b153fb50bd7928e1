// The part of libmgx.so that touches no device (mgx_policy.cpp): the calling thread's error text, the validation of a
// Config, the entry points that are arithmetic on the structs of include/mgx.h -- mgx_version, mgx_last_error,
// mgx_config_default, mgx_design_fir, mgx_loudness_gate, mgx_audit_gate, mgx_spectrogram_plan, mgx_delivery_gain, mgx_delivery_limit_step, their _shaped forms,
// mgx_noise_shaper_preset, mgx_profile_bytes, mgx_eq_shape_check, mgx_shape_fir, mgx_eq_tone_default, mgx_eq_tone_check,
// mgx_eq_tone_curve, mgx_tone_fir --
// and what the device entry points settle from their numbers alone before they touch a handle.
// No HIP here: g++ compiles the unit by itself (tests/emu/emu_policy_driver.cpp runs it under the sanitizers), and
// mgx.hip uses what is declared below.
#pragma once

#include <cstdint>
#include <string>

#include "../../include/mgx.h"
#include "fir_design.h"
#include "loudness_plan.h"
#include "noise_shaper.h"
#include "resample_plan.h"
#include "visuals_plan.h"

namespace mgx {

// what mgx_last_error returns to the calling thread: the one definition, whichever unit fails
extern thread_local std::string g_error;
int fail(int code, const std::string& msg);
#define MGX_TRY(expr)          \
    do {                       \
        int rc_ = (expr);      \
        if (rc_ != 0) return rc_; \
    } while (0)

int check_config(const mgx_config* c);
int check_length(long long n);
// the one construction of the host design's parameters from a Config (mgx_design_fir, run_fir_design)
FirDesignParams fir_design_params(const mgx_config& c);
void loudness_fill(const LoudnessGated& g, int64_t nsub, int S, mgx_loudness_report* report);
int deliver_format_check(int32_t bits, int32_t dither);

// What the device entry points of mgx.hip settle from the numbers alone, before they look at their handle or their
// pointers, each with the entry point's own codes and messages in its own order.  resample_request is mgx_resample's
// (`channels` its argument) and mgx_convert_rate's (`channels` null: resident frames are stereo) up to the output length,
// which goes to *n_out; `subject` is "the track is" / "the frames are".  loudness_request writes *count (where given)
// and *S, the frames of a sub-block, once the frame count is accepted.
int resample_request(const char* entry, const char* subject, const int32_t* channels, int64_t n, int32_t rate_in,
                     int32_t rate_out, ResampleGeometry* g, int64_t* n_out);
int loudness_request(const mgx_loudness_report* report, int64_t n, int32_t sample_rate, const double* sub_energy,
                     int64_t capacity, int64_t* count, int* S);
// mgx_audit: audit_request writes *count (where given) and *B, the frames of a sub-block, once the numbers are accepted;
// audit_clear leaves the report of a track without frames (zero counts and sums, positions -1); audit_gate is
// mgx_audit_gate behind its argument checks: the derived figures from the report's sums and `count` sub-block sums
int audit_request(const mgx_audit_limits* limits, const mgx_audit_report* report, int64_t n_frames, int32_t bits,
                  int32_t sample_rate, const double* sub_sums, int64_t capacity, int64_t* count, int* B);
void audit_clear(mgx_audit_report* report, int32_t bits);
int audit_gate(const double* sub_sums, int64_t count, int64_t n_frames, int B, mgx_audit_report* report);
// mgx_spectrogram_plan behind its name: every refusal of a spectrogram that its numbers alone decide, then the hops T,
// the columns W and the workgroups per column; overview_request the same for mgx_overview (n_frames == 0: accepted, no
// columns, *parts 0)
struct SpectroPlan {
    long long hops;
    int columns, parts;
};
int spectrogram_request(int64_t n_frames, const mgx_spectrogram_spec* spec, const int32_t* edges, SpectroPlan* plan);
int overview_request(int64_t n_frames, int32_t columns, int* parts);
int deliver_check(int64_t samples, double gain, int32_t bits, int32_t dither);
// a shaper as every entry point that takes one accepts it, and mgx_deliver_shaped's numbers
int shaper_check(const mgx_noise_shaper* shaper);
int deliver_shaped_check(int64_t n_frames, double gain, int32_t bits, const mgx_noise_shaper* shaper);
// (the ranges include/mgx.h documents; mgx.hip holds tp_limit_kernel.h's constants to them)
constexpr int TP_LIMIT_LOOKAHEAD_MAX = 2048;
constexpr double TP_LIMIT_RELEASE_MAX = 4194304.0;             // 2^22 frames
int tp_limit_check(int64_t n, double pre_gain, double ceiling, int32_t lookahead, double release);
int profile_merge_check(const void* const* profiles_dev, const int32_t* weights, int32_t count, const mgx_config* cfg,
                        const void* profile_dev);
// matching EQ controls (mgx_eq_shape): the fft_size range of the minimum-phase chain (eq_shape_kernels.h: N = 4F points
// per channel through the call's scratch), and what a shape asks of the design -- false for NULL and for a shape that
// changes nothing, which then costs no launch
constexpr int EQ_MINPHASE_FFT_MIN = 64, EQ_MINPHASE_FFT_MAX = 16384;
bool eq_shape_curve_stage(const mgx_eq_shape* shape);          // amount != 1 or a cap: k_eq_shape runs
bool eq_shape_minimum_phase(const mgx_eq_shape* shape);
// its tone controls (mgx_eq_tone): true for NULL and for a tone that asks for nothing -- the call then takes the route
// without a tone (k_eq_shape or no launch), not k_eq_tone with factors of one
bool eq_tone_neutral(const mgx_eq_tone* tone);

}  // namespace mgx
