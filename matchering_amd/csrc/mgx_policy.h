// The part of libmgx.so that touches no device (mgx_policy.cpp): the calling thread's error text, the validation of a
// Config, and the entry points that are arithmetic on the structs of include/mgx.h -- mgx_version, mgx_last_error,
// mgx_config_default, mgx_design_fir, mgx_loudness_gate, mgx_delivery_gain, mgx_delivery_limit_step, mgx_profile_bytes.
// No HIP here: g++ compiles the unit by itself (tests/emu/emu_policy_driver.cpp runs it under the sanitizers), and
// mgx.hip uses what is declared below.
#pragma once

#include <cstdint>
#include <string>

#include "../../include/mgx.h"
#include "fir_design.h"
#include "loudness_plan.h"

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

}  // namespace mgx
