// Host plan of the loudness meter (ITU-R BS.1770-4 integrated loudness and true peak, EBU Tech 3341 momentary and
// short-term loudness, EBU Tech 3342 loudness range) -- tests/loudness_oracle.py is the numpy / scipy form.
//
// K-weighting at sample rate fs is two biquads in cascade per channel, a high shelf and a high-pass, run as
// scipy.signal.lfilter runs them (transposed direct form II, float64, zero state at frame 0):
//     y  = b0 x + s1;      s1 = s2 + b1 x - a1 y;      s2 = b2 x - a2 y           (shelf; then the same on y with c, d)
// The four state words z = (s1, s2, t1, t2) of a channel move by z' = A z + B x, so a run of R frames acts on the state
// it meets as z -> A^R z + v with v the state the run leaves from zero: k_loudness (loudness_kernel.h) gives each
// thread R frames and composes the runs of a tile by an ordered scan that needs P = A^R and P^2, P^4, ... only.
// A workgroup starts `warmup` frames before the sub-blocks it owns with state zero: what the true state there would
// still contribute is at most ||A^warmup|| <= 1e-12 of it.  (rho^k <= 1e-12, rho the largest pole modulus, is reached a quarter
// sooner, but the high-pass's near-double pole leaves A^k far above rho^k there.)
//
// A sub-block is S = (fs + 5) / 10 frames (100 ms); e[s][c] is the sum of y^2 over sub-block s of channel c.  The
// gating below works on those sums alone.  No GPU code here: g++ compiles this file for the CPU emulation
// (tests/emu/emu_loudness.cpp).
#pragma once

#include <cstdint>
#include <vector>

namespace mgx {

constexpr int LOUD_THREADS = 256;                               // threads of a workgroup of k_loudness
constexpr int LOUD_RUN = 16;                                    // consecutive frames per thread, as in the limiter
constexpr int LOUD_TILE = LOUD_THREADS * LOUD_RUN;              // frames a workgroup holds in LDS at a time
constexpr int LOUD_SCAN_STEPS = 8;                              // log2(LOUD_THREADS): P^(2^k), k = 0 .. 7
constexpr int LOUD_OWN = 12;                                    // sub-blocks a workgroup owns at most (1.2 s; the warm-up is 13 % at 44.1 kHz)
constexpr int LOUD_WORKGROUPS = 400;                            // ... and fewer on a track too short to give this many workgroups
constexpr int LOUD_OWN_MAX = 32;                                // ... and the most the kernel's LDS accumulators hold
constexpr int LOUD_MIN_RATE = 8000;                             // S >= 800: a tile of 4096 frames meets at most 7 sub-blocks
constexpr int LOUD_TILE_SUBS = 8;
constexpr int LOUD_TP_TAPS = 12;                                // taps of each of the three oversampled phases
constexpr int LOUD_TP_BEFORE = 5, LOUD_TP_AFTER = 6;            // frames before / behind frame m its phases read
constexpr int64_t LOUD_FRAMES_MAX = 500000000;                  // 32-bit byte offsets, as everywhere in the library

// the table the kernel reads: the taps of phases 1..3, tp[p - 1][i] multiplying x[m + LOUD_TP_AFTER - i], then the
// LOUD_SCAN_STEPS matrices P^(2^k), row-major 4 x 4
constexpr int LOUD_TABLE_TAPS = 0, LOUD_TABLE_POWERS = 3 * LOUD_TP_TAPS;
constexpr int LOUD_TABLE_DOUBLES = LOUD_TABLE_POWERS + LOUD_SCAN_STEPS * 16;

struct LoudnessGeometry {
    int S = 0;                  // frames of a sub-block
    int64_t nsub = 0;           // whole sub-blocks of the track
    int warmup = 0;             // H
    int own = 0;                // sub-blocks per workgroup: ceil(nsub / LOUD_WORKGROUPS) within [1, LOUD_OWN]
    int64_t workgroups = 0;     // max(1, ceil(nsub / own)): the last one also takes the n % S frames behind the last sub-block
};

struct LoudnessPlan {
    int rate = 0;
    double c[10];               // shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2
    double A[16], B[4];         // z' = A z + B x, z = (s1, s2, t1, t2), row-major
    double rho = 0.0;           // largest pole modulus
    int warmup_poles = 0;       // ceil(ln 1e-12 / ln rho): 5089 frames at 44.1 kHz, 22156 at 192 kHz
    int warmup = 0;             // H: the first k >= warmup_poles with ||A^k|| <= 1e-12 (largest row sum)
    std::vector<double> table;  // LOUD_TABLE_DOUBLES
};

// the closed-form K-weighting coefficients at `rate` (BS.1770-4's tables at 48 kHz), A, B, the powers and the taps
LoudnessPlan loudness_design(int rate);
LoudnessGeometry loudness_geometry(const LoudnessPlan& plan, int64_t n);

// h[k] = sinc(k / 4) * kaiser(49, 8.0)[k + 24], k = -24 .. 24, in taps[k + 24]
void loudness_true_peak_taps(double* taps49);

struct LoudnessGated {
    double integrated, range, momentary_max, short_term_max;
};
// the gating of BS.1770-4 / Tech 3341 / Tech 3342 over e[nsub][2]; -inf (never NaN) where no block qualifies
LoudnessGated loudness_gate(const double* e, int64_t nsub, int S);

}  // namespace mgx
