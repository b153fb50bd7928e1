// Host plan of the sample-rate converter (matchering/checker.py:30-45; matchering_amd/resample.py is the numpy form).
//
// rate_out / rate_in = L / M in lowest terms.  Output t sits at input time t M / L = n + p / L with
//     n = (t * M) / L,   p = (t * M) % L          (64-bit integers: exact an hour into a file and beyond)
// and resampy's weights depend on the phase p only.  `rows` holds them a row per phase, W = 2 * taps entries each:
//     y[t] = sum over k in [0, W) of rows[p][k] * x[n - (k - taps)],        frames outside the array count as zero
// -- the right wing (x[n + 1] .. x[n + taps]) in entries 0 .. taps - 1, nearest sample last, then the left wing
// (x[n] .. x[n - taps + 1]).  These are the numbers resample._prototype puts into its prototype filter: the Kaiser
// windowed sinc table of resample.kaiser_best(), scaled by the ratio when it is below 1, walked with the INTEGER
// stride int(scale * 512) and interpolated linearly between its entries, each wing as long as the table allows for
// its phase.  No GPU code here: g++ compiles this file for the CPU emulation (tests/emu/emu_resample.cpp).
#pragma once

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace mgx {

constexpr int RESAMPLE_MAX_PHASES = 4096;                       // resample.resample's max_phases: beyond it the host runs its literal loop
constexpr int RESAMPLE_BLOCK = 256;                             // outputs per workgroup of k_resample (resample_kernel.h)
constexpr int RESAMPLE_SPAN_MAX = 7680;                         // input frames a workgroup may stage: 60 KB of LDS as stereo float32
constexpr size_t RESAMPLE_MATRIX_MAX = (size_t)64 << 20;        // bytes of weights kept per handle and rate pair
constexpr int64_t RESAMPLE_FRAMES_MAX = 500000000;              // 32-bit byte offsets, as everywhere in the library

struct ResampleGeometry {
    int L = 0, M = 0;           // phases, hop
    int taps = 0, W = 0;        // longest wing, entries of a row
    int index_step = 0;         // stride through the table
    double ratio = 0.0, scale = 0.0;
    int span = 0;               // input frames RESAMPLE_BLOCK consecutive outputs reach, at most
};

// 0 and the geometry, or -1 and the reason this rate pair stays on the host (rates must be positive and different)
int resample_geometry(int rate_in, int rate_out, ResampleGeometry* g, std::string* why);

// int(n * (rate_out / rate_in)) with the same IEEE operations as resample.resample
int64_t resample_length(int64_t n, int rate_in, int rate_out);

struct ResamplePlan {
    ResampleGeometry g;
    std::vector<double> rows;   // [L][W]
    double max_row_sum = 0.0;   // largest sum of |w| over a row
};

// designs the rows (the table behind them is built once per process)
std::shared_ptr<const ResamplePlan> resample_design(int rate_in, int rate_out);

// The matrix as the kernel reads it: a row per TAP and a column per output of one period, column j holding phase
// (j * M) % L -- the order in which consecutive outputs meet the phases, so that the 64 lanes of a wave, which take
// consecutive outputs, read consecutive doubles.  [W][L].
std::vector<double> resample_device_matrix(const ResamplePlan& plan);

}  // namespace mgx
