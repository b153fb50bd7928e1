// CPU emulation of the sample-rate converter -- TEST INFRASTRUCTURE (tests/test_resample_plan.py).
//
// Compiled by tests/emu/build.py ("resample") with a plain host compiler and -DMGX_HOST_EMU: the host plan
// (matchering_amd/csrc/resample_plan.cpp) as the library compiles it, the launch as mgx_resample fills it
// (resample_launch) and the SAME per-thread phase functions k_resample inlines (resample_kernel.h), driven by a loop
// over thread ids where the GPU has a workgroup and a plain sequence point where it has a barrier.  Not part of the
// product.
#include <cstring>
#include <vector>

#include "../../matchering_amd/csrc/resample_kernel.h"
#include "../../matchering_amd/csrc/resample_plan.h"

using namespace mgx;

// geometry[0..5] = L, M, taps, W, index_step, span; -1 when the library would refuse the rate pair
extern "C" int emu_resample_geometry(int rate_in, int rate_out, int* geometry) {
    ResampleGeometry g;
    std::string why;
    if (resample_geometry(rate_in, rate_out, &g, &why) != 0) return -1;
    const int v[6] = {g.L, g.M, g.taps, g.W, g.index_step, g.span};
    std::memcpy(geometry, v, sizeof v);
    return 0;
}

extern "C" long long emu_resample_length(long long n, int rate_in, int rate_out) {
    return resample_length(n, rate_in, rate_out);
}

// rows[L][W] and the largest row sum of |w|
extern "C" int emu_resample_rows(int rate_in, int rate_out, double* rows, double* max_row_sum) {
    const auto plan = resample_design(rate_in, rate_out);
    if (!plan) return -1;
    std::memcpy(rows, plan->rows.data(), plan->rows.size() * sizeof(double));
    *max_row_sum = plan->max_row_sum;
    return 0;
}

// launch[0..1] = the grid and the dynamic LDS bytes mgx_resample launches with for n_out outputs; -1 for a refused rate pair
extern "C" int emu_resample_launch(int rate_in, int rate_out, int channels, long long n_out, long long* launch) {
    ResampleGeometry g;
    std::string why;
    if (resample_geometry(rate_in, rate_out, &g, &why) != 0) return -1;
    ResampleArgs a;
    const ResampleLaunch l = resample_launch(a, g, 0, n_out, channels);
    launch[0] = l.grid, launch[1] = (long long)l.lds;
    return 0;
}

template <int CH>
static void run(const ResampleArgs& a, int span_max, double* sums) {
    std::vector<float> lds((size_t)span_max * CH);
    for (long long t0 = 0; t0 < a.n_out; t0 += RESAMPLE_BLOCK) {
        const ResampleTile tile = resample_tile(a, t0);
        if (tile.span > span_max) throw 1;                    // the launch's LDS would not hold the tile
        std::fill(lds.begin(), lds.end(), 1.0e30f);           // (what a previous workgroup left behind must not matter)
        for (int tid = 0; tid < RESAMPLE_BLOCK; ++tid) resample_stage<CH>(a, tile, lds.data(), tid);
        // -- barrier --
        for (int tid = 0; tid < RESAMPLE_BLOCK; ++tid) {
            const double2 acc = resample_sum<CH>(a, tile, lds.data(), tid);
            if (t0 + tid < a.n_out) {
                sums[2 * (t0 + tid)] = acc.x;
                sums[2 * (t0 + tid) + 1] = acc.y;
            }
            resample_store(a, t0 + tid, acc);
        }
    }
}

// x[n][channels] float32 -> out[n_out][2] float32 as the kernel stores it, and sums[n_out][2]: the float64
// accumulators before that rounding.  `out` must hold exactly n_out frames (stores beyond it are dropped, as on the
// device).  Returns n_out, -1 for a refused rate pair, -2 when a tile outgrows the LDS the launch would give it.
extern "C" long long emu_resample(const float* x, long long n, int channels, int rate_in, int rate_out, double* sums,
                                  float* out) {
    const auto plan = resample_design(rate_in, rate_out);
    if (!plan) return -1;
    const std::vector<double> matrix = resample_device_matrix(*plan);
    ResampleArgs a;
    const ResampleLaunch launch = resample_launch(a, plan->g, n, resample_length(n, rate_in, rate_out), channels);
    a.x = x;
    a.w = matrix.data();
    a.out = out;
    const int span_max = (int)(launch.lds / (channels * sizeof(float)));        // frames the launch's LDS holds
    try {
        if (channels == 2)
            run<2>(a, span_max, sums);
        else
            run<1>(a, span_max, sums);
    } catch (int) {
        return -2;
    }
    return a.n_out;
}
