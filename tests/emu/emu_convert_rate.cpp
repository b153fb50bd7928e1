// CPU emulation of the deliveries' sample-rate converter -- TEST INFRASTRUCTURE (tests/test_convert_rate_host.py).
//
// Compiled by tests/emu/build.py ("convert_rate") with a plain host compiler and -DMGX_HOST_EMU: the host plan
// (matchering_amd/csrc/resample_plan.cpp) as the library compiles it, the tiling rule, the launch as mgx_convert_rate
// fills it (convert_rate_launch) and the SAME per-thread phase functions k_convert_rate inlines
// (convert_rate_kernel.h), driven by a loop over thread ids where the GPU has a workgroup and a plain sequence point
// where it has a barrier.  Not part of the product.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../matchering_amd/csrc/convert_rate_kernel.h"
#include "../../matchering_amd/csrc/resample_plan.h"

using namespace mgx;

// tiling[0..2] = P, S, span for `forced` = 0 (the rule) or that P (P = 0: it does not fit); -1 for a refused rate pair
extern "C" int emu_convert_rate_tiling(int rate_in, int rate_out, int forced, int* tiling) {
    ResampleGeometry g;
    std::string why;
    if (resample_geometry(rate_in, rate_out, &g, &why) != 0) return -1;
    const ConvertRateTiling t = convert_rate_tiling(g, forced);
    tiling[0] = t.P, tiling[1] = t.S, tiling[2] = t.span;
    return 0;
}

// launch[0..2] = P, the grid and the dynamic LDS bytes mgx_convert_rate launches with for n_out outputs (`forced` as
// above; P = 0: nothing else is set); -1 for a refused rate pair
extern "C" int emu_convert_rate_launch(int rate_in, int rate_out, int forced, long long n_out, long long* launch) {
    ResampleGeometry g;
    std::string why;
    if (resample_geometry(rate_in, rate_out, &g, &why) != 0) return -1;
    ConvertRateArgs a;
    const ConvertRateLaunch l = convert_rate_launch(a, g, 0, n_out, forced);
    launch[0] = l.P, launch[1] = l.grid, launch[2] = (long long)l.lds;
    return 0;
}

template <int P>
static void run(const ConvertRateArgs& a, int span_max, long long first_tile, long long x_first, double* sums) {
    std::vector<float> lds((size_t)span_max * 2);
    const long long size = (long long)P * a.S, tiles = (a.n_out + size - 1) / size;
    for (long long index = first_tile; index < tiles; ++index) {
        const ConvertRateTile tile = convert_rate_tile(a, P, index);
        if (tile.span > span_max) throw 2;                      // the launch's LDS would not hold the tile
        if (tile.first < x_first && x_first > 0) throw 3;       // the tile reaches frames the caller did not bring
        std::fill(lds.begin(), lds.end(), 1.0e30f);             // (what a previous workgroup left behind must not matter)
        for (int tid = 0; tid < CONVERT_RATE_BLOCK; ++tid) convert_rate_stage(a, tile, lds.data(), tid);
        // -- barrier --
        for (int tid = 0; tid < CONVERT_RATE_BLOCK; ++tid)
            for (int i = tid; i < a.S; i += CONVERT_RATE_BLOCK) {
                double2 acc[P];
                const int live = convert_rate_sum<P>(a, tile, lds.data(), i, acc);
                for (int q = 0; q < live; ++q) {
                    const long long t = tile.t0 + i + (long long)q * a.S;
                    sums[2 * t] = acc[q].x;
                    sums[2 * t + 1] = acc[q].y;
                }
                convert_rate_store<P>(a, tile, i, live, acc);
            }
    }
}

// x: the frames [x_first, n) of an (n, 2) float32 track -- x_first = 0: all of it; otherwise only tiles that read
// nothing before x_first may be run.  Tiles first_tile .. last are run with `forced` as in emu_convert_rate_tiling;
// out and sums hold the outputs [first_tile P S, n_out): the float32 frames as the kernel stores them and the float64
// accumulators before that rounding.  Returns n_out, -1 for a refused rate pair, -2 when P does not fit or a tile
// outgrows the LDS the launch would give it, -3 when a tile reaches before x_first.
extern "C" long long emu_convert_rate(const float* x, long long n, long long x_first, int rate_in, int rate_out, int forced,
                                      long long first_tile, double* sums, float* out) {
    const auto plan = resample_design(rate_in, rate_out);
    if (!plan) return -1;
    ConvertRateArgs a;
    const ConvertRateLaunch launch = convert_rate_launch(a, plan->g, n, resample_length(n, rate_in, rate_out), forced);
    if (launch.P == 0) return -2;
    const std::vector<double> matrix = resample_device_matrix(*plan);
    const long long out_first = first_tile * launch.P * a.S;
    a.x = x - 2 * x_first;
    a.w = matrix.data();
    a.out = out - 2 * out_first;
    double* all = sums - 2 * out_first;
    const int span_max = (int)(launch.lds / sizeof(float2));        // frames the launch's LDS holds
    try {
        switch (launch.P) {
            case 8: run<8>(a, span_max, first_tile, x_first, all); break;
            case 4: run<4>(a, span_max, first_tile, x_first, all); break;
            case 2: run<2>(a, span_max, first_tile, x_first, all); break;
            default: run<1>(a, span_max, first_tile, x_first, all); break;
        }
    } catch (int code) {
        return -code;
    }
    return a.n_out;
}
