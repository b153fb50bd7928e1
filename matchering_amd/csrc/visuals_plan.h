// Visuals (waveform overview, spectrogram): the limits and the index arithmetic that the device-free entry point
// (mgx_policy.cpp: mgx_spectrogram_plan), the host runners (mgx.hip), the kernels (visuals_kernel.h) and the CPU
// emulation share.  Plain C++, no HIP.  Definitions: include/mgx.h, "Visuals"; DESIGN.md section 3.18.
#pragma once

#include <cstdint>

namespace mgx {

constexpr int SPECTRO_LOG2_MIN = 8, SPECTRO_LOG2_MAX = 14;      // transforms of 256 .. 16384 points
// hops of one output column a workgroup of k_spectrogram accumulates in float32 before its partial goes out; a column
// of more hops is split over several workgroups whose partials k_spectro_pool folds in float64
constexpr int SPECTRO_RUN_CAP = 32;
// the partial spectra ([columns * parts][2][N/2+1] float32) and the picture ([columns][2][bands] float32) each stay
// under this many bytes: a request beyond it is refused, it asks for fewer columns
constexpr long long VISUALS_BYTES_MAX = 1ll << 31;
constexpr long long VISUALS_FRAMES_MAX = 500000000ll;           // as the meter's and the audit's
constexpr int OVERVIEW_THREADS = 256;
constexpr int OVERVIEW_SHARE = 16384;                           // frames of one column a workgroup of k_overview walks
constexpr int OVERVIEW_COLUMNS_MAX = 65536;

#if defined(__HIPCC__) && !defined(MGX_HOST_EMU)
#define MGX_PLAN_HD __host__ __device__ inline
#else
#define MGX_PLAN_HD inline
#endif

// hops of a track of n frames: hop t is centred on frame t * hop, the last one on the last multiple below n
MGX_PLAN_HD long long spectro_hops(long long n, int hop) { return n > 0 ? (n - 1) / hop + 1 : 0; }
// the `count` items (hops of a picture, frames of a track) of column c of `columns`: [c count / columns, (c + 1) count / columns)
MGX_PLAN_HD void visuals_column(long long count, int columns, int c, long long& first, long long& last) {
    first = (long long)c * count / columns;
    last = (long long)(c + 1) * count / columns;
}
// workgroups per column, the same for every column: the longest column has ceil(count / columns) items
MGX_PLAN_HD int visuals_parts(long long count, int columns, int share) {
    const long long longest = (count + columns - 1) / columns;
    return (int)((longest + share - 1) / share);
}
// part p of a column [first, last): `share` items from first + p share on, cut at last (empty where the column is
// shorter than the longest one by the one item that opened a new part)
MGX_PLAN_HD void visuals_part(long long first, long long last, int p, int share, long long& begin, long long& end) {
    begin = first + (long long)p * share;
    end = begin + share < last ? begin + share : last;
    if (begin > last) begin = end = last;
}

}  // namespace mgx
