// Stage 1 on the host side: the analysis launch of one track or a pair, and the piece decisions and spectrum sums
// behind it (analysis2_kernel.h, levels_kernels.h).
#pragma once

#include "handle.h"

// ---------------------------------------------------------------------------
// stage runners, here and in the run_*.h beside (asynchronous: the front-half runners on h->fq, the others on h->stream)
// ---------------------------------------------------------------------------

// workgroups of k_analyze<log2f> one CU holds (LDS and wave slots)
static int analysis_workgroups_per_cu(int log2f) {
    size_t lds = 0;
    int threads = 64;
    if (log2f < 6) return 8;                                     // k_analyze_small: 256 threads, a few hundred bytes of LDS
    switch (log2f) {
#define CASE(L) case L: lds = analysis_lds_bytes<L>(); threads = Fft2<L>::T; break;
        CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14)
#undef CASE
        case 15:                                                                     // two 16384-point transforms per segment
        case 16: lds = analysis_lds_bytes<14>(); threads = Fft2<14>::T; break;       // four
        default: return 1;
    }
    return std::min(ANALYZE_MAX_WGS, workgroups_per_cu(threads, lds));
}

// `kernel` runs transforms of 2^LOG2N points: k_analyze<LOG2N>, or k_analyze_double / k_analyze_quad on 16384 points
template <int LOG2N>
static int launch_analysis(mgx_handle* h, void (*kernel)(AnalysisArgs, AnalysisArgs, int), const AnalysisArgs& a0,
                           const AnalysisArgs& a1, int nwg0, int nwg) {
    const size_t lds = analysis_lds_bytes<LOG2N>();
    MGX_TRY(allow_lds(kernel, lds));
    hipLaunchKernelGGL(kernel, dim3(nwg), dim3(Fft2<LOG2N>::T), lds, h->fq, a0, a1, nwg0);
    HIP_TRY(hipGetLastError());
    return 0;
}

// geometry of a track's analysis (match_levels.py:47-59) and the workspace it fills; chunks per piece
// are chosen by the caller (they depend on what shares the launch)
static int plan_analysis(mgx_handle* h, long long n, const mgx_config* cfg, int is_reference, TrackWork& w) {
    const int f = cfg->fft_size;
    if (n <= f) return fail(MGX_ERR_ARGUMENT, "track must be longer than fft_size frames (core.py:69-74)");
    MGX_TRY(check_length(n));
    piece_geometry(n, cfg->max_piece_size, w.divisions, w.piece);
    w.segs_per_piece = (int)(w.piece / f);
    if (w.segs_per_piece < 1)
        return fail(MGX_ERR_UNSUPPORTED, "analysis pieces shorter than fft_size are not implemented");
    w.is_reference = is_reference;
    return 0;
}

// Every workgroup runs its segments back to back and a CU's residents share its throughput, so the
// kernel lasts about as long as the busiest CU has segments: ceil(workgroups / CUs) * segments per
// workgroup.  Pick the segments per workgroup that minimise it over ALL tracks of the launch (ties:
// more workgroups); a second dispatch wave of a few stragglers would double the kernel's duration.
static int choose_chunks(mgx_handle* h, const mgx_config* cfg, TrackWork* const* tracks, int count) {
    const int per_cu = analysis_workgroups_per_cu(ilog2_exact(cfg->fft_size));
    int longest = 1;
    for (int t = 0; t < count; ++t) longest = std::max(longest, tracks[t]->segs_per_piece);
    long long best_cost = -1;
    int best_s = longest;
    for (int s = 1; s <= longest; ++s) {
        long long wgs = 0;
        for (int t = 0; t < count; ++t)
            wgs += (long long)tracks[t]->divisions * ((tracks[t]->segs_per_piece + s - 1) / s);
        const long long deep = (wgs + h->cus - 1) / h->cus;
        if (deep > per_cu) continue;
        const long long cost = deep * s;
        if (best_cost < 0 || cost < best_cost) {
            best_cost = cost;
            best_s = s;
        }
    }
    for (int t = 0; t < count; ++t) {
        TrackWork& w = *tracks[t];
        w.chunks = (w.segs_per_piece + best_s - 1) / best_s;
        w.nwg = w.divisions * w.chunks;
        const int half = cfg->fft_size / 2;
        MGX_TRY(ensure(h, w.wg_sumsq, (size_t)w.nwg * sizeof(double)));
        MGX_TRY(ensure(h, w.wg_peak, (size_t)w.nwg * sizeof(float)));
        MGX_TRY(ensure(h, w.wg_spec, (size_t)w.nwg * 2 * (half + 1) * sizeof(float)));
        if (cfg->fft_size == 65536)
            MGX_TRY(ensure(h, w.wg_pack, (size_t)w.nwg * AnalysisQuad<14>::SCRATCH_FLOAT2 * sizeof(float2)));
        MGX_TRY(ensure(h, w.stats, sizeof(TrackStats)));
        MGX_TRY(ensure(h, w.rms, (size_t)w.divisions * sizeof(double)));
        MGX_TRY(ensure(h, w.loud, (size_t)w.divisions * sizeof(int)));
        MGX_TRY(ensure(h, w.avg, (size_t)2 * (half + 1) * sizeof(double)));
    }
    return 0;
}

static int analysis_args(mgx_handle* h, const float* x, long long n, const mgx_config* cfg, const TrackWork& w,
                         AnalysisArgs& a) {
    a.x = reinterpret_cast<const float2*>(x);
    a.n = n;
    a.fft = cfg->fft_size;
    a.piece = w.piece;
    a.divisions = w.divisions;
    a.segs_per_piece = w.segs_per_piece;
    a.chunks_per_piece = w.chunks;
    a.wg_sumsq = (double*)w.wg_sumsq.p;
    a.wg_peak = (float*)w.wg_peak.p;
    a.wg_spec = (float*)w.wg_spec.p;
    a.wg_pack = (float2*)w.wg_pack.p;
    a.tw = nullptr;
    if (cfg->fft_size < 64) return 0;                            // k_analyze_small transforms in registers: no table
    // (fft_size 32768 and 65536 run on 16384-point transforms: AnalysisDouble, AnalysisQuad)
    return get_twiddles(h, std::min(14, ilog2_exact(cfg->fft_size)), &a.tw);
}

// one launch for one track (second == nullptr) or for the target and the reference of a pair
static int run_analysis(mgx_handle* h, const mgx_config* cfg, const float* x0, long long n0, TrackWork& w0,
                        const float* x1 = nullptr, long long n1 = 0, TrackWork* w1 = nullptr) {
    MGX_TRY(plan_analysis(h, n0, cfg, w0.is_reference, w0));
    if (w1) MGX_TRY(plan_analysis(h, n1, cfg, w1->is_reference, *w1));
    TrackWork* tracks[2] = {&w0, w1};
    MGX_TRY(choose_chunks(h, cfg, tracks, w1 ? 2 : 1));
    AnalysisArgs a0, a1;
    MGX_TRY(analysis_args(h, x0, n0, cfg, w0, a0));
    a1 = a0;
    if (w1) MGX_TRY(analysis_args(h, x1, n1, cfg, *w1, a1));
    const int nwg = w0.nwg + (w1 ? w1->nwg : 0);
    switch (ilog2_exact(cfg->fft_size)) {
#define SMALL(L) case L: hipLaunchKernelGGL(k_analyze_small<L>, dim3(nwg), dim3(256), 0, h->fq, a0, a1, w0.nwg); HIP_TRY(hipGetLastError()); break;
        SMALL(3) SMALL(4) SMALL(5)
#undef SMALL
#define CASE(L) case L: MGX_TRY(launch_analysis<L>(h, k_analyze<L>, a0, a1, w0.nwg, nwg)); break;
        CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14)
#undef CASE
        case 15: MGX_TRY(launch_analysis<14>(h, k_analyze_double<14>, a0, a1, w0.nwg, nwg)); break;
        case 16: MGX_TRY(launch_analysis<14>(h, k_analyze_quad<14>, a0, a1, w0.nwg, nwg)); break;
        default: return fail(MGX_ERR_UNSUPPORTED, "fft_size not supported by the analysis kernel");
    }
    return 0;
}

static LevelsArgs levels_args(const TrackWork& w) {
    LevelsArgs a;
    a.wg_sumsq = (const double*)w.wg_sumsq.p;
    a.wg_peak = (const float*)w.wg_peak.p;
    a.chunks_per_piece = w.chunks;
    a.divisions = w.divisions;
    a.piece = w.piece;
    a.is_reference = w.is_reference;
    a.st = (TrackStats*)w.stats.p;
    a.rms = (double*)w.rms.p;
    a.loud = (int*)w.loud.p;
    return a;
}
static SpectraArgs spectra_args(const TrackWork& w) {
    SpectraArgs a;
    a.wg_spec = (const float*)w.wg_spec.p;
    a.loud = (const int*)w.loud.p;
    a.chunks_per_piece = w.chunks;
    a.nwg = w.nwg;
    a.part = (double*)w.part.p;
    return a;
}
// piece statistics -> decisions, then the loud pieces' spectrum sums; one launch each for 1 or 2 tracks
static int run_levels(mgx_handle* h, const mgx_config* cfg, TrackWork* first, TrackWork* second) {
    const int tracks = second ? 2 : 1, half = cfg->fft_size / 2;
    const int max_div = std::max(first->divisions, second ? second->divisions : 0);
    const size_t lds = (size_t)(64 + max_div) * sizeof(double);
    if (lds > LDS_PER_WORKGROUP_MAX) return fail(MGX_ERR_UNSUPPORTED, "too many analysis pieces");
    MGX_TRY(allow_lds(k_levels, lds));
    for (TrackWork* w : {first, second})
        if (w) MGX_TRY(ensure(h, w->part, (size_t)SPEC_SLICES * 2 * (half + 1) * sizeof(double)));
    const LevelsArgs l0 = levels_args(*first), l1 = second ? levels_args(*second) : l0;
    hipLaunchKernelGGL(k_levels, dim3(tracks), dim3(1024), lds, h->fq, l0, l1, cfg->threshold, cfg->min_value);
    const SpectraArgs s0 = spectra_args(*first), s1 = second ? spectra_args(*second) : s0;
    hipLaunchKernelGGL(k_average_spectra, dim3((half + 1 + 63) / 64, 2, SPEC_SLICES * tracks), dim3(1024), 0, h->fq,
                       s0, s1, half + 1);
    HIP_TRY(hipGetLastError());
    return 0;
}

// One track analysed by itself and its spectra finished into w.avg: what mgx_analyze hands out and
// mgx_reference_profile packs.  (A master call never runs this: its curve kernels work from the partial sums.)
static int run_track_spectra(mgx_handle* h, const mgx_config* cfg, const float* x, long long n, TrackWork& w) {
    MGX_TRY(run_analysis(h, cfg, x, n, w));
    MGX_TRY(run_levels(h, cfg, &w, nullptr));
    const int total = 2 * (cfg->fft_size / 2 + 1);
    hipLaunchKernelGGL(k_finish_spectra, dim3((total + 255) / 256), dim3(256), 0, h->stream, (const double*)w.part.p,
                       (const TrackStats*)w.stats.p, w.segs_per_piece, cfg->fft_size, (double*)w.avg.p);
    HIP_TRY(hipGetLastError());
    return 0;
}
