// Stage 2's first half on the host side: the matching curve of a pair or of a target against a profile, and the FIR
// designed from it on the device (fir_kernels.h, profile_kernels.h).
#pragma once

#include "handle.h"
#include "run_analysis.h"

// device-side FIR design (fir_plan.h): spectra partial sums of both tracks -> cx.taps ([2][F] float),
// level gain c0 -> cx.scalars[0].  No host synchronisation.  The chain raw -> smooth is one dense
// operator per plan (fir_kernels.h), built on first use.
static int build_fir_operator(mgx_handle* h, const FirPlanView& pl, double** out, int2** band_out) {
    const size_t per = (size_t)3 * pl.bins + (size_t)3 * pl.nlog + pl.lw.anchors;
    const int batch = std::min(pl.bins, 256);
    DevBuf scratch_tmp, M_tmp, band_tmp;                        // (freed on every way out; M and band are handed over at the end)
    HIP_TRY(hipMalloc(&scratch_tmp.p, (size_t)batch * per * sizeof(double)));
    double* scratch = (double*)scratch_tmp.p;
    HIP_TRY(hipMalloc(&M_tmp.p, (size_t)pl.bins * pl.bins * sizeof(double)));
    double* M = (double*)M_tmp.p;
    const size_t lds_scan = (size_t)FirDesign::Scan::SCRATCH * sizeof(Affine);
    for (int col0 = 0; col0 < pl.bins; col0 += batch) {
        const int nb = std::min(batch, pl.bins - col0);
        hipLaunchKernelGGL(k_fir_unit_a, dim3(nb), dim3(1024), lds_scan, h->fq, pl, scratch, col0);
        hipLaunchKernelGGL(k_fir_lowess, dim3((pl.lw.anchors + 15) / 16, nb), dim3(1024), 0, h->fq, pl, scratch);
        hipLaunchKernelGGL(k_fir_b, dim3(nb), dim3(1024), lds_scan, h->fq, pl, scratch);
        hipLaunchKernelGGL(k_fir_gather, dim3((nb + 255) / 256, pl.bins), dim3(256), 0, h->fq, pl, scratch, col0,
                           nb, M);
    }
    HIP_TRY(hipMalloc(&band_tmp.p, (size_t)pl.bins * sizeof(int2)));
    int2* band = (int2*)band_tmp.p;
    hipLaunchKernelGGL(k_fir_band, dim3(pl.bins), dim3(256), 0, h->fq, (const double*)M, pl.bins, band);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->fq));
    *out = M;
    *band_out = band;
    M_tmp.p = band_tmp.p = nullptr;                             // the caller's from here; the scratch goes
    return 0;
}

constexpr size_t FIR_FACTOR_DENSE_BUDGET = (size_t)1 << 30;      // 1 GiB for a factor's dense intermediate

// A dense [rows][cols] matrix -> its rows' windows (k_fir_band), packed.  The dense matrix stays the caller's.
static int pack_fir_factor(mgx_handle* h, double* dense, int rows, int cols, PlanDev::Factor& f) {
    DevBuf band_tmp;
    HIP_TRY(hipMalloc(&band_tmp.p, (size_t)rows * sizeof(int2)));
    int2* band_dev = (int2*)band_tmp.p;
    hipLaunchKernelGGL(k_fir_band, dim3(rows), dim3(256), 0, h->fq, (const double*)dense, cols, band_dev);
    HIP_TRY(hipGetLastError());
    std::vector<int2> band(rows);
    HIP_TRY(hipMemcpyAsync(band.data(), band_dev, (size_t)rows * sizeof(int2), hipMemcpyDeviceToHost, h->fq));
    HIP_TRY(hipStreamSynchronize(h->fq));
    std::vector<FactorRow> desc(rows);
    long long total = 0;
    for (int r = 0; r < rows; ++r) {
        desc[r] = FactorRow{band[r].x, band[r].y, total};
        total += (band[r].y - band[r].x + 1) & ~1;               // (rows start on 16-byte boundaries)
    }
    f.bytes = (size_t)std::max<long long>(total, 2) * sizeof(double);
    HIP_TRY(hipMalloc((void**)&f.rows, (size_t)rows * sizeof(FactorRow)));
    HIP_TRY(hipMalloc((void**)&f.packed, f.bytes));
    HIP_TRY(hipMemcpyAsync(f.rows, desc.data(), (size_t)rows * sizeof(FactorRow), hipMemcpyHostToDevice, h->fq));
    HIP_TRY(hipMemsetAsync(f.packed, 0, f.bytes, h->fq));
    hipLaunchKernelGGL(k_fir_pack, dim3(rows), dim3(256), 0, h->fq, (const double*)dense, cols, (const FactorRow*)f.rows,
                       f.packed);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->fq));
    return 0;
}

// raw -> smooth as B * (A * raw) through the anchors' LOWESS fits (fir_kernels.h): unit vectors pushed through the two
// halves of the chain, 256 at a time, gathered into dense matrices that live only until their windows are packed
static int build_fir_factors(mgx_handle* h, const FirPlanView& pl, PlanDev& pd) {
    const size_t per = (size_t)3 * pl.bins + (size_t)3 * pl.nlog + pl.lw.anchors;
    const int anchors = pl.lw.anchors, batch = 256;
    DevBuf scratch_tmp, dense_tmp;
    HIP_TRY(hipMalloc(&scratch_tmp.p, (size_t)batch * per * sizeof(double)));
    double* scratch = (double*)scratch_tmp.p;
    const size_t lds_scan = (size_t)FirDesign::Scan::SCRATCH * sizeof(Affine);
    // A: unit raw curves -> the anchors' fits
    HIP_TRY(hipMalloc(&dense_tmp.p, (size_t)anchors * pl.bins * sizeof(double)));
    double* dense = (double*)dense_tmp.p;
    for (int col0 = 0; col0 < pl.bins; col0 += batch) {
        const int nb = std::min(batch, pl.bins - col0);
        hipLaunchKernelGGL(k_fir_unit_a, dim3(nb), dim3(1024), lds_scan, h->fq, pl, scratch, col0);
        hipLaunchKernelGGL(k_fir_lowess, dim3((anchors + 15) / 16, nb), dim3(1024), 0, h->fq, pl, scratch);
        hipLaunchKernelGGL(k_fir_gather_plane, dim3((nb + 255) / 256, anchors), dim3(256), 0, h->fq, pl, scratch, col0,
                           nb, pl.bins, 1, dense);
    }
    HIP_TRY(hipGetLastError());
    MGX_TRY(pack_fir_factor(h, dense, anchors, pl.bins, pd.A));
    // B: unit fits -> the smooth curve on the linear grid (the same bytes: bins x anchors)
    for (int col0 = 0; col0 < anchors; col0 += batch) {
        const int nb = std::min(batch, anchors - col0);
        hipLaunchKernelGGL(k_fir_unit_fit, dim3(nb), dim3(256), 0, h->fq, pl, scratch, col0);
        hipLaunchKernelGGL(k_fir_b, dim3(nb), dim3(1024), lds_scan, h->fq, pl, scratch);
        hipLaunchKernelGGL(k_fir_gather_plane, dim3((nb + 255) / 256, pl.bins), dim3(256), 0, h->fq, pl, scratch, col0,
                           nb, anchors, 0, dense);
    }
    HIP_TRY(hipGetLastError());
    MGX_TRY(pack_fir_factor(h, dense, pl.bins, anchors, pd.B));
    return 0;
}

static ProfileWant profile_want(const mgx_config* cfg) {
    return ProfileWant{cfg->internal_sample_rate, cfg->fft_size, cfg->max_piece_size, cfg->threshold, cfg->min_value};
}

// Bins per workgroup of the curve kernels (k_match_curve, k_profile_curve; their grid is tiles x 2): tiles of 33 bins
// where they save a round of workgroups (one workgroup of 1024 threads per CU), else 32
static int curve_tile(const mgx_handle* h, int bins) {
    auto rounds = [&](int tile) { return (2 * ((bins + tile - 1) / tile) + h->cus - 1) / h->cus; };
    return rounds(33) < rounds(32) ? 33 : 32;
}

// The raw matching curve of a target against a reference PROFILE (mgx_master_with_profile): k_profile_curve, one launch,
// while the target's piece tables fit a workgroup's LDS -- its own carve, the target's rows only -- else k_levels +
// k_average_spectra on the target and k_profile_raw.  Leaves what the pair route's curve kernels leave.
static int run_profile_curve(mgx_handle* h, const mgx_config* cfg, const FirPlanView& pl, const TrackWork& tw,
                             const mgx_profile_header* profile, double* raw) {
    CallContext& cx = context(h);
    const ProfileWant want = profile_want(cfg);
    const size_t lds_curve = profile_curve_lds_bytes(tw.divisions, tw.nwg);
    if (lds_curve <= LDS_PER_WORKGROUP_MAX) {
        CurveTrack ct{levels_args(tw), (const float*)tw.wg_spec.p, tw.nwg, tw.segs_per_piece};
        const int tile = curve_tile(h, pl.bins);
        const auto curve = tile == 33 ? k_profile_curve<33> : k_profile_curve<32>;
        MGX_TRY(allow_lds(curve, lds_curve));
        hipLaunchKernelGGL(curve, dim3((pl.bins + tile - 1) / tile, 2), dim3(1024), lds_curve, h->fq, ct, profile, want,
                           pl.bins, pl.fft, cfg->threshold, cfg->min_value, pl.min_value, raw, (double*)cx.scalars.p,
                           (CorrectionState*)cx.cstate.p, h->error_dev);
    } else {
        TrackWork& t = const_cast<TrackWork&>(tw);
        MGX_TRY(run_levels(h, cfg, &t, nullptr));
        hipLaunchKernelGGL(k_profile_raw, dim3((pl.bins + 255) / 256, 2), dim3(256), 0, h->fq, pl,
                           (const double*)tw.part.p, (const TrackStats*)tw.stats.p, tw.segs_per_piece, profile, want,
                           cfg->min_value, raw, (double*)cx.scalars.p, (CorrectionState*)cx.cstate.p, h->error_dev);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// The raw matching curve of a pair: piece decisions of both tracks, loud-piece spectra and the curve in one launch while
// the piece tables fit a workgroup's LDS (always, short of thousands of pieces), three otherwise.
static int run_pair_curve(mgx_handle* h, const mgx_config* cfg, const FirPlanView& pl, const TrackWork& tw,
                          const TrackWork& rw, double* raw) {
    CallContext& cx = context(h);
    const int max_div = std::max(tw.divisions, rw.divisions);
    const size_t lds_curve = match_curve_lds_bytes(max_div, tw.nwg + rw.nwg);
    if (lds_curve <= LDS_PER_WORKGROUP_MAX) {
        CurveTrack ct{levels_args(tw), (const float*)tw.wg_spec.p, tw.nwg, tw.segs_per_piece};
        CurveTrack cr{levels_args(rw), (const float*)rw.wg_spec.p, rw.nwg, rw.segs_per_piece};
        const int tile = curve_tile(h, pl.bins);
        const auto curve = tile == 33 ? k_match_curve<33> : k_match_curve<32>;
        MGX_TRY(allow_lds(curve, lds_curve));
        hipLaunchKernelGGL(curve, dim3((pl.bins + tile - 1) / tile, 2), dim3(1024), lds_curve, h->fq, ct, cr, pl.bins,
                           pl.fft, max_div, cfg->threshold, cfg->min_value, pl.min_value, raw, (double*)cx.scalars.p,
                           (CorrectionState*)cx.cstate.p, h->error_dev);
    } else {
        TrackWork& t = const_cast<TrackWork&>(tw);
        TrackWork& r = const_cast<TrackWork&>(rw);
        MGX_TRY(run_levels(h, cfg, &t, &r));
        FirInputs in;
        in.part_t = (const double*)tw.part.p;
        in.part_r = (const double*)rw.part.p;
        in.st_t = (const TrackStats*)tw.stats.p;
        in.st_r = (const TrackStats*)rw.stats.p;
        in.segs_t = tw.segs_per_piece;
        in.segs_r = rw.segs_per_piece;
        in.eps = cfg->min_value;
        hipLaunchKernelGGL(k_fir_raw, dim3((pl.bins + 255) / 256, 2), dim3(256), 0, h->fq, pl, in, raw,
                           (double*)cx.scalars.p, (CorrectionState*)cx.cstate.p);
    }
    return 0;
}

// The designed taps of `cx` -> their minimum-phase form, in place (eq_shape_kernels.h): four transforms of N = 4F float64
// points per channel, a sub-transform launch and a combine launch each.  fft from 64 to 16384 (mgx_eq_shape_check).
static int run_minimum_phase(mgx_handle* h, CallContext& cx, int fft) {
    MinPhaseArgs a;
    a.fft = fft;
    a.n = fft * MINPHASE_OVERSAMPLE;
    minphase_geometry(fft, a.log2m, a.r);
    {
        std::lock_guard<std::mutex> lock(g_plan_mu);
        double2*& table = g_minphase_twiddles[std::make_pair(h->device, a.n)];
        if (!table) {
            std::vector<double2> host(a.n);
            const double pi = 3.14159265358979323846;
            for (int j = 0; j < a.n; ++j) host[j] = make_double2(std::cos(2.0 * pi * j / a.n), std::sin(2.0 * pi * j / a.n));
            DevBuf tmp;
            HIP_TRY(hipMalloc(&tmp.p, host.size() * sizeof(double2)));
            HIP_TRY(hipMemcpy(tmp.p, host.data(), host.size() * sizeof(double2), hipMemcpyHostToDevice));
            table = (double2*)tmp.p;
            tmp.p = nullptr;
        }
        a.tw = table;
    }
    MGX_TRY(ensure(h, cx.eq_work, minphase_work_bytes(fft)));
    a.taps = (float*)cx.taps.p;
    a.a = (double2*)cx.eq_work.p;
    a.b = a.a + (size_t)2 * a.n;
    a.hmax = (unsigned long long*)(a.b + (size_t)2 * a.n);
    const int threads = minphase_threads(a.log2m);
    const size_t lds = minphase_lds_bytes(a.log2m);
    MGX_TRY(allow_lds(k_minphase_sub, lds));
    for (int step = 0; step < 4; ++step) {
        hipLaunchKernelGGL(k_minphase_sub, dim3(a.r, 2), dim3(threads), lds, h->fq, a, step);
        hipLaunchKernelGGL(k_minphase_combine, dim3((minphase_combine_count(a, step) + 255) / 256, 2), dim3(256), 0, h->fq, a,
                           step);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// fir_given: a FIR pair to use instead of the designed one (album mode), or null.  profile: the reference as a profile
// (then `rw` is not looked at), or null
// shape: the matching EQ's controls (include/mgx.h, mgx_eq_shape; checked by the caller), or null
// tone: its tone controls (mgx_eq_tone; checked by the caller, not neutral, and then `shape` is not null), or null
static int run_fir_design(mgx_handle* h, const mgx_config* cfg, const TrackWork& tw, const TrackWork& rw,
                          const float* fir_given, const mgx_profile_header* profile = nullptr,
                          const mgx_eq_shape* shape = nullptr, const mgx_eq_tone* tone = nullptr) {
    CallContext& cx = context(h);
    std::shared_ptr<FirPlanHost> plan = FirPlanHost::get(fir_design_params(*cfg));
    // no operator when LOWESS is not linear (robustness passes): the chain runs on the curve itself.  Otherwise the
    // dense operator up to fft_size 8192 (134 MB there, of which a product reads a sixth), its two packed factors
    // from 16384 on (h->fir_round4: the choices of round 4, dense at 16384 and the chain itself beyond)
    const bool robust = cfg->lowess_it > 0;
    // (the factors are found by pushing unit vectors through the chain into two DENSE anchors x bins matrices before they
    // are packed: with lowess_delta = 0 every point of the log grid is an anchor -- 8.6 GB at fft_size 32768 -- so the
    // factored form needs that intermediate to fit a budget; beyond it the chain runs on the curve itself, as in round 4)
    const size_t dense_bytes = (size_t)plan->anchors() * (size_t)plan->bins() * sizeof(double);
    const bool factored = !robust && plan->bins() > 4097 && !h->fir_round4 && dense_bytes <= FIR_FACTOR_DENSE_BUDGET;
    const bool direct = robust || (!factored && plan->bins() > 8193);
    PlanDev pd;
    {
        // (the first handle to need an operator builds it on its own stream and waits for it; its siblings
        // wait here and find it complete)
        std::lock_guard<std::mutex> lock(g_plan_mu);
        PlanDev& shared = g_plan_dev[std::make_pair(h->device, (const FirPlanHost*)plan.get())];
        if (!shared.blob) {
            HIP_TRY(hipMalloc(&shared.blob, plan->blob_bytes()));
            HIP_TRY(hipMemcpy(shared.blob, plan->blob(), plan->blob_bytes(), hipMemcpyHostToDevice));
            shared.plan = plan;
        }
        if (factored) {
            if (!shared.A.packed || !shared.B.packed) {
                // (a build that failed half-way leaves nothing behind: both factors or neither)
                for (PlanDev::Factor* f : {&shared.A, &shared.B}) {
                    if (f->rows) hipFree(f->rows);
                    if (f->packed) hipFree(f->packed);
                    *f = PlanDev::Factor();
                }
                MGX_TRY(build_fir_factors(h, plan->view(shared.blob), shared));
            }
        } else if (!direct && !shared.M) {
            MGX_TRY(build_fir_operator(h, plan->view(shared.blob), &shared.M, &shared.band));
        }
        pd = shared;
    }
    const FirPlanView pl = plan->view(pd.blob);
    const size_t per = (size_t)3 * pl.bins + (size_t)3 * pl.nlog + pl.lw.anchors;
    // (two scratch planes, the raw curves, and the partial transforms of the tap synthesis: [2][fft/2] double2)
    MGX_TRY(ensure(h, cx.fir_scratch, (2 * per + 2 * (size_t)pl.bins + 2 * (size_t)pl.fft + 2) * sizeof(double)));
    MGX_TRY(ensure(h, cx.scalars, 64));
    MGX_TRY(ensure(h, cx.taps, (size_t)2 * cfg->fft_size * sizeof(float)));
    double* scratch = (double*)cx.fir_scratch.p;
    double* raw = scratch + 2 * per;
    MGX_TRY(ensure(h, cx.cstate, sizeof(CorrectionState)));
    if (profile)
        MGX_TRY(run_profile_curve(h, cfg, pl, tw, profile, raw));
    else
        MGX_TRY(run_pair_curve(h, cfg, pl, tw, rw, raw));
    if (fir_given) {             // the levels above are this pair's own; the matching EQ is somebody else's
        if (fir_given != (const float*)cx.taps.p)
            HIP_TRY(hipMemcpyAsync(cx.taps.p, fir_given, (size_t)2 * cfg->fft_size * sizeof(float),
                                   hipMemcpyDeviceToDevice, h->fq));
        cx.last_taps = cfg->fft_size;
        return 0;
    }
    if (direct) {
        const size_t lds_scan = (size_t)FirDesign::Scan::SCRATCH * sizeof(Affine);
        hipLaunchKernelGGL(k_fir_direct_a, dim3(2), dim3(1024), lds_scan, h->fq, pl, scratch, (const double*)raw);
        if (robust) {
            MGX_TRY(ensure(h, cx.fir_robust, (size_t)4 * pl.nlog * sizeof(double)));
            hipLaunchKernelGGL(k_fir_lowess_robust, dim3(2), dim3(1024), 0, h->fq, pl, scratch,
                               (double*)cx.fir_robust.p, cfg->lowess_it);
        } else {
            hipLaunchKernelGGL(k_fir_lowess, dim3((pl.lw.anchors + 15) / 16, 2), dim3(1024), 0, h->fq, pl, scratch);
        }
        hipLaunchKernelGGL(k_fir_b, dim3(2), dim3(1024), lds_scan, h->fq, pl, scratch);
    } else if (factored) {
        hipLaunchKernelGGL(k_fir_apply_a, dim3(pl.lw.anchors), dim3(256), 0, h->fq, pl, (const double*)pd.A.packed,
                           (const FactorRow*)pd.A.rows, (const double*)raw, scratch);
        hipLaunchKernelGGL(k_fir_apply_b, dim3((pl.bins + 255) / 256), dim3(256), 0, h->fq, pl, (const double*)pd.B.packed,
                           (const FactorRow*)pd.B.rows, (const double*)raw, scratch);
    } else {
        hipLaunchKernelGGL(k_fir_matvec, dim3(pl.bins), dim3(256), 0, h->fq, pl, (const double*)pd.M,
                           (const int2*)pd.band, (const double*)raw, scratch);
    }
    // the matching EQ's shape stage, in place on the two smooth planes: launched only where it changes the curve.  With
    // a tone the tone stage runs in its place (eq_tone_kernels.h): one launch either way
    if (tone && shape)
        hipLaunchKernelGGL(k_eq_tone, dim3((pl.bins + 255) / 256, 2), dim3(256), 0, h->fq, pl, scratch,
                           EqToneArgs{shape->amount, shape->max_boost_db, shape->max_cut_db, cfg->min_value, *tone,
                                      (double)cfg->internal_sample_rate, cfg->fft_size});
    else if (eq_shape_curve_stage(shape))
        hipLaunchKernelGGL(k_eq_shape, dim3((pl.bins + 255) / 256, 2), dim3(256), 0, h->fq, pl, scratch,
                           EqShapeArgs{shape->amount, shape->max_boost_db, shape->max_cut_db, cfg->min_value});
    if (pl.fft < 64) {                                          // 8 .. 32 taps: the plain cosine sum, one thread per tap
        hipLaunchKernelGGL(k_fir_taps_direct, dim3(2), dim3(1024), 0, h->fq, pl, (const double*)scratch, (float*)cx.taps.p);
        HIP_TRY(hipGetLastError());
        cx.last_taps = cfg->fft_size;
        return 0;
    }
    // tap synthesis: the symmetric cosine sum up to 4096 taps (8 us in one launch -- two launches of the split
    // transform cost 10), the split transform from 8192 taps on (13 us against 47 at 16384;
    // profiles/r03_x_tap_synthesis.txt).
    if (pl.fft >= TAP_TRANSFORM_FROM) {
        // (65536 taps: sixteen sub-transforms of 2048 points -- the longest one instantiated)
        const int split = pl.fft > 32768 ? 2 * TAP_SPLIT : TAP_SPLIT;
        const int m = pl.fft / 2 / split;
        const size_t sub_at = (2 * per + 2 * (size_t)pl.bins + 1) & ~(size_t)1;      // 16-byte aligned
        double2* sub = reinterpret_cast<double2*>(scratch + sub_at);
        const size_t lds_sub = fir_taps_sub_lds_bytes(m);
        switch (m) {
#define MGX_TAPS_SUB(L)                                                                                                \
    case 1 << L:                                                                                                       \
        hipLaunchKernelGGL(k_fir_taps_sub<L>, dim3(split, 2), dim3(TapFft<L>::T), lds_sub, h->fq, pl,              \
                           (const double*)scratch, sub);                                                               \
        break;
            MGX_TAPS_SUB(9) MGX_TAPS_SUB(10) MGX_TAPS_SUB(11)
#undef MGX_TAPS_SUB
            default: return fail(MGX_ERR_UNSUPPORTED, "tap synthesis: transform length not instantiated");
        }
        hipLaunchKernelGGL(k_fir_taps_combine, dim3((pl.fft / 2 + 255) / 256, 2), dim3(256), 0, h->fq, pl,
                           (const double2*)sub, split, (float*)cx.taps.p);
    } else {
        const size_t lds_taps = ((size_t)pl.bins + 2048 + 2 * TAP_ROWS) * sizeof(double);
        MGX_TRY(allow_lds(k_fir_taps, lds_taps));
        hipLaunchKernelGGL(k_fir_taps, dim3((pl.fft / 4 + 1 + TAP_ROWS - 1) / TAP_ROWS, 2), dim3(1024), lds_taps, h->fq,
                           pl, (const double*)scratch, (float*)cx.taps.p);
    }
    HIP_TRY(hipGetLastError());
    if (eq_shape_minimum_phase(shape)) MGX_TRY(run_minimum_phase(h, cx, cfg->fft_size));
    cx.last_taps = cfg->fft_size;
    return 0;
}
