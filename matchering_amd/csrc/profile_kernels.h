// Reference profiles on the device (include/mgx.h, mgx_profile_header): the reference's half of stages.py:38-104 kept as
// a block of memory instead of recomputed per target.  Device only:
//   * k_profile_pack: TrackStats + finished loud-piece spectra of a reference -> a profile (mgx_reference_profile),
//   * k_profile_curve: k_match_curve (fir_kernels.h) for a target ALONE, the reference's terms read from a profile,
//   * k_profile_raw: k_fir_raw's sibling behind k_levels + k_average_spectra, for piece tables beyond a workgroup's LDS,
//   * k_profile_merge: several profiles pooled into one over the union of their loud pieces (mgx_profile_merge).
#pragma once

#include "../../include/mgx.h"
#include "fir_kernels.h"
#include "levels_kernels.h"
#include "wave_util.h"

namespace mgx {

// the Config fields a profile must have been made with (by value: the kernels compare them with the header)
struct ProfileWant {
    int internal_sample_rate, fft_size;
    double max_piece_size, threshold, min_value;
};
// What the host reads in the handle's error word DEVICE_ERROR_SLOT_PROFILE: the first header field that does not fit.
enum { PROFILE_OK = 0, PROFILE_BAD_MAGIC, PROFILE_BAD_VERSION, PROFILE_BAD_RATE, PROFILE_BAD_FFT, PROFILE_BAD_PIECE,
       PROFILE_BAD_THRESHOLD, PROFILE_BAD_MIN_VALUE, PROFILE_BAD_COUNT };
// (every thread reads the same few header words: the block behind the header is only as long as the profile's OWN
// fft_size makes it, so nobody may touch the spectra before this has answered PROFILE_OK)
__device__ __forceinline__ int profile_check(const mgx_profile_header* p, const ProfileWant& want) {
    if (p->magic != MGX_PROFILE_MAGIC) return PROFILE_BAD_MAGIC;
    if (p->version != MGX_PROFILE_VERSION) return PROFILE_BAD_VERSION;
    if (p->internal_sample_rate != want.internal_sample_rate) return PROFILE_BAD_RATE;
    if (p->fft_size != want.fft_size) return PROFILE_BAD_FFT;
    if (p->max_piece_size != want.max_piece_size) return PROFILE_BAD_PIECE;
    if (p->threshold != want.threshold) return PROFILE_BAD_THRESHOLD;
    if (p->min_value != want.min_value) return PROFILE_BAD_MIN_VALUE;
    return PROFILE_OK;
}
__device__ __forceinline__ const double* profile_spectra(const mgx_profile_header* p) {
    return reinterpret_cast<const double*>(p + 1);              // [2][bins], mid then side
}

// grid over 2 * bins values, 256 threads; thread 0 of workgroup 0 writes the header.  `avg`: k_finish_spectra's output.
__global__ __launch_bounds__(256) void k_profile_pack(const TrackStats* st, const double* avg, ProfileWant made_with,
                                                      long long frames, int bins, mgx_profile_header* out, int* error) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    double* spectra = reinterpret_cast<double*>(out + 1);
    if (i < 2 * bins) spectra[i] = avg[i];
    if (i != 0) return;
    mgx_profile_header hd;
    hd.magic = MGX_PROFILE_MAGIC;
    hd.version = MGX_PROFILE_VERSION;
    hd.internal_sample_rate = made_with.internal_sample_rate;
    hd.fft_size = made_with.fft_size;
    hd.max_piece_size = made_with.max_piece_size;
    hd.threshold = made_with.threshold;
    hd.min_value = made_with.min_value;
    hd.frames = frames;
    hd.piece = st->piece;
    hd.divisions = st->divisions;
    hd.loud_count = st->loud_count;
    hd.peak = st->peak;
    hd.amplitude_coefficient = st->amplitude_c;
    hd.average_rms = st->average_rms;
    hd.match_rms = st->match_rms;
    *out = hd;
    // NaN or infinity among the reference's samples (k_match_curve reports the same for a pair): no profile silently
    if (error && (st->loud_count == 0 || !(fabs(st->match_rms) < 1.0e300))) error[DEVICE_ERROR_SLOT_INPUT] = 1;
}

// LDS carve of k_profile_curve, in doubles: acc[1024] | scal[8] | sums[divisions] | ss[nwg] ; then ints loud[divisions]
// and floats pk[nwg] -- the target's rows only
__host__ __device__ inline size_t profile_curve_lds_bytes(int divisions, int nwg) {
    return ((size_t)1024 + 8 + (size_t)divisions + nwg) * 8 + ((size_t)divisions + nwg + 4) * 4;
}
// k_match_curve for the target alone: the same piece decisions (one wave, wave_decide), the same fixed-order sums of the
// loud rows of wg_spec through the same buffer loads -- for the same workgroup rows the target's level, statistics and
// averaged spectrum are those of the pair route bit for bit; the rows themselves are cut by the analysis launch, whose
// chunks per piece are chosen over the tracks that share it (choose_chunks), so a target analysed alone may sum in other
// groups than beside a reference -- and the reference's half is two loads from the profile:
//     c0 = profile.match_rms / max(eps, target match),   raw[plane][k] = avg_r[k] / max(curve_floor, avg_t[k] * c0)
// (k_fir_raw's expression with the reference's term finished).  Grid (bin tiles of TILE, 2 planes) x 1024 threads;
// workgroup (0, 0) leaves the target's TrackStats, piece tables, c0, the reset correction state and the verdict on
// the profile's header.
template <int TILE>
__global__ __launch_bounds__(1024) void k_profile_curve(CurveTrack tt, const mgx_profile_header* prof, ProfileWant want,
                                                        int bins, int fft, double threshold, double eps,
                                                        double curve_floor, double* raw /* [2][bins] */, double* c0_out,
                                                        CorrectionState* cs_init, int* error) {
    MGX_LDS;
    const int rows = tt.nwg, divisions = tt.lv.divisions;
    double* acc = reinterpret_cast<double*>(mgx_smem);
    double* scal = acc + 1024;                                  // {amplitude_c, match, count, -}
    double* sums = scal + 8;                                    // [divisions]
    double* ss = sums + divisions;                              // [rows] piece-chunk sums of mid^2
    int* loud = reinterpret_cast<int*>(ss + rows);              // [divisions]
    float* pk = reinterpret_cast<float*>(loud + divisions);     // [rows]
    const bool writer = blockIdx.x == 0 && blockIdx.y == 0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // as in k_match_curve: the first sixteen rows are asked for before the decisions they will be weighed by
    constexpr int ROWL = 1024 / TILE;
    const int b = threadIdx.x % TILE, row_lane = threadIdx.x / TILE, plane = blockIdx.y;      // (row_lane == ROWL: the idle thread)
    const int bin = row_lane < ROWL ? blockIdx.x * TILE + b : bins;
    const MemView vt = mem_view(tt.wg_spec, (long long)tt.nwg * 2 * bins * 4);
    const unsigned lane_off = bin < bins ? (unsigned)((((size_t)row_lane * 2 + plane) * bins + bin) * 4) : 0xfffffff0u;
    const unsigned row_step = (unsigned)((size_t)ROWL * 2 * bins * 4);
    double ssv[2] = {0.0, 0.0};
    float pkv[2] = {0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int w = threadIdx.x + 1024 * u;
        if (w < rows) {
            ssv[u] = tt.lv.wg_sumsq[w];
            pkv[u] = tt.lv.wg_peak[w];
        }
    }
    float v0[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v0[u] = ld_f1(vt, lane_off, (unsigned)u * row_step);
    // the reference's half: the header's verdict first -- the spectra are only as long as the profile's own fft_size
    const int verdict = profile_check(prof, want);
    const double ref_match = prof->match_rms;
    const bool mine = verdict == PROFILE_OK && row_lane == 0 && bin < bins;
    const double avg_r = mine ? profile_spectra(prof)[(size_t)plane * bins + bin] : 0.0;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int w = threadIdx.x + 1024 * u;
        if (w < rows) {
            ss[w] = ssv[u];
            pk[w] = pkv[u];
        }
    }
    for (int w = threadIdx.x + 2048; w < rows; w += 1024) {       // (more rows than that: the plain way)
        ss[w] = tt.lv.wg_sumsq[w];
        pk[w] = tt.lv.wg_peak[w];
    }
    lds_barrier();
    for (int d = threadIdx.x; d < divisions; d += 1024) {
        const double* src = ss + (size_t)d * tt.lv.chunks_per_piece;
        double sum = 0.0;
        for (int ch = 0; ch < tt.lv.chunks_per_piece; ++ch) sum += src[ch];
        sums[d] = sum;
    }
    lds_barrier();
    if (wave == 0) {
        const LevelsArgs& t = tt.lv;
        float m = 0.f;
        for (int w = lane; w < rows; w += 64) m = fmaxf(m, pk[w]);
        const double peak = (double)wave_max(m);
        double c = 1.0;
        if (t.is_reference && peak < threshold) c = fmax(eps, peak / threshold);     // dsp.py:98-99
        double avg, match;
        int count;
        wave_decide(sums, divisions, t.piece, 1.0 / c, writer ? t.rms : nullptr, loud, avg, match, count);
        if (lane == 0) {
            scal[0] = c;
            scal[1] = match;
            scal[2] = (double)count;
        }
        if (writer) {
            for (int d = lane; d < divisions; d += 64) t.loud[d] = loud[d];
            if (lane == 0) {
                TrackStats st;
                st.peak = peak;
                st.amplitude_c = c;
                st.average_rms = avg;
                st.match_rms = match;
                st.divisions = divisions;
                st.loud_count = count;
                st.piece = t.piece;
                *t.st = st;
                // (k_match_curve's report of a NaN or an infinity among the samples; a profile that carries one too)
                if (error && (count == 0 || !(fabs(match) < 1.0e300) || !(fabs(ref_match) < 1.0e300)))
                    error[DEVICE_ERROR_SLOT_INPUT] = 1;
                if (error && verdict != PROFILE_OK) error[DEVICE_ERROR_SLOT_PROFILE] = verdict;
            }
        }
    }
    lds_barrier();
    const double c0 = ref_match / fmax(eps, scal[1]);            // match_levels.py:106-111
    if (writer && threadIdx.x == 0) {
        *c0_out = c0;
        if (cs_init) correction_reset(cs_init, 1.0);            // stages.py:138-170 starts from gain 1
    }
    double sacc = 0.0;
    {
        // workgroup row -> piece without a division per row (k_match_curve)
        const unsigned magic = (unsigned)((0x100000000ull + tt.lv.chunks_per_piece - 1) / tt.lv.chunks_per_piece);
#pragma unroll 1
        for (int w0 = 0; w0 < rows; w0 += ROWL * 16) {
            if (opaque(w0) > 0) {                               // (the first batch is in flight since the top)
#pragma unroll
                for (int u = 0; u < 16; ++u) v0[u] = ld_f1(vt, lane_off, (unsigned)(w0 / ROWL + u) * row_step);
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int w = w0 + row_lane + ROWL * u;
                const int piece = tt.lv.chunks_per_piece == 1 ? w : (int)__umulhi((unsigned)w, magic);
                const bool on = w < rows && loud[w < rows ? piece : 0] != 0;
                sacc += on ? (double)v0[u] : 0.0;
            }
        }
    }
    acc[threadIdx.x] = sacc;
    __syncthreads();
    if (row_lane == 0 && bin < bins) {
        double total = 0.0;
#pragma unroll 8
        for (int l = 0; l < ROWL; ++l) total += acc[l * TILE + b];
        // mean over loud pieces and segments of |rfft|/F of the target (match_frequencies.py:42)
        const double level = total / (scal[2] * (double)tt.segs_per_piece * (double)fft * scal[0]);
        // (a refused profile: its spectra are not read and the curve is flat; c0 and the scalars the later stages read are
        // still the foreign header's -- the launches behind this one are bounded whatever they hold, and the call fails)
        raw[(size_t)plane * bins + bin] = verdict == PROFILE_OK ? avg_r / fmax(curve_floor, level * c0) : 1.0;   // stages.py:90-91 on the target
    }
}

// The raw matching curves behind k_levels + k_average_spectra on the target alone: k_fir_raw with the reference's
// spectrum and match RMS read from the profile.  Grid (bins / 256, 2 planes).
__global__ __launch_bounds__(256) void k_profile_raw(FirPlanView pl, const double* part_t, const TrackStats* st_t,
                                                     int segs_t, const mgx_profile_header* prof, ProfileWant want,
                                                     double eps, double* raw /* [2][bins] */, double* c0_out,
                                                     CorrectionState* cs_init, int* error) {
    const int k = blockIdx.x * 256 + threadIdx.x, plane = blockIdx.y;
    const int verdict = profile_check(prof, want);
    const double ref_match = prof->match_rms;
    const double c0 = ref_match / fmax(eps, st_t->match_rms);                      // match_levels.py:106-111
    if (plane == 0 && k == 0) {
        *c0_out = c0;
        if (cs_init) correction_reset(cs_init, 1.0);       // stages.py:138-170 starts from gain 1
        if (error && (st_t->loud_count == 0 || !(fabs(st_t->match_rms) < 1.0e300) || !(fabs(ref_match) < 1.0e300)))
            error[DEVICE_ERROR_SLOT_INPUT] = 1;
        if (error && verdict != PROFILE_OK) error[DEVICE_ERROR_SLOT_PROFILE] = verdict;
    }
    if (k >= pl.bins) return;
    const double sc_t = spectrum_scale(st_t, segs_t, pl.fft) * c0;                 // stages.py:90-91
    const double at = spectrum_at(part_t, plane, pl.bins, k) * sc_t;
    // (a refused profile: its spectra are not read and the curve is flat, as in k_profile_curve)
    const double ar = verdict == PROFILE_OK ? profile_spectra(prof)[(size_t)plane * pl.bins + k] : 0.0;
    raw[(size_t)plane * pl.bins + k] = verdict == PROFILE_OK ? ar / fmax(pl.min_value, at) : 1.0;
}

// The sources of a merge, by value in the kernel's arguments (64 x 12 bytes): one launch, nothing copied.
struct ProfileMergeArgs {
    const mgx_profile_header* src[MGX_PROFILE_MERGE_MAX];
    int weight[MGX_PROFILE_MERGE_MAX];      // positive: "count this reference w times"
    int count;
};
// Several profiles into one: the reference's own means (match_levels.py:62-71 get_average_rms over the loud pieces'
// RMS, match_frequencies.py:30-42 the mean over pieces and segments) over the UNION of the sources' loud-piece lists,
// source i counted weight[i] times.  With n_i = weight[i] * loud_count_i and N = sum n_i:
//     spectra[k] = sum_i n_i avg_i[k] / N,   match_rms = sqrt(sum_i n_i match_i^2 / N),   peak and coefficient: the largest
// -- float64 sums in source order.  Grid over 2 * bins values, 256 threads; thread 0 of workgroup 0 writes the header.
// Every thread checks every source's header first (profile_check, and counts that are positive and fit int32 when
// summed): a source's spectra are only as long as its OWN fft_size makes them.  The first refused source leaves
// verdict | (index + 1) << 8 in the error word and an output header whose magic is 0; no spectra are read then.
__global__ __launch_bounds__(256) void k_profile_merge(ProfileMergeArgs a, ProfileWant want, int bins,
                                                       mgx_profile_header* out, int* error) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int refused = 0;
    long long loud = 0, divisions = 0;
    for (int s = 0; s < a.count; ++s) {
        const mgx_profile_header* p = a.src[s];
        int verdict = profile_check(p, want);
        if (verdict == PROFILE_OK) {
            const long long w = a.weight[s];
            if (p->loud_count <= 0 || p->divisions < p->loud_count) verdict = PROFILE_BAD_COUNT;
            loud += w * p->loud_count;
            divisions += w * p->divisions;
            if (loud > 0x7fffffffll || divisions > 0x7fffffffll) verdict = PROFILE_BAD_COUNT;
        }
        if (verdict != PROFILE_OK) {
            refused = verdict | (s + 1) << 8;
            break;
        }
    }
    if (refused) {
        if (i == 0) {
            mgx_profile_header hd = {};                         // (magic 0: never a usable profile)
            *out = hd;
            if (error) error[DEVICE_ERROR_SLOT_PROFILE] = refused;
        }
        return;
    }
    // one source counted once is that source: its bytes as they are ((n x) / n is not always x)
    const bool copy = a.count == 1 && a.weight[0] == 1;
    const double total = (double)loud;
    if (i < 2 * bins) {
        double sum = 0.0;
        for (int s = 0; s < a.count; ++s) {
            const mgx_profile_header* p = a.src[s];
            const double n = (double)((long long)a.weight[s] * p->loud_count);
            sum += n * profile_spectra(p)[i];
        }
        reinterpret_cast<double*>(out + 1)[i] = copy ? profile_spectra(a.src[0])[i] : sum / total;
    }
    if (i != 0) return;
    if (copy) {
        *out = *a.src[0];
    } else {
        mgx_profile_header hd = *a.src[0];                      // magic, version and the five Config fields
        hd.frames = 0;
        double match = 0.0, average = 0.0;
        for (int s = 0; s < a.count; ++s) {
            const mgx_profile_header* p = a.src[s];
            const long long w = a.weight[s];
            hd.frames += w * p->frames;
            if (p->piece != hd.piece) hd.piece = 0;
            hd.peak = fmax(hd.peak, p->peak);
            hd.amplitude_coefficient = fmax(hd.amplitude_coefficient, p->amplitude_coefficient);   // match_levels.py:29-44 on the largest peak
            match += (double)(w * p->loud_count) * (p->match_rms * p->match_rms);
            average += (double)(w * p->divisions) * (p->average_rms * p->average_rms);
        }
        hd.divisions = (int)divisions;
        hd.loud_count = (int)loud;
        hd.match_rms = sqrt(match / total);
        hd.average_rms = sqrt(average / (double)divisions);
        *out = hd;
    }
    if (!error) return;
    for (int s = 0; s < a.count; ++s) {                          // (k_profile_pack's report, for a source that carries one)
        const mgx_profile_header* p = a.src[s];
        if (!(fabs(p->match_rms) < 1.0e300) || !(fabs(p->amplitude_coefficient) < 1.0e300)) error[DEVICE_ERROR_SLOT_INPUT] = 1;
    }
}

}  // namespace mgx
