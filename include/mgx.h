/* mgx -- C ABI of the MI355X-native mastering core.
 *
 * sergree/matchering is pure Python: it has no FFI of its own.  The functions
 * below are the boundary a maintainer would bind (ctypes stub in INTEGRATION.md)
 * to replace the body of matchering/stages.py:210-272 (`main`) and, one level
 * down, the stage helpers it calls.  Each entry point cites the reference
 * interface it replaces.  Plain pointers and sizes only; no framework types.
 *
 * Conventions
 *  - audio is float32, interleaved stereo frames (n,2) -- numpy C order, the
 *    layout soundfile hands to matchering/loader.py:35.
 *  - "dev" pointers are device (HBM) addresses obtained from mgx_malloc; "host"
 *    pointers are ordinary memory.  Nothing is freed or retained across calls
 *    except through the handle.
 *  - every function returns 0 on success, a negative mgx_status otherwise;
 *    mgx_last_error() gives the message (thread-local).
 *  - a handle is bound to one GPU and one HIP stream ("the handle's stream" below);
 *    calls on one handle are serialised by the caller, different handles are
 *    independent.  Work takes effect in the order of the calls.  Behind that order
 *    the analysis and FIR design of an mgx_master call may run on a second stream
 *    of the handle's, under the previous call's convolution and limiter, where it
 *    reads nothing a call before it writes; mgx_synchronize and every other call
 *    that waits for the stream wait for that work too.  Only a handle that is
 *    its device's only live handle does this.
 */
#ifndef MGX_H
#define MGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mgx_handle mgx_handle;

enum mgx_status {
    MGX_OK = 0,
    MGX_ERR_ARGUMENT = -1,     /* bad size / null pointer / unsupported parameter */
    MGX_ERR_HIP = -2,          /* HIP runtime error (message has the hipError name) */
    MGX_ERR_NO_DEVICE = -3,    /* no usable GPU: there is NO CPU fallback */
    MGX_ERR_UNSUPPORTED = -4,  /* valid for the reference but not implemented here */
    MGX_ERR_RCCL = -5,
    MGX_ERR_RETRY = -6         /* a bounded device-side wait expired (the GPU is shared with somebody else's kernels); the
                                  outputs of the calls since the last synchronisation are not valid, the handle has
                                  switched to the mode that cannot wait for ever, and the same call succeeds when made
                                  again.  Blocking calls retry by themselves where nothing of the failed run has
                                  reached the host; this code is for the asynchronous ones. */
};

/* matchering/defaults.py:25-58 LimiterConfig + :61-155 Config, the fields the
 * hot path consumes.  max_piece_size is in SAMPLES (defaults.py:109 already
 * multiplied it by the sample rate). */
typedef struct mgx_config {
    int32_t internal_sample_rate;
    int32_t fft_size;
    int32_t lin_log_oversampling;
    int32_t rms_correction_steps;
    double max_piece_size;
    double threshold;
    double min_value;
    double lowess_frac;
    int32_t lowess_it;
    int32_t reserved0;
    double lowess_delta;
    /* limiter */
    double attack_ms, hold_ms, release_ms;
    double attack_filter_coefficient;
    int32_t hold_filter_order;
    int32_t release_filter_order;
    double hold_filter_coefficient;
    double release_filter_coefficient;
} mgx_config;

/* Scalars that flow between the stages of stages.py:210-272 (what the reference
 * logs through debug()).  Filled by mgx_master / the stage calls. */
typedef struct mgx_report {
    double final_amplitude_coefficient;  /* match_levels.py:29-44 */
    double target_match_rms, reference_match_rms;
    double rms_coefficient;              /* stages.py:80-88 */
    double correction_coefficients[16];  /* stages.py:149-168, first rms_correction_steps entries */
    double normalize_coefficient;        /* stages.py:186-191 (0 when not requested) */
    double result_peak;                  /* max |result_no_limiter| */
    int32_t target_divisions, reference_divisions;
    int64_t target_piece, reference_piece;
    int32_t target_loud_count, reference_loud_count;
    int32_t limiter_active;              /* 0 = hyrax.py:83-85 early-out */
    int32_t reserved;
} mgx_report;

/* ---- library / device ---------------------------------------------------- */
int mgx_version(void);
const char* mgx_last_error(void);
int mgx_device_count(int* count);
/* PCI address of GPU `device` as the driver prints it ("0000:0d:00.0", NUL-terminated, capacity >= 16): which physical
 * GPU a rank really sits on -- the batch front end and bench.py put it beside every rank's numbers (core.py:32-121 has
 * no notion of devices; this is part of the new surface, like the handle). */
int mgx_device_pci_bus_id(int device, char* out, int32_t capacity);
int mgx_create(int device, mgx_handle** out);
int mgx_destroy(mgx_handle* h);
int mgx_config_default(mgx_config* cfg);         /* Config() defaults, defaults.py:61-84 */

/* device memory + transfers (the Python host has no other way to hold HBM) */
int mgx_malloc(mgx_handle* h, size_t bytes, void** dev);
int mgx_free(mgx_handle* h, void* dev);
int mgx_memcpy_h2d(mgx_handle* h, void* dev, const void* host, size_t bytes);
int mgx_memcpy_d2h(mgx_handle* h, void* host, const void* dev, size_t bytes);
int mgx_synchronize(mgx_handle* h);
/* Page-locked host memory and copies that return at once (ordered on the handle's stream; the host
 * buffer must stay valid and untouched until mgx_synchronize): what a host needs to overlap the
 * upload of pair k+1 and the download of pair k-1 with the kernels of pair k (loader.py:30-47 and
 * saver.py:27-33 sit on either side of stages.main; PCIe is the bound of the whole process()). */
int mgx_host_alloc(size_t bytes, void** host);
int mgx_host_free(void* host);
int mgx_memcpy_h2d_async(mgx_handle* h, void* dev, const void* host, size_t bytes);
int mgx_memcpy_d2h_async(mgx_handle* h, void* host, const void* dev, size_t bytes);
/* HIP-event timing on the handle's stream: bracket any sequence of calls */
int mgx_timer_start(mgx_handle* h);
int mgx_timer_stop(mgx_handle* h, float* milliseconds);

/* ---- the drop-in boundary: stages.main ------------------------------------ */
/* Replaces matchering/stages.py:210-272 `main(target, reference, config,
 * need_default, need_no_limiter, need_no_limiter_normalized)`.  target_dev /
 * reference_dev: (n,2) float32 in HBM.  Each non-null output receives (n_target,2)
 * float32 in HBM; a null output = the corresponding need_* flag False.  Inputs
 * are not modified.  Everything, the FIR design included, is queued on the
 * handle's stream without a host round trip: with report == NULL the call returns
 * before the GPU has finished (mgx_synchronize to wait); with a report it waits
 * itself and fills it.
 * Limits (MGX_ERR_UNSUPPORTED, never a silent approximation): fft_size in
 * [8, 65536]; lowess_it in [0, 64]; tracks up to 536 million frames (32-bit byte
 * offsets; 3.3 hours at 44.1 kHz); limiter hold / release filters (defaults.py:48-56
 * accepts any positive order, hyrax.py:61-73 runs it) of order 1 to 3 whose
 * transfer-function form is well conditioned: a filter of order n at fc Hz is refused
 * when the rounding noise of the reference's own float64 recursion, about
 * 1.1e-16 / (2 pi fc / fs)^(n - 1/2) of full scale, exceeds 1e-6 -- there is then no
 * well-defined output to be within 1e-5 of (at the default cut-offs: hold order 3
 * runs, release order 3 does not; tests/test_limiter_order3_conditioning.py). */
int mgx_master(mgx_handle* h, const float* target_dev, int64_t n_target,
               const float* reference_dev, int64_t n_reference, const mgx_config* cfg,
               float* result_dev, float* result_no_limiter_dev,
               float* result_no_limiter_normalized_dev, mgx_report* report);

/* ---- stage-level entry points (parity tests, custom pipelines) ------------- */
/* match_levels.py:134-161 analyze_levels (+ dsp.py:93-100 peak for the reference,
 * match_levels.py:29-44) and match_frequencies.py:30-42 __average_fft of the loud
 * pieces, in one pass.  Host outputs (any may be null): piece_rms[divisions],
 * loud[divisions] (0/1), avg_mid/avg_side[fft_size/2+1] = mean |rfft|/F over the
 * loud pieces of the (peak-normalised, if is_reference) track. */
int mgx_analyze(mgx_handle* h, const float* x_dev, int64_t n, const mgx_config* cfg,
                int is_reference, double* peak, double* amplitude_coefficient,
                double* match_rms, int32_t* divisions, int64_t* piece_size,
                double* piece_rms, int32_t* loud, double* avg_mid, double* avg_side);

/* match_frequencies.py:78-101 get_fir from averaged spectra (host, float64).
 * avg_target must already include the level gain of stages.py:90-91.  A host-side
 * cross-check of the design (a direct float64 evaluation, no precomputed operator)
 * for tests and tools: it needs no GPU and is NOT what mgx_master runs -- there the
 * same design happens on the device (k_fir_raw / k_fir_matvec / k_fir_taps). */
int mgx_design_fir(const mgx_config* cfg, const double* avg_target, const double* avg_reference,
                   double* taps, double* curve_raw, double* curve_smooth);

/* Matching EQ controls: how much of the matching curve is applied, how far it may boost and cut, and the phase of the FIR
 * (get_fir, match_frequencies.py:78-101, has none of this: one linear-phase FIR from the whole curve).  Part of the new
 * surface.  With s[k], k = 0 .. F/2, a channel's smoothed curve (match_frequencies.py:45-75, bins 0 and 1 pinned):
 *   1. shape, float64, for k >= 1:
 *          d = amount * 20 log10(max(s[k], min_value));   d = min(d, max_boost_db);   d = max(d, -max_cut_db)
 *          s'[k] = 10^(d / 20);    s'[0] = 0
 *      A NaN cap is no cap.  With amount == 1 and no cap the stage is skipped, not multiplied by one.  Level matching is
 *      untouched: rms_coefficient and the correction rounds still bring the result to the reference's RMS.
 *   2. linear-phase taps lin[0 .. F): the existing synthesis (irfft, ifftshift, Hann) on s', float32 in the handle.
 *   3. phase == 1, minimum phase, with N = 4F, float64:
 *          H[m] = |DFT_N(lin, zero padded)[m]|;   L[m] = ln(max(H[m], 1e-9 max H));   c = Re IDFT_N(L)
 *          fold: c[0] and c[N/2] stay, c[1 .. N/2) doubles, c(N/2 .. N) = 0;   g = Re IDFT_N(exp(DFT_N(c)))
 *          taper[j] = 1 for j < F/4,  (1 + cos(pi (j - F/4) / (F/4))) / 2 for F/4 <= j < F/2
 *          taps[F/2 + j] = g[j] taper[j] for j < F/2,   taps[k] = 0 for k < F/2;   one rounding to float32 at the store
 *      The response starts where the linear-phase FIR peaks: the result stays time-aligned with a linear-phase master
 *      of the same pair, and nothing precedes the main tap.
 * mgx_eq_shape_check: needs no GPU.  MGX_ERR_ARGUMENT, the message naming the field: a null argument, amount outside
 * [0, 2] or not finite, a cap that is negative or infinite, phase outside {0, 1}, reserved != 0.  MGX_ERR_UNSUPPORTED,
 * the size named: phase == 1 with fft_size below 64 or above 16384 (the chain runs N = 4F points per channel through
 * one call's scratch; 32768 and 65536 are not instantiated).
 * mgx_shape_fir: steps 1 to 3 on the host in float64 from a smoothed curve (mgx_design_fir's curve_smooth), taps[F]
 * float64 without the rounding to float32 of steps 2 and 3.  Like mgx_design_fir a cross-check for tests and tools: it
 * needs no GPU, takes any power of two from 8 (phase == 1: from 64), and is NOT what the master runs -- there the same
 * steps happen on the device (csrc/eq_shape_kernels.h).
 * mgx_master_shaped: mgx_master (reference_dev given, profile_dev NULL) or mgx_master_with_profile (the reverse) with the
 * FIR designed under `shape`; exactly one of the two is non-null.  shape == NULL is exactly those calls.  The shape is
 * copied when the call is queued: pipelined calls with different shapes each get their own.  Refusals come before
 * anything is queued.  mgx_last_fir returns the shaped taps.  mgx_master_with_fir is unaffected: a given FIR is used as
 * given. */
typedef struct mgx_eq_shape {
    double amount;                       /* [0, 2]; 1 = the whole curve */
    double max_boost_db;                 /* >= 0, or NaN: no cap */
    double max_cut_db;                   /* >= 0, or NaN: no cap */
    int32_t phase;                       /* 0 linear, 1 minimum */
    int32_t reserved;                    /* 0 */
} mgx_eq_shape;
int mgx_eq_shape_check(const mgx_config* cfg, const mgx_eq_shape* shape);
int mgx_shape_fir(const mgx_config* cfg, const mgx_eq_shape* shape, const double* curve_smooth, double* taps);
int mgx_master_shaped(mgx_handle* h, const float* target_dev, int64_t n_target, const float* reference_dev,
                      int64_t n_reference, const void* profile_dev, const mgx_config* cfg, const mgx_eq_shape* shape,
                      float* result_dev, float* result_no_limiter_dev, float* result_no_limiter_normalized_dev,
                      mgx_report* report);

/* Matching EQ tone controls: which part of the spectrum is matched, a side amount of its own, mono bass, and manual trims
 * (a tilt, up to eight bells and shelves) on top of the match.  Part of the new surface.  They replace step 1 above; steps
 * 2 and 3 then run on s' unchanged.  With fs = internal_sample_rate, F = fft_size, f_k = (k * fs) / F (the product first:
 * exact in double), channel c = 0 mid, 1 side, and
 *     ramp(x)        = 0 for x <= 0,  1 for x >= 1,  0.5 - 0.5 cos(pi x) between
 *     edge(f, f0, w) = ramp(log2(f / f0) / w + 0.5) for w > 0;   for w == 0: 1 if f >= f0, else 0
 * per bin k >= 1, float64:
 *     w  = (low_hz NaN ? 1 : edge(f_k, low_hz, range_octaves)) * (high_hz NaN ? 1 : 1 - edge(f_k, high_hz, range_octaves))
 *     a  = c == side and side_amount not NaN ? side_amount : shape.amount
 *     d  = (a * w) * 20 log10(max(s[k], min_value));   d = min(d, max_boost_db);   d = max(d, -max_cut_db)   (NaN cap: none)
 *     t  = tilt_db_per_octave * log2(f_k / tilt_pivot_hz)
 *        + sum over the bands whose `channels` name c of
 *              bell (0):        gain_db / (1 + (q * (f_k / hz - hz / f_k))^2)
 *              low shelf (1):   gain_db / (1 + (f_k / hz)^(4 q))
 *              high shelf (2):  gain_db / (1 + (hz / f_k)^(4 q))
 *     g  = c == side and mono_below_hz not NaN ? edge(f_k, mono_below_hz, mono_octaves) : 1
 *     s'[k] = 10^((d + t) / 20) * g;     s'[0] = 0
 * The caps bound the matching part only: the trims are what the caller asked for and are bounded by the field ranges.
 * Level matching is untouched.  A NEUTRAL tone -- low_hz, high_hz, side_amount and mono_below_hz NaN, tilt 0, no bands --
 * is the call without a tone, not a multiplication by one.  A NULL shape with a tone is amount 1, no caps, linear phase.
 * mgx_eq_tone_default: the neutral tone (range_octaves 1, mono_octaves 1, tilt_pivot_hz 1000).
 * mgx_eq_tone_check: needs no GPU; shape may be NULL.  MGX_ERR_ARGUMENT, the message naming the field: a null cfg or tone;
 * low_hz outside (0, fs/2), high_hz outside (0, fs/2], low_hz >= high_hz (NaN: open on that side); range_octaves or
 * mono_octaves outside [0, 4]; side_amount outside [0, 2] (NaN: the shape's amount); mono_below_hz outside (0, fs/2) (NaN:
 * off); tilt_db_per_octave outside [-6, 6]; tilt_pivot_hz not positive and finite; band_count outside [0, 8]; of a band
 * below band_count, kind outside {0, 1, 2}, channels outside {1, 2, 3}, hz outside (0, fs/2], gain_db outside [-24, 24],
 * q outside [0.1, 20] (named bands[i].field); reserved != 0.  Then every refusal of mgx_eq_shape_check(cfg, shape).
 * mgx_eq_tone_curve: the three per-bin terms of `channel` (0 or 1) on the host, each [F/2 + 1] doubles or NULL: a * w,
 * t and g; entry 0 of each is 0.  What a front end plots.
 * mgx_tone_fir: mgx_shape_fir with the tone, for `channel`: float64, host only, a cross-check and NOT what the master
 * runs.  A NULL or neutral tone is mgx_shape_fir (a NULL shape: the default one).
 * mgx_master_eq: mgx_master_shaped with a tone (csrc/eq_tone_kernels.h: k_eq_tone runs INSTEAD of k_eq_shape, at the same
 * point of the design).  A NULL or neutral tone is exactly mgx_master_shaped.  The tone is copied when the call is queued,
 * as the shape is.  Refusals come before anything is queued.  mgx_last_fir returns the toned taps.  mgx_master_with_fir
 * is unaffected. */
#define MGX_EQ_BANDS_MAX 8
typedef struct mgx_eq_band {
    int32_t kind;                        /* 0 bell, 1 low shelf, 2 high shelf */
    int32_t channels;                    /* 1 mid, 2 side, 3 both */
    double hz;                           /* (0, fs/2] */
    double gain_db;                      /* [-24, 24] */
    double q;                            /* [0.1, 20] */
} mgx_eq_band;
typedef struct mgx_eq_tone {
    double low_hz, high_hz;              /* the matching range; NaN: open on that side */
    double range_octaves;                /* [0, 4]: width of each raised-cosine edge, centred on the edge frequency */
    double side_amount;                  /* [0, 2], or NaN: the shape's amount */
    double mono_below_hz;                /* (0, fs/2), or NaN: off */
    double mono_octaves;                 /* [0, 4] */
    double tilt_db_per_octave;           /* [-6, 6] */
    double tilt_pivot_hz;                /* > 0 */
    int32_t band_count;                  /* [0, MGX_EQ_BANDS_MAX] */
    int32_t reserved;                    /* 0 */
    mgx_eq_band bands[MGX_EQ_BANDS_MAX];
} mgx_eq_tone;
int mgx_eq_tone_default(mgx_eq_tone* tone);
int mgx_eq_tone_check(const mgx_config* cfg, const mgx_eq_shape* shape, const mgx_eq_tone* tone);
int mgx_eq_tone_curve(const mgx_config* cfg, const mgx_eq_shape* shape, const mgx_eq_tone* tone, int32_t channel,
                      double* weight_times_amount, double* trim_db, double* gate);
int mgx_tone_fir(const mgx_config* cfg, const mgx_eq_shape* shape, const mgx_eq_tone* tone, int32_t channel,
                 const double* curve_smooth, double* taps);
int mgx_master_eq(mgx_handle* h, const float* target_dev, int64_t n_target, const float* reference_dev,
                  int64_t n_reference, const void* profile_dev, const mgx_config* cfg, const mgx_eq_shape* shape,
                  const mgx_eq_tone* tone, float* result_dev, float* result_no_limiter_dev,
                  float* result_no_limiter_normalized_dev, mgx_report* report);

/* match_frequencies.py:104-119 convolve (fftconvolve "same" on mid and side,
 * then ms_to_lr): y = L/R result (n,2), y_mid (n) optional.  taps are host
 * float64 arrays of fft_size entries; `gain` scales both (stages.py:80-88 folded in). */
int mgx_convolve(mgx_handle* h, const float* x_dev, int64_t n, const double* fir_mid,
                 const double* fir_side, int32_t taps, double gain, float* y_dev, float* y_mid_dev,
                 double* peak);

/* One round of stages.py:149-160: piece RMS of clip(gain*mid, -1, 1) over the
 * target's piece grid.  Host output sumsq[divisions] = sum of squares per piece. */
int mgx_clipped_piece_sumsq(mgx_handle* h, const float* mid_dev, int64_t n, int64_t piece_size,
                            int32_t divisions, double gain, double* sumsq);

/* limiter/hyrax.py:78-99 limit(array*gain) * post_gain, float32 in/out in HBM.
 * active (host, may be null) receives 0 when the limiter early-outs. */
int mgx_limit(mgx_handle* h, const float* x_dev, int64_t n, const mgx_config* cfg, double gain,
              double post_gain, float* out_dev, int32_t* active);

/* dsp.py:89-90 amplify on interleaved frames: out = x * gain */
int mgx_scale(mgx_handle* h, const float* x_dev, int64_t n, double gain, float* out_dev);

/* Integer PCM at the boundary.  The reference reads and writes files through soundfile
 * (loader.py:35 sf.read, saver.py:27-33 sf.write), i.e. libsndfile converts between the file's integer
 * samples and floats on the host.  These two entry points do that conversion in HBM, so that the integer
 * samples -- half the bytes of float32 at 16 bits -- are what crosses PCIe: `samples` counts single
 * samples (2 per stereo frame), interleaved as in the file; bits = 16 (int16), 24 (three bytes per
 * sample, little-endian, packed) or 32 (int32).  Scaling as libsndfile: decode x = v / 2^(bits-1);
 * encode v = rint(x * (2^(bits-1) - 1)), clipped to the integer range, evaluated in float64.  Queued on
 * the handle's stream. */
/* dsp.py:49-54 count_max_peaks on interleaved float32 samples in HBM: the largest magnitude and the number
 * of samples numpy.isclose (rtol 1e-5, atol 1e-8) puts on it, either sign -- what checker.py:118-130 looks
 * at to warn about clipped or already limited targets.  Waits for the result. */
int mgx_peak_count(mgx_handle* h, const float* x_dev, int64_t samples, double* peak, int64_t* count);
int mgx_pcm_decode(mgx_handle* h, const void* pcm_dev, int64_t samples, int32_t bits, float* out_dev);
int mgx_pcm_encode(mgx_handle* h, const float* x_dev, int64_t samples, int32_t bits, void* pcm_dev);

/* Sample-rate conversion in HBM: matchering/checker.py:30-45 (`resampy.resample(array, sample_rate,
 * required_sample_rate, axis=0)`, filter kaiser_best) for a track that mgx_pcm_decode has just left on the device, so
 * that a file at another rate than Config.internal_sample_rate never becomes a float64 array on the host.  x_dev:
 * (n, channels) float32, one or two channels; out_dev: (n_out, 2) float32 -- a mono track comes out as two equal
 * columns (dsp.py:45-46) -- with n_out = int(n * (rate_out / rate_in)), known before the launch: with out_dev == NULL
 * the call only reports it (and needs no handle), so that the caller can allocate.  The sum is resampy's, phase by
 * phase with exact integer phase arithmetic, samples and weights in float64, rounded once to float32 at the store.
 * Queued on the handle's stream.  The weights of a rate pair are designed and uploaded on the handle's first
 * conversion between those rates and kept.  MGX_ERR_ARGUMENT: channels other than 1 or 2, a rate <= 0, rate_in ==
 * rate_out, out_capacity_frames < n_out.  MGX_ERR_UNSUPPORTED (the host converts such a file, as it did before): a
 * ratio of more than 4096 phases (44100 -> 44101), an output rate so far below the input rate that 256 outputs reach
 * more than 7680 input frames, more than 64 MiB of weights.  n_out == 0 succeeds and launches nothing.
 * mgx_resample_plan: the device address and shape ([row_entries][phases] float64) of the weights kept for a rate
 * pair, and how many plans this handle has designed and uploaded so far: a second conversion between the same rates
 * changes neither. */
int mgx_resample(mgx_handle* h, const float* x_dev, int64_t n, int32_t channels, int32_t rate_in, int32_t rate_out,
                 float* out_dev, int64_t out_capacity_frames, int64_t* n_out);
int mgx_resample_plan(mgx_handle* h, int32_t rate_in, int32_t rate_out, void** weights_dev, int32_t* phases,
                      int32_t* row_entries, int64_t* designed);

/* Sample-rate conversion of a delivery: (n, 2) float32 frames in HBM at rate_in -> (n_out, 2) float32 frames in HBM at
 * rate_out, n_out = int(n * (rate_out / rate_in)); queued on the handle's stream, waits for nothing.  Each output is the
 * sum mgx_resample computes for the same frames -- the same plan rows, float64 samples and weights, explicit fma in tap
 * order, one rounding to float32 at the store -- so the result is bit-identical to mgx_resample(..., channels = 2, ...)
 * on the same input; the kernel (csrc/convert_rate_kernel.h) loads each weight once for up to 8 outputs a whole number
 * of periods apart.  The weights are those of mgx_resample, shared: whichever entry point meets a rate pair first on a
 * handle designs and uploads them, mgx_resample_plan reports both.  The contract is mgx_resample's: with out_dev ==
 * NULL the call only reports n_out and the refusal (and needs no handle).  MGX_ERR_ARGUMENT: a rate <= 0, rate_in ==
 * rate_out, out_capacity_frames < n_out.  MGX_ERR_UNSUPPORTED: what mgx_resample refuses for its ratio -- more than
 * 4096 phases (44100 -> 44056), 256 outputs reaching more than 7680 input frames, more than 64 MiB of weights -- and
 * more than 500 million frames on either side; a delivery has no host path to fall back to.  n_out == 0 succeeds and
 * launches nothing. */
int mgx_convert_rate(mgx_handle* h, const float* x_dev, int64_t n, int32_t rate_in, int32_t rate_out, float* out_dev,
                     int64_t out_capacity_frames, int64_t* n_out);

/* Album mode (the use of the FIR broadcast): stages.main with the matching-EQ FIR
 * GIVEN instead of designed from this pair's spectra -- `fir_dev` = [2][fft_size] float32 in HBM, mid
 * taps then side taps, e.g. the table mgx_last_fir returns on the rank that designed it, after
 * mgx_comm_broadcast_f32 brought it here.  Levels are still matched per track (stages.py:80-91,
 * 138-170 unchanged); only match_frequencies.py:78-101 is replaced. */
int mgx_master_with_fir(mgx_handle* h, const float* target_dev, int64_t n_target, const float* reference_dev,
                        int64_t n_reference, const mgx_config* cfg, const float* fir_dev, float* result_dev,
                        float* result_no_limiter_dev, float* result_no_limiter_normalized_dev,
                        mgx_report* report);

/* Reference profiles: everything stages.main takes from the reference track (stages.py:38-104: match_levels.py:29-44
 * final_amplitude_coefficient, match_levels.py:134-161 reference_match_rms, match_frequencies.py:30-42 the loud pieces'
 * average spectra of mid and side), analysed once and kept, so that any number of targets are mastered against it
 * without its audio.  A profile is a plain block of device memory that the CALLER owns, mgx_profile_bytes(cfg) long:
 *
 *     mgx_profile_header                          (96 bytes, below)
 *     double avg_mid [fft_size / 2 + 1]           mean |rfft| / fft_size over the loud pieces of the peak-normalised
 *     double avg_side[fft_size / 2 + 1]           reference: what mgx_analyze(is_reference = 1) returns
 *
 * Nothing in it is a pointer or a handle and every field is little-endian as the GPU wrote it: mgx_memcpy_d2h keeps
 * it, mgx_memcpy_h2d brings it back, on any handle and any GPU.  The library's own handling of a profile never waits for
 * the device: mgx_reference_profile only queues, and mgx_master_with_profile waits exactly where mgx_master does (for a
 * report).
 * The header repeats the Config fields the analysis depends on.  A profile that does not fit the `cfg` it is used
 * with -- another magic or version, or one of those five fields different -- is never used silently: the device finds
 * out (the host could only by waiting), leaves the outputs of that call invalid, and the next blocking call on the
 * handle fails with MGX_ERR_ARGUMENT and a message that names the field.  The handle is good for the next call. */
#define MGX_PROFILE_MAGIC 0x5250474du    /* "MGPR" */
#define MGX_PROFILE_VERSION 1u
typedef struct mgx_profile_header {
    uint32_t magic, version;
    int32_t internal_sample_rate;        /* Config: defaults.py:61-84 */
    int32_t fft_size;
    double max_piece_size;               /* in samples, as in mgx_config */
    double threshold;
    double min_value;
    int64_t frames;                      /* the reference: its length, */
    int64_t piece;                       /* match_levels.py:47-59 piece size and count, */
    int32_t divisions;
    int32_t loud_count;                  /* match_levels.py:93-103: pieces at or above the average RMS */
    double peak;                         /* dsp.py:97 */
    double amplitude_coefficient;        /* match_levels.py:29-44 final_amplitude_coefficient */
    double average_rms;                  /* match_levels.py:62-71, of the normalised reference */
    double match_rms;                    /* match_levels.py:93-103 reference_match_rms */
} mgx_profile_header;
/* Size of a profile for `cfg` (header + 2 * (fft_size / 2 + 1) doubles).  Needs no GPU. */
int mgx_profile_bytes(const mgx_config* cfg, size_t* bytes);
/* The reference half of stages.py:38-104 (match_levels.py:134-161 analyze_levels with normalisation,
 * match_frequencies.py:30-42 __average_fft): the analysis mgx_analyze(is_reference = 1) runs, its results packed into
 * profile_dev.  Queued on the handle's stream.  A reference with NaN or infinite samples makes the next blocking call
 * fail, as it does for mgx_master (match_frequencies.py:42). */
int mgx_reference_profile(mgx_handle* h, const float* reference_dev, int64_t n_reference, const mgx_config* cfg,
                          void* profile_dev);
/* stages.py:210-272 `main` with the reference given as a profile: mgx_master, or mgx_master_with_fir when fir_dev is
 * not NULL, with stage 1 run on the target alone.  A report's reference_* fields and final_amplitude_coefficient are
 * the profile's.  Returns before the GPU has finished when report == NULL, as mgx_master does. */
int mgx_master_with_profile(mgx_handle* h, const float* target_dev, int64_t n_target, const void* profile_dev,
                            const mgx_config* cfg, const float* fir_dev, float* result_dev,
                            float* result_no_limiter_dev, float* result_no_limiter_normalized_dev,
                            mgx_report* report);
/* Reference sets: several profiles pooled into one, "master this to the sound of these five records".  Every source
 * stays what mgx_reference_profile made of its own track (normalised, cut and selected on its own); the merged profile
 * is the reference's own means over the UNION of the sources' loud pieces, the piece as the unit: match_levels.py:62-71
 * (get_average_rms over the loud pieces' RMS) and match_frequencies.py:30-42 (the mean over pieces and segments).  With
 * w_i = weights[i] ("count this reference w times"), n_i = w_i * loud_count_i and N = sum n_i, float64 sums in source
 * order:
 *     spectra[k]            = sum_i n_i * spectra_i[k] / N
 *     match_rms             = sqrt(sum_i n_i * match_rms_i^2 / N)
 *     amplitude_coefficient = max_i amplitude_coefficient_i      (match_levels.py:29-44 on the largest peak)
 *     peak                  = max_i peak_i
 *     loud_count = N,  divisions = sum_i w_i * divisions_i,  frames = sum_i w_i * frames_i
 *     average_rms           = sqrt(sum_i w_i divisions_i average_rms_i^2 / divisions)     (informational)
 *     piece                 = the sources' common value, or 0 when they differ
 * The result is an ordinary version-1 profile of mgx_profile_bytes(cfg) bytes: mgx_master_with_profile takes it, and so
 * does a later merge.  One source with weight 1 comes out byte for byte.  profiles_dev: a HOST array of `count` device
 * pointers; weights: a host array, or NULL for all 1.  Only queued on the handle's stream: the call waits for nothing.
 * MGX_ERR_ARGUMENT at once: a null argument, count outside [1, MGX_PROFILE_MERGE_MAX], a weight outside [1, 65536],
 * profile_dev overlapping a source.  A source that does not fit `cfg` (as for mgx_master_with_profile), whose
 * loud_count is not positive or exceeds its divisions, or counts whose weighted sums leave int32: the device finds
 * out, writes an output whose magic is 0, and the next blocking call fails with MGX_ERR_ARGUMENT naming the field and
 * the source. */
#define MGX_PROFILE_MERGE_MAX 64
int mgx_profile_merge(mgx_handle* h, const void* const* profiles_dev, const int32_t* weights, int32_t count,
                      const mgx_config* cfg, void* profile_dev);

/* Loudness metering on frames in HBM: ITU-R BS.1770-4 integrated loudness and true peak, EBU Tech 3341 momentary and
 * short-term maxima, EBU Tech 3342 loudness range -- what a delivery specification states ("-14 LUFS, -1 dBTP") and
 * neither mgx_report's RMS coefficients nor mgx_peak_count's sample peak can say (the reference has no meter at all; its
 * limiter's ceiling, hyrax.py:78-99, is a sample-peak ceiling).  Part of the new surface, like the handle.
 *   K-weighting: two float64 biquads per channel (high shelf, high-pass) from the closed form that gives BS.1770-4's
 *     tables at 48 kHz, at any rate from 8000 Hz; transposed direct form II, zero state at frame 0.
 *   sub-blocks: S = (sample_rate + 5) / 10 frames; sub_energy[s][c] = sum of the K-weighted squares of channel c over
 *     sub-block s, s < n / S (the n % S frames behind the last sub-block count for the peaks only).
 *   momentary / short-term blocks: 4 / 30 sub-blocks stepping one; l = -0.691 + 10 log10(mean square, both channels
 *     weighted 1).  integrated: the momentary blocks above -70 LUFS and above (their loudness - 10).  range: short-term
 *     blocks stepping ten, above -70 and above (their loudness - 20), 95th minus 10th percentile
 *     (index int((m - 1) q + 0.5) of the sorted values).  Where no block qualifies (silence, fewer than 4 sub-blocks) the
 *     loudness fields are -infinity, never NaN, and the range is 0.
 *   true_peak: largest magnitude of the 4x oversampled track, oversampled by h[k] = sinc(k / 4) * kaiser(49, 8.0)[k + 24]
 *     in float64, frames outside the track zero; sample_peak: the largest sample magnitude.  Both linear (1.0 = 0 dBFS).
 * mgx_loudness: one launch that reads the frames once, waits for the result.  sub_energy (host, [capacity][2], may be
 * NULL) receives the n / S sub-block energies and *count (may be NULL) their number.  n == 0 and n < S succeed.
 * MGX_ERR_ARGUMENT: a null handle, report or (n > 0) x_dev, sample_rate < 8000, capacity < n / S, and a track with a NaN
 * or an infinite sample (the handle is good for the next call).
 * mgx_loudness_gate: the host half on its own -- the four loudness fields (and sub_blocks, sub_block_frames) from
 * `count` sub-block energies; the peaks are left as they are.  Needs no GPU. */
typedef struct mgx_loudness_report {
    double integrated;                   /* LUFS */
    double range;                        /* LU */
    double momentary_max, short_term_max;/* LUFS */
    double true_peak, sample_peak;       /* linear */
    int64_t sub_blocks;
    int32_t sub_block_frames;
    int32_t reserved;
} mgx_loudness_report;
int mgx_loudness(mgx_handle* h, const float* x_dev, int64_t n, int32_t sample_rate, mgx_loudness_report* report,
                 double* sub_energy, int64_t capacity, int64_t* count);
int mgx_loudness_gate(const double* sub_energy, int64_t count, int32_t sample_rate, mgx_loudness_report* report);

/* Delivery renditions: a rendering written AT a delivery specification -- a loudness target, a true-peak ceiling,
 * dithered integer PCM -- from frames that are still in HBM (the reference has none of this; saver.py:27-33 rounds
 * without dither).  Part of the new surface, like the meter it builds on.
 * mgx_delivery_gain is the policy, on the host, from a measurement of mgx_loudness; needs no GPU.  Linear gain only --
 * what EBU R 128 normalisation is -- never an approximation of a limiter:
 *     g_loud = 10^((target_lufs - integrated) / 20)      1 without a target, or where integrated is -infinity
 *     g_peak = (10^(ceiling_dbtp / 20) - A e / 2^(bits-1)) / true_peak      +infinity without a ceiling or at true_peak 0
 *     gain   = min(g_loud, g_peak)
 * A e / 2^(bits-1) is the quantiser's head-room: A = the largest per-phase sum of the meter's absolute oversampling taps
 * (phase 2: 1.76294455...), computed from the taps themselves; e = the most that dither and rounding add to a sample in
 * LSB: 0.5 without dither, 1.5 with either, 0 for float output.  With it the ceiling holds for the written file as the
 * meter reads it back (decoded by v / 2^(bits-1)): DESIGN.md section 3.11 has the derivation.
 * limited_by: 2 where the ceiling set the gain (g_peak < g_loud), else 1 where a loudness target did, else 0 (nothing was
 * asked for, or nothing that was asked for changes the gain).  shortfall_lu = target_lufs - achieved_lufs where the ceiling
 * kept the loudness below the target, else 0.
 * MGX_ERR_ARGUMENT, the message naming the field: a null argument; ceiling_dbtp above 0 (clipping would break the bound) or
 * so low that the head-room leaves g_peak nothing; an infinite target_lufs or ceiling_dbtp; bits outside {0, 16, 24, 32};
 * dither outside {0, 1, 2}, or dither with bits 0 or 32; a measured true_peak that is negative or not finite, a measured
 * integrated that is NaN or +infinity. */
typedef struct mgx_delivery {
    double target_lufs;                  /* NaN: no loudness target */
    double ceiling_dbtp;                 /* NaN: no ceiling; otherwise <= 0 */
    int32_t bits;                        /* 0 = float32 out, or 16, 24, 32 */
    int32_t dither;                      /* 0 none, 1 TPDF, 2 high-passed TPDF */
    uint64_t seed;
} mgx_delivery;
typedef struct mgx_delivery_result {
    double gain;                         /* linear */
    double achieved_lufs;                /* integrated + 20 log10(gain); -infinity where integrated is */
    double achieved_true_peak;           /* gain * true_peak, linear: as predicted from the measurement */
    double shortfall_lu;                 /* >= 0 */
    int32_t limited_by;                  /* 0 nothing, 1 loudness, 2 true peak */
    int32_t reserved;
} mgx_delivery_result;
int mgx_delivery_gain(const mgx_delivery* delivery, const mgx_loudness_report* measured, mgx_delivery_result* result);
/* One pass over interleaved float32 samples in HBM: gain, dither, quantise, pack.  `samples` counts single samples, as
 * mgx_pcm_encode does; out_dev receives `samples` float32 (bits 0), int16, packed 24-bit or int32 values.  With
 * top = 2^(bits-1) - 1:
 *     a = ((double)x[s] * gain) * top;     v = clip(rint(a + d(s)), -top - 1, top)        bits 0: out[s] = (float)(x[s] * gain)
 * d = 0 without dither: at gain 1.0 the output is mgx_pcm_encode's, byte for byte.  The random numbers are Philox4x32-10
 * (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85), key = (seed low word, seed high word),
 * counter = (q low, q high, stream, 0) with q = s >> 2; W(s, stream) = output word s & 3;
 * U(s, stream) = ((W >> 8) + 0.5) 2^-24 - 0.5, 0 for s < 0.  TPDF: d(s) = U(s, 0) + U(s, 1).  High-passed TPDF:
 * d(s) = U(s, 0) - U(s - 2, 0), the same channel one frame earlier: triangular density, first-differenced spectrum, no
 * error feedback.  Every value is defined bit for bit (tests/delivery_oracle.py).  Queued on the handle's stream; waits
 * for nothing.  x_dev and out_dev must be 16-byte aligned (what mgx_malloc returns is).  MGX_ERR_ARGUMENT: a null
 * argument, negative samples, a misaligned pointer, a gain that is not finite, bits or dither as for mgx_delivery_gain. */
int mgx_deliver(mgx_handle* h, const float* x_dev, int64_t samples, double gain, int32_t bits, int32_t dither,
                uint64_t seed, void* out_dev);

/* A true-peak look-ahead limiter for deliveries whose ceiling binds: where mgx_delivery_gain answers limited_by == 2 the
 * linear policy leaves the file `shortfall_lu` under its target, and this is what makes up for it.  It is not the mastering
 * limiter (mgx_limit: the reference's sample-peak limiter, part of the parity surface) and shares nothing with it: three
 * launches per call, none of whose workgroups waits for another.  For x[n][2], pre-gain g > 0, linear ceiling c > 0,
 * look-ahead L >= 1 frames and release R >= 0 frames, rho = exp(-1 / R) and rho = 0 at R = 0:
 *   1. envelope   e[m] = g max over p = 0 .. 3 and both channels of |sum_j h[p + 4 j] x[m - j]|, h the meter's taps
 *                 (mgx_loudness), frames outside the track zero: max_m e[m] / g is the meter's true peak of x.
 *   2. reduction  d0[m] = 1 - c / e[m] where e[m] > c, else 0 (a NaN compares false: 0).
 *   3. hold       d[m] = max of d0[m + j], |j| <= L, 0 <= m + j < n.
 *   4. release    q[m] = max(d[m], rho q[m - 1]), q[-1] = 0.
 *   5. smoothing  s[m] = sum_{|k| <= L} w[k] q[clamp(m + k, 0, n - 1)], w[k] = (L + 1 - |k|) / (L + 1)^2: two box-cars of
 *                 L + 1 frames, weights >= 0 that sum to 1.  The edge frames are repeated, not padded with zeros.
 *   6. output     out[m][ch] = (float)(((double)x[m][ch] g) (1 - s[m])), one gain for both channels; *max_reduction =
 *                 max_m s[m].
 * Guarantee: (1 - s[m]) e[m] <= c for every frame -- every q in the window of m is at least d there, and every d within L
 * of m is at least d0[m].  Not guaranteed: that a meter reads `out` under c, because its interpolator sees 12 neighbouring
 * frames with a gain each (the excess is about 1e-5 at L = 66, 2e-2 at L = 1).  A delivery therefore
 * meters what the limiter made and trims it with mgx_delivery_gain, whose bound is the one that holds for the file.
 * Float64 throughout, except that d0 crosses launches as float32 (rounded to nearest: 2^-25 on the gain); two calls give
 * the same bytes.  Queued on the handle's stream; waits only when max_reduction (host, may be NULL) is asked for.  n == 0
 * succeeds and launches nothing.  MGX_ERR_ARGUMENT, the message naming the field: a null handle, x_dev or out_dev; n < 0;
 * out_dev overlapping x_dev; a pointer that is not 8-byte aligned; pre_gain or ceiling not finite or <= 0; lookahead
 * outside [1, 2048]; release negative, not finite or above 2^22.  The handle is good for the next call. */
int mgx_tp_limit(mgx_handle* h, const float* x_dev, int64_t n, double pre_gain, double ceiling, int32_t lookahead,
                 double release, float* out_dev, double* max_reduction);
/* The policy of a limited delivery, on the host; needs no GPU.  Called with the passes run so far -- their pre-gains in dB
 * and the integrated loudness mgx_loudness read from each pass's output, passes == 0 before the first -- it says whether to
 * run another pass, at which pre-gain, and the limiter's ceiling.  Every pass limits the ORIGINAL rendering.
 *     ceiling   = 10^(ceiling_dbtp / 20) - A e / 2^(bits-1): the numerator of mgx_delivery_gain's g_peak
 *     passes 0:   run only where mgx_delivery_gain(delivery, rendering) answers limited_by == 2;
 *                 p_1 = target_lufs - rendering->integrated, 0 without a target or where that loudness is -infinity
 *     passes k:   stop where there is no target, target - I_k <= tolerance_lu, k == max_passes, I_k is -infinity, or
 *                 k >= 2 and (I_k - I_{k-1}) / (p_k - p_{k-1}) < 0.1 (a steady tone cannot be made louder under a ceiling);
 *                 else p_{k+1} = p_k + (target - I_k) / slope, slope 1 after the first pass, then that quotient, at most 1
 * When it answers run == 0 after k >= 1 passes the delivery is mgx_delivery_gain on the measurement of the last pass's
 * output and mgx_deliver of that output: gain, head-room, shortfall_lu and the ceiling's proof are theirs.
 * MGX_ERR_ARGUMENT: a null argument, a delivery without a ceiling or that mgx_delivery_gain refuses, max_passes outside
 * [1, 16], passes outside [0, max_passes], tolerance_lu negative or not finite, NaN or +infinity among the passes. */
#define MGX_LIMIT_PASSES_MAX 16
typedef struct mgx_delivery_limit_plan {
    double pre_gain_db;                  /* the next pass's pre-gain; with run == 0 the last pass's (0 before the first) */
    double ceiling;                      /* linear */
    int32_t run;                         /* 1: run a pass at pre_gain_db; 0: finish */
    int32_t reserved;
} mgx_delivery_limit_plan;
int mgx_delivery_limit_step(const mgx_delivery* delivery, const mgx_loudness_report* rendering, int32_t passes,
                            const double* pre_gain_db, const double* integrated, int32_t max_passes, double tolerance_lu,
                            mgx_delivery_limit_plan* next);

/* Noise-shaped dither for CD-width deliveries: the quantiser's error is fed back through a short filter, so that the
 * noise leaves the 2-5 kHz region, where the ear is most sensitive, for the top of the band.  Error feedback is a
 * non-linear recurrence that no scan removes; it is defined here on SEGMENTS, so that a track is many short chains
 * (DESIGN.md section 3.15).  With frames x[n][2], a gain, bits in {16, 24}, top = 2^(bits-1) - 1, a seed and a shaper
 * c[1..K], 0 <= K <= MGX_SHAPER_TAPS_MAX (mgx_noise_shaper.c[k - 1] holds c[k]), per sample s = 2 m + ch:
 *     a[s] = ((double)x[s] * gain) * top;     d[s] = U(s, 0) + U(s, 1)        exactly mgx_deliver's TPDF values
 * Segment j covers the frames [j B, min(n, (j + 1) B)), B = MGX_SHAPER_SEGMENT; each channel of each segment is one chain.
 * A chain starts at frame max(0, j B - W), W = MGX_SHAPER_WARMUP, with e_1 .. e_K = 0, and at every frame computes
 *     t = 0.0;  for k = 1..K:  t = t + c[k] * e_k        (one product and one sum per tap, each rounded, in this order)
 *     w = a - t;   r = rint(w + d);   e_new = r - w;   (e_K, .., e_1) <- (e_{K-1}, .., e_1, e_new)
 *     for frames >= j B:  out = clip(r, -top - 1, top)   (the error is taken BEFORE the clip: |e| stays about 3/2)
 * The warm-up frames j B - W .. j B - 1 are computed and not written.  The noise transfer function is
 * H(z) = 1 - sum_k c[k] z^-k; with K = 0 the bytes are mgx_deliver's at dither 1.  Every value is defined bit for bit
 * (tests/deliver_shaped_oracle.py).
 * mgx_noise_shaper_preset hands out the library's table of published coefficients, designed for 44.1 kHz; host only:
 *     id 1  Lipshitz, Vanderkooy, Wannamaker 1991, 5 taps:  2.033, -2.165, 1.959, -1.590, 0.6149
 *     id 2  Wannamaker 1992, F-weighted, 9 taps:  2.412, -3.370, 3.937, -4.174, 3.353, -2.205, 1.281, -0.569, 0.0847
 * for file rates from 44100 to 48000 Hz; MGX_ERR_UNSUPPORTED for every other rate, MGX_ERR_ARGUMENT for another id or a
 * null `out`.  Custom coefficients are taken at any rate.
 * Head-room.  Where nothing clips the file differs from a by e[n] - sum_k c[k] e[n-k] with |e| <= 3/2, plus float64
 * rounding, so the shaped quantiser's e of mgx_delivery_gain's head-room A e / 2^(bits-1) is
 *     e_shaped = (3/2) (1 + sum_k |c[k]|) (1 + 2^-20)
 * -- the last factor covers every rounding of the recurrence whenever the policy accepts the ceiling at all (DESIGN.md
 * section 3.15 has the derivation) -- and nothing clips under a ceiling <= 0 dBTP, since A > 1.
 * mgx_delivery_gain_shaped is mgx_delivery_gain and mgx_delivery_limit_step_shaped is mgx_delivery_limit_step (its
 * arguments plus the shaper), both with that head-room; delivery->dither must be 1 and delivery->bits 16 or 24.
 * MGX_ERR_ARGUMENT, the message naming the field: what the plain functions refuse, a null shaper, taps outside
 * [0, MGX_SHAPER_TAPS_MAX], a coefficient c[k] that is not finite.
 * mgx_deliver_shaped: n_frames frames of x_dev -> 2 n_frames int16 or packed 24-bit samples in out_dev, in one launch
 * (csrc/deliver_shaped_kernel.h); queued on the handle's stream, waits for nothing; n_frames == 0 succeeds and launches
 * nothing.  MGX_ERR_ARGUMENT, the message naming the field: a null h, x_dev, shaper or out_dev; n_frames negative; x_dev
 * or out_dev not 16-byte aligned; bits outside {16, 24}; taps outside [0, 16]; a coefficient or a gain that is not
 * finite.  MGX_ERR_UNSUPPORTED: more than 536 million frames.  The handle is good for the next call. */
#define MGX_SHAPER_TAPS_MAX 16
#define MGX_SHAPER_SEGMENT 1024
#define MGX_SHAPER_WARMUP 64
typedef struct mgx_noise_shaper {
    int32_t taps;                        /* K */
    int32_t reserved;
    double c[16];                        /* c[k - 1] = c[k] of the definition; entries from `taps` on are ignored */
} mgx_noise_shaper;
int mgx_noise_shaper_preset(int32_t id, int32_t sample_rate, mgx_noise_shaper* out);
int mgx_delivery_gain_shaped(const mgx_delivery* delivery, const mgx_noise_shaper* shaper, const mgx_loudness_report* measured,
                             mgx_delivery_result* result);
int mgx_delivery_limit_step_shaped(const mgx_delivery* delivery, const mgx_noise_shaper* shaper,
                                   const mgx_loudness_report* rendering, int32_t passes, const double* pre_gain_db,
                                   const double* integrated, int32_t max_passes, double tolerance_lu,
                                   mgx_delivery_limit_plan* next);
int mgx_deliver_shaped(mgx_handle* h, const float* x_dev, int64_t n_frames, double gain, int32_t bits,
                       const mgx_noise_shaper* shaper, uint64_t seed, void* out_dev);

/* Audit: the quality-control pass a distributor's intake check makes, over frames or file PCM that are still in HBM -- DC
 * offset, runs of samples at the rail, a stereo image that cancels in mono, dropouts, head and tail silence, samples that
 * are not finite numbers (the reference's checker counts the samples on the peak and nothing else; mgx_loudness gives
 * loudness and peaks).  Part of the new surface, like the meter.  DESIGN.md section 3.17.
 *   input: n stereo frames, interleaved.  bits 0: float32; bits 16, 24, 32: file PCM as mgx_pcm_decode reads it
 *     (little-endian, 24-bit packed in three bytes).  An integer sample v has the value v / 2^(bits-1) as a double, so
 *     32-bit samples are exact; all arithmetic on values is float64, every product rounded once and every sum on its own
 *     (no fused multiply-add).
 *   limits: clip_level (linear, > 0), clip_run (>= 1), silence_level (linear, >= 0; 0: exact zeros only).
 *   per sample: non-finite = NaN or +-Inf (bits 0 only); at the rail = finite and |x| >= clip_level; a frame is silent
 *     when both samples are finite and |x| <= silence_level.  A non-finite sample is counted in nonfinite[c], left out of
 *     every sum and of peak, is not at the rail and makes its frame not silent.
 *   per channel c: sum[c], sumsq[c]; peak[c] = max |x| over the finite samples; nonfinite[c].  A run is a maximal
 *     sequence of consecutive at-rail samples of one channel, of either sign; an event is a run of length >= clip_run.
 *     clip_events[c] = events, clip_samples[c] = samples inside events, clip_longest[c] = the longest run of any length
 *     (0: none), clip_first[c] = the frame of the first event's first sample (-1: none).
 *   stereo: sum_lr = sum of L R over the frames whose samples are both finite.
 *   silence: head_silence = silent frames before the first frame that is not (n when every frame is silent),
 *     tail_silence the same from the end; gap_longest / gap_at = the longest run of silent frames strictly between the
 *     first and the last non-silent frame and where it starts (0 and -1: none; of equal runs the earliest).
 *   sub-blocks: B = (sample_rate + 5) / 10 frames -- the meter's grid, rounded as mgx_loudness rounds it (sample_rate / 10
 *     wherever the rate is a multiple of 10).  sub_sums[k] = {sum L^2, sum R^2, sum L R} over sub-block k,
 *     k < (n + B - 1) / B: unlike the meter's, the last, partial sub-block is included; n implies its length.
 *   mgx_audit_gate, the device-free rule, from the report's sums and the sub-block sums:
 *     dc[c] = sum[c] / n;  rms[c] = sqrt(sumsq[c] / n);  balance_db = 10 log10(sumsq[0] / sumsq[1]);
 *     correlation = sum_lr / sqrt(sumsq[0] sumsq[1]);
 *     mono_loss_db = 10 log10((sumsq[0] + sumsq[1] + 2 sum_lr) / (2 (sumsq[0] + sumsq[1]))): (L + R) / 2 against the mean
 *       channel power (a numerator that rounds below 0 counts as 0: -infinity);
 *     correlation_min / correlation_min_at = the minimum, and the index of its first sub-block, of the correlation over
 *       windows of 30 consecutive sub-blocks stepping one (each window's three sums added in sub-block order); a window
 *       whose mean power (sum L^2 + sum R^2) / (2 frames) is below 10^-7 (-70 dB) or one of whose channel sums is 0 is
 *       skipped; a track of fewer than 30 sub-blocks has the one window of all of them; of equal minima the earliest.
 *       Where nothing qualifies: NaN and -1.  Every ratio above is NaN where its denominator is 0 (n == 0 included).
 * mgx_audit: two launches on the handle's stream (csrc/audit_kernel.h), none of whose workgroups waits for another; it
 * waits for the result, fills the measured fields and applies mgx_audit_gate, so the report is complete.  Two calls on
 * the same input give the same bits.  sub_sums (host, [capacity][3], may be NULL) receives the sub-block sums and
 * *count (may be NULL) their number.  n_frames == 0 succeeds, launches nothing and gives zero counts and sums, positions
 * -1 and NaN ratios.  MGX_ERR_ARGUMENT, the message naming the field: a null h, limits, report or (n_frames > 0) x_dev;
 * x_dev not 16-byte aligned (what mgx_malloc returns is); n_frames negative; bits outside {0, 16, 24, 32}; sample_rate
 * below 8000; clip_level not finite or <= 0; clip_run < 1; silence_level negative or not finite; capacity below the
 * number of sub-blocks where sub_sums is given.  MGX_ERR_UNSUPPORTED: more than 500 million frames.  The handle is good
 * for the next call.
 * mgx_audit_gate needs no GPU: it reads report->sum, sumsq and sum_lr and writes frames, sub_blocks, sub_block_frames
 * and the derived figures; MGX_ERR_ARGUMENT for a null report, a negative count or n_frames, a null sub_sums with
 * count > 0, a sample_rate below 8000, and a count that is not (n_frames + B - 1) / B. */
typedef struct mgx_audit_limits {
    double clip_level;                   /* linear */
    double silence_level;                /* linear */
    int32_t clip_run;                    /* samples */
    int32_t reserved;
} mgx_audit_limits;
typedef struct mgx_audit_report {
    int64_t frames;
    int64_t nonfinite[2];
    int64_t clip_events[2], clip_samples[2], clip_longest[2], clip_first[2];
    int64_t head_silence, tail_silence, gap_longest, gap_at;
    int64_t sub_blocks;
    int32_t sub_block_frames;
    int32_t bits;
    double sum[2], sumsq[2], peak[2];
    double sum_lr;
    /* mgx_audit_gate's */
    double dc[2], rms[2];
    double balance_db, correlation, mono_loss_db;
    double correlation_min;
    int64_t correlation_min_at;
} mgx_audit_report;
int mgx_audit(mgx_handle* h, const void* x_dev, int64_t n_frames, int32_t bits, int32_t sample_rate,
              const mgx_audit_limits* limits, mgx_audit_report* report, double* sub_sums, int64_t capacity,
              int64_t* count);
int mgx_audit_gate(const double* sub_sums, int64_t count, int64_t n_frames, int32_t sample_rate, mgx_audit_report* report);

/* Clip repair: the short flat tops of a track that was clipped, rebuilt from the samples around them while the frames
 * are in HBM (the reference warns about a clipping target, checker.py, and masters it as it is).  Opt-in, part of the
 * new surface, like the audit that counts such runs.  DESIGN.md section 3.20.  Each channel on its own:
 *   input: x[n][2] float32; level L > 0, min_run >= 1, min_run <= max_run <= MGX_DECLIP_MAX_RUN, max_rise K >= 1.
 *   per sample, xd = (double)x[i]: high = finite and xd >= L; low = finite and xd <= -L.
 *   run [a, b): a maximal sequence of consecutive high samples, or of consecutive low ones; r = b - a.  A NaN or an
 *     infinity ends a run; a low run may follow a high one at once.
 *   a run is REPAIRED iff min_run <= r <= max_run, a >= 2, b + 1 <= n - 1 and the four anchors x[a-2], x[a-1], x[b],
 *     x[b+1] are finite.  Every other run is left as it is and counted once: short (r < min_run), else long
 *     (r > max_run), else edge (it lacks four finite anchors).
 *   a repaired run, from the anchors' ORIGINAL values (runs are independent of each other), every operation float64
 *   and rounded on its own (no fused multiply-add):
 *     h = (double)(r + 1);  p0 = x[a-1];  p1 = x[b];  m0 = h * (p0 - x[a-2]);  m1 = h * (x[b+1] - p1)
 *     for i = a - 1 + k, k = 1..r:   t = k / h;  t2 = t * t;  t3 = t2 * t
 *       y = ((2*t3 - 3*t2 + 1) * p0 + (t3 - 2*t2 + t) * m0) + ((3*t2 - 2*t3) * p1 + (t3 - t2) * m1)
 *     (sums from left to right): the cubic Hermite segment through the two inner anchors with the one-sided slopes.
 *     high run:  if (y > K L) y = K L;    out[i] = y > xd ? (float)y : x[i]         (K L is one product)
 *     low run:   if (y < -K L) y = -K L;  out[i] = y < xd ? (float)y : x[i]
 *   every other sample is copied bit for bit, the ones that are not finite included.
 *   report, per channel c: runs_repaired[c]; samples_repaired[c], the samples inside those runs; samples_raised[c], the
 *     samples whose output bits differ from the input's; longest_repaired[c] (0: none); first_repaired[c], the first
 *     frame of the first repaired run (-1: none); runs_short[c], runs_long[c], runs_edge[c]; peak_before[c] and
 *     peak_after[c] = max |.| over the finite samples of the input and of the output.
 * mgx_declip_check needs no GPU.  MGX_ERR_ARGUMENT, the message naming the field: params null; level not finite or
 * <= 0; max_rise not finite or < 1; min_run < 1; max_run outside [min_run, MGX_DECLIP_MAX_RUN].
 * mgx_declip: n_frames frames of x_dev -> out_dev in two launches on the handle's stream (csrc/declip_kernel.h: k_declip,
 * a workgroup per 4096 frames with a halo of max-run + 2 frames either side; k_declip_fold, which folds the workgroups'
 * counters), none of whose workgroups waits for another; no atomics: two calls on the same input give the same bytes.
 * Queued; it waits for the result only where `report` (host, may be NULL) is given.  n_frames == 0 succeeds, launches
 * nothing and reports zeros and -1.  MGX_ERR_ARGUMENT beyond mgx_declip_check's: a null h, x_dev or out_dev; n_frames
 * negative; x_dev or out_dev not 16-byte aligned (what mgx_malloc returns is); out_dev overlapping x_dev (out of place
 * only: a workgroup reads its neighbours' frames).  MGX_ERR_UNSUPPORTED: more than 500 million frames.  The handle is
 * good for the next call.
 * mgx_declip_report_read: the report of the handle's most recent mgx_declip call, for a caller that queued it without
 * one and reads it where it waits anyway; it waits for the stream.  Zeros and -1 where that call had no frames or there
 * was none.  MGX_ERR_ARGUMENT: a null h or report. */
#define MGX_DECLIP_MAX_RUN 512
typedef struct mgx_declip_params {
    double level;                        /* linear */
    double max_rise;                     /* a repaired sample stays within max_rise * level */
    int32_t min_run;                     /* samples */
    int32_t max_run;
} mgx_declip_params;
typedef struct mgx_declip_report {
    int64_t runs_repaired[2], samples_repaired[2], samples_raised[2], longest_repaired[2], first_repaired[2];
    int64_t runs_short[2], runs_long[2], runs_edge[2];
    double peak_before[2], peak_after[2];
} mgx_declip_report;
int mgx_declip_check(const mgx_declip_params* params);
int mgx_declip(mgx_handle* h, const float* x_dev, int64_t n_frames, const mgx_declip_params* params, float* out_dev,
               mgx_declip_report* report);
int mgx_declip_report_read(mgx_handle* h, mgx_declip_report* report);

/* Visuals: the pictures a mastering front end shows -- a waveform overview and a spectrogram -- computed from (n, 2)
 * float32 frames while they are in HBM; what comes back is a few hundred kilobytes (the reference has nothing of the
 * kind; a caller would download every frame and transform on the host).  Part of the new surface, like the meter and the
 * audit.  DESIGN.md section 3.18.
 * (V1) Overview.  W columns, 1 <= W <= min(n, 65536).  Column c covers frames [floor(c n / W), floor((c + 1) n / W)),
 *   in 64-bit arithmetic.  Per column and channel: the smallest and the largest sample, as the float32 values
 *   themselves, and the float64 sum of squares (a float32 square is exact in float64).  A NaN is skipped by the minimum
 *   and the maximum (fminf / fmaxf from +inf / -inf, as numpy's fmin / fmax) and enters the sum as it is.
 * (V2) Spectrogram.
 *   parameters: N = 2^log2_fft, log2_fft in 8..14; hop H, 1 <= H <= N; W columns; channels 0 (left, right) or 1 (mid,
 *     side exactly as the analysis forms them: m = (L + R) * 0.5f, s = m - R, in float32); B bands, edges[0..B].
 *   window: periodic Hann, w[i] = 0.5 - 0.5 cos(2 pi i / N), computed in float64 and rounded to float32; sum w is the
 *     float64 sum of those float32 values.
 *   hops: centred.  Hop t is frames [t H - N/2, t H + N/2), frames outside the track being zero; T = floor((n - 1) / H) + 1.
 *   power: per hop and channel P_t[k] = |X_t[k]|^2 (2 / sum w)^2, k = 0 .. N/2, X the N-point DFT of the windowed hop:
 *     a full-scale sine on a bin centre reads 1.0.  DC and Nyquist are NOT treated specially: having no mirror bin they
 *     read four times what the convention of a real tone would give them.
 *   time pooling: with 1 <= W <= T, column c is the mean of P_t over t in [floor(c T / W), floor((c + 1) T / W));
 *     columns == 0 means W = T; W = 1 is the long-term average spectrum.
 *   frequency pooling: band b is the mean of bins [edges[b], edges[b + 1]); edges strictly ascending, edges[0] >= 0,
 *     edges[B] <= N/2 + 1.  edges = 0, 1, .., N/2 + 1 gives every bin.
 *   output: linear power, float32, [W][2][B] (column, channel, band), on the host.  Decibels are the caller's.
 * (V3) Empty input: n == 0 gives zero hops and zero columns, launches nothing and returns 0, as mgx_audit does.
 * (V4) Limits: more than 500 million frames is MGX_ERR_UNSUPPORTED; so is a spectrogram whose partial spectra
 *   (W ceil(ceil(T / W) / 32) (N + 2) floats) or whose picture (2 W B floats) exceed 2 GiB -- it asks for fewer columns.
 *   Every other bad argument is MGX_ERR_ARGUMENT; mgx_last_error names the field and the offending value.
 * mgx_spectrogram_plan needs no device: it makes every refusal of (V2) and (V4) that depends on the numbers alone and
 * returns T in *hops and W in *columns (either may be NULL).
 * mgx_spectrogram: two launches on the handle's stream (csrc/visuals_kernel.h: k_spectrogram<log2_fft>, a workgroup per
 * run of at most 32 consecutive hops of one column, accumulated in float32 in hop order; k_spectro_pool, which adds a
 * column's runs in order and a band's bins in float64), none of whose workgroups waits for another; no atomics: two calls
 * on the same input give the same bits.  It waits for the result (as mgx_loudness does).  `power` (host) receives
 * [W][2][B] floats, `capacity` is the number of floats it holds, *count (may be NULL) receives W.  Beyond the plan's
 * refusals: a null h, power or (n > 0) x_dev; x_dev not 8-byte aligned; capacity below 2 W B.
 * mgx_overview: two launches (k_overview, a workgroup per 16384 frames of a column; k_overview_fold, which folds a
 * column's shares in order), waits.  minmax (host) receives [W][2][2] = column, channel, {smallest, largest}; sumsq
 * [W][2].  Refusals as (V1), (V4): a null h, minmax, sumsq or (n > 0) x_dev, a misaligned x_dev, n negative, columns
 * outside 1 .. min(n, 65536) (V3 first: with n == 0 the columns are not looked at). */
typedef struct mgx_spectrogram_spec {
    int32_t log2_fft;
    int32_t hop;
    int32_t columns;                     /* 0: one per hop */
    int32_t channels;                    /* 0: left / right, 1: mid / side */
    int32_t bands;
} mgx_spectrogram_spec;
int mgx_spectrogram_plan(int64_t n_frames, const mgx_spectrogram_spec* spec, const int32_t* edges, int64_t* hops,
                         int32_t* columns);
int mgx_spectrogram(mgx_handle* h, const float* x_dev, int64_t n_frames, const mgx_spectrogram_spec* spec,
                    const int32_t* edges, float* power, int64_t capacity, int64_t* count);
int mgx_overview(mgx_handle* h, const float* x_dev, int64_t n_frames, int32_t columns, float* minmax /* [W][2][2] */,
                 double* sumsq /* [W][2] */);

/* A/B previews (matchering/preview_creator.py:30-94) on frames that are still in HBM.
 * mgx_window_energy: dsp.py:128-143 (strided_app_2d + batch_rms_2d): sum of squares over both channels of
 * every window of `size` frames taken every `step` frames (`size` > n: the whole track is the one window);
 * energy[w] for w < *count (host array of `capacity` doubles); the loudest window is the argmax (the square
 * root and the mean of dsp.py:80-86 are monotone).  Waits for the stream.
 * mgx_preview_cut: frames [begin, begin + size) clipped to +-clip_limit (dsp.py:109-110; <= 0: not clipped)
 * and faded in and out over `fade` frames (dsp.py:146-152, numpy.linspace(0, 1, fade)), written to
 * out_dev [size][2]; queued on the handle's stream. */
int mgx_window_energy(mgx_handle* h, const float* x_dev, int64_t n, int64_t size, int64_t step, double* energy,
                      int64_t capacity, int64_t* count);
int mgx_preview_cut(mgx_handle* h, const float* x_dev, int64_t n, int64_t begin, int64_t size, int64_t fade,
                    double clip_limit, float* out_dev);

/* Measurement aid (bench.py): with timing enabled, mgx_master brackets each of
 * its stages with HIP events recorded on the handle's own stream (no synchronisation is added);
 * mgx_stage_times waits for the stream and returns the device time of every stage of the LAST
 * mgx_master call in milliseconds, -1 for a stage that did not run.  The stages are those of
 * stages.py:210-272 with `convolve` (match_frequencies.py:104-119) and the limiter
 * (hyrax.py:78-99) on their own, since each is a single kernel launch. */
enum mgx_stage {
    MGX_STAGE_ANALYZE = 0,          /* match_levels.py:134-161 + match_frequencies.py:30-42, target AND
                                       reference: ONE launch of k_analyze */
    MGX_STAGE_DESIGN_FIR = 1,       /* match_levels.py:62-71, match_frequencies.py:45-101 */
    MGX_STAGE_FILTER_SPECTRA = 2,   /* transforms of the FIR pair the convolution multiplies by */
    MGX_STAGE_CONVOLVE = 3,         /* match_frequencies.py:104-119: ONE launch of k_conv */
    MGX_STAGE_CORRECT_LEVELS = 4,   /* stages.py:138-170 */
    MGX_STAGE_SCALE_OUTPUTS = 5,    /* stages.py:185-191 */
    MGX_STAGE_LIMIT = 6,            /* hyrax.py:78-99: ONE launch of the limiter kernel */
    MGX_STAGE_COUNT = 7
};
int mgx_stage_timing(mgx_handle* h, int32_t enable);
int mgx_stage_times(mgx_handle* h, float* ms /* [MGX_STAGE_COUNT] */);

/* Code bytes of the seven big kernel families (analyze, match_curve, conv_prep, conv, correction_round,
 * correction_tail, limit), bytes[family * 16 + variant] with variant = log2 of the transform size (0 / 1 for the
 * 256 / 1024-block limiter, 0 for the untemplated kernels, 15 in the conv family for the two-partition
 * delay-line kernel, 6 in the conv and conv_prep families for the N = 4F kernel of 4096 taps), as read from this
 * library's own device code
 * object -- what the kernels' first workgroups read as data to put their code into the L2 ahead of the
 * instruction cache ("fast and slow boxes").  Returns the number of families; needs no
 * GPU.  Zeros mean the code object could not be read and the kernels do not warm. */
int mgx_code_bytes(int32_t* bytes, int32_t capacity);

/* Device address of the FIR pair ([2][fft_size] float32: mid taps then side taps, level gain
 * not included) designed by the last mgx_master / uploaded by the last mgx_convolve on this
 * handle -- the payload of the RCCL exchange below.  The address is good until the next mgx_master* or
 * mgx_convolve call on the handle: a handle keeps two such tables and consecutive calls may use them in
 * turn, so a later call's FIR need not appear behind an address obtained earlier.  Copy the table out
 * (or pass the address as fir_dev to the very next call) and ask again after every call. */
int mgx_last_fir(mgx_handle* h, void** taps_dev, int32_t* taps);

/* ---- multi-GPU: one process per GPU, FIR taps over RCCL/xGMI ---------------- */
int mgx_comm_unique_id(void* id128);                                  /* ncclGetUniqueId, 128 bytes */
int mgx_comm_init(mgx_handle* h, const void* id128, int rank, int world);
int mgx_comm_count(mgx_handle* h, int32_t* ranks);                    /* ncclCommCount: the ranks RCCL itself sees */
int mgx_comm_broadcast_f32(mgx_handle* h, float* dev, int64_t count, int root);
int mgx_comm_allgather_f32(mgx_handle* h, const float* send_dev, float* recv_dev, int64_t count);
int mgx_comm_destroy(mgx_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* MGX_H */
