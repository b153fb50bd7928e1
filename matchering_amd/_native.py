"""ctypes binding of libmgx.so (include/mgx.h).

The library is the product: there is no Python or numpy implementation of the
hot path behind it.  If the shared object is missing it is built in place with
hipcc (matchering_amd/build.py); if that is impossible the import fails loudly.
"""

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MGX_LIB") or os.path.join(_HERE, "libmgx.so")

c_float_p = ctypes.POINTER(ctypes.c_float)
c_double_p = ctypes.POINTER(ctypes.c_double)
c_int32_p = ctypes.POINTER(ctypes.c_int32)
c_int64_p = ctypes.POINTER(ctypes.c_int64)


class MgxConfig(ctypes.Structure):
    """mgx_config (include/mgx.h)."""

    _fields_ = [
        ("internal_sample_rate", ctypes.c_int32),
        ("fft_size", ctypes.c_int32),
        ("lin_log_oversampling", ctypes.c_int32),
        ("rms_correction_steps", ctypes.c_int32),
        ("max_piece_size", ctypes.c_double),
        ("threshold", ctypes.c_double),
        ("min_value", ctypes.c_double),
        ("lowess_frac", ctypes.c_double),
        ("lowess_it", ctypes.c_int32),
        ("reserved0", ctypes.c_int32),
        ("lowess_delta", ctypes.c_double),
        ("attack_ms", ctypes.c_double),
        ("hold_ms", ctypes.c_double),
        ("release_ms", ctypes.c_double),
        ("attack_filter_coefficient", ctypes.c_double),
        ("hold_filter_order", ctypes.c_int32),
        ("release_filter_order", ctypes.c_int32),
        ("hold_filter_coefficient", ctypes.c_double),
        ("release_filter_coefficient", ctypes.c_double),
    ]


class MgxReport(ctypes.Structure):
    """mgx_report (include/mgx.h)."""

    _fields_ = [
        ("final_amplitude_coefficient", ctypes.c_double),
        ("target_match_rms", ctypes.c_double),
        ("reference_match_rms", ctypes.c_double),
        ("rms_coefficient", ctypes.c_double),
        ("correction_coefficients", ctypes.c_double * 16),
        ("normalize_coefficient", ctypes.c_double),
        ("result_peak", ctypes.c_double),
        ("target_divisions", ctypes.c_int32),
        ("reference_divisions", ctypes.c_int32),
        ("target_piece", ctypes.c_int64),
        ("reference_piece", ctypes.c_int64),
        ("target_loud_count", ctypes.c_int32),
        ("reference_loud_count", ctypes.c_int32),
        ("limiter_active", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class MgxProfileHeader(ctypes.Structure):
    """mgx_profile_header (include/mgx.h): the fixed head of a reference profile; 2 * (fft_size / 2 + 1) float64 follow."""

    _fields_ = [
        ("magic", ctypes.c_uint32),
        ("version", ctypes.c_uint32),
        ("internal_sample_rate", ctypes.c_int32),
        ("fft_size", ctypes.c_int32),
        ("max_piece_size", ctypes.c_double),
        ("threshold", ctypes.c_double),
        ("min_value", ctypes.c_double),
        ("frames", ctypes.c_int64),
        ("piece", ctypes.c_int64),
        ("divisions", ctypes.c_int32),
        ("loud_count", ctypes.c_int32),
        ("peak", ctypes.c_double),
        ("amplitude_coefficient", ctypes.c_double),
        ("average_rms", ctypes.c_double),
        ("match_rms", ctypes.c_double),
    ]


class MgxLoudnessReport(ctypes.Structure):
    """mgx_loudness_report (include/mgx.h)."""

    _fields_ = [
        ("integrated", ctypes.c_double),
        ("range", ctypes.c_double),
        ("momentary_max", ctypes.c_double),
        ("short_term_max", ctypes.c_double),
        ("true_peak", ctypes.c_double),
        ("sample_peak", ctypes.c_double),
        ("sub_blocks", ctypes.c_int64),
        ("sub_block_frames", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class MgxAuditLimits(ctypes.Structure):
    """mgx_audit_limits (include/mgx.h)."""

    _fields_ = [
        ("clip_level", ctypes.c_double),
        ("silence_level", ctypes.c_double),
        ("clip_run", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class MgxAuditReport(ctypes.Structure):
    """mgx_audit_report (include/mgx.h)."""

    _fields_ = [
        ("frames", ctypes.c_int64),
        ("nonfinite", ctypes.c_int64 * 2),
        ("clip_events", ctypes.c_int64 * 2),
        ("clip_samples", ctypes.c_int64 * 2),
        ("clip_longest", ctypes.c_int64 * 2),
        ("clip_first", ctypes.c_int64 * 2),
        ("head_silence", ctypes.c_int64),
        ("tail_silence", ctypes.c_int64),
        ("gap_longest", ctypes.c_int64),
        ("gap_at", ctypes.c_int64),
        ("sub_blocks", ctypes.c_int64),
        ("sub_block_frames", ctypes.c_int32),
        ("bits", ctypes.c_int32),
        ("sum", ctypes.c_double * 2),
        ("sumsq", ctypes.c_double * 2),
        ("peak", ctypes.c_double * 2),
        ("sum_lr", ctypes.c_double),
        ("dc", ctypes.c_double * 2),
        ("rms", ctypes.c_double * 2),
        ("balance_db", ctypes.c_double),
        ("correlation", ctypes.c_double),
        ("mono_loss_db", ctypes.c_double),
        ("correlation_min", ctypes.c_double),
        ("correlation_min_at", ctypes.c_int64),
    ]


class MgxDeclipParams(ctypes.Structure):
    """mgx_declip_params (include/mgx.h)."""

    _fields_ = [
        ("level", ctypes.c_double),
        ("max_rise", ctypes.c_double),
        ("min_run", ctypes.c_int32),
        ("max_run", ctypes.c_int32),
    ]


class MgxDeclipReport(ctypes.Structure):
    """mgx_declip_report (include/mgx.h)."""

    _fields_ = [
        ("runs_repaired", ctypes.c_int64 * 2),
        ("samples_repaired", ctypes.c_int64 * 2),
        ("samples_raised", ctypes.c_int64 * 2),
        ("longest_repaired", ctypes.c_int64 * 2),
        ("first_repaired", ctypes.c_int64 * 2),
        ("runs_short", ctypes.c_int64 * 2),
        ("runs_long", ctypes.c_int64 * 2),
        ("runs_edge", ctypes.c_int64 * 2),
        ("peak_before", ctypes.c_double * 2),
        ("peak_after", ctypes.c_double * 2),
    ]


class MgxSpectrogramSpec(ctypes.Structure):
    """mgx_spectrogram_spec (include/mgx.h)."""

    _fields_ = [
        ("log2_fft", ctypes.c_int32),
        ("hop", ctypes.c_int32),
        ("columns", ctypes.c_int32),
        ("channels", ctypes.c_int32),
        ("bands", ctypes.c_int32),
    ]


class MgxDelivery(ctypes.Structure):
    """mgx_delivery (include/mgx.h)."""

    _fields_ = [
        ("target_lufs", ctypes.c_double),
        ("ceiling_dbtp", ctypes.c_double),
        ("bits", ctypes.c_int32),
        ("dither", ctypes.c_int32),
        ("seed", ctypes.c_uint64),
    ]


class MgxDeliveryResult(ctypes.Structure):
    """mgx_delivery_result (include/mgx.h)."""

    _fields_ = [
        ("gain", ctypes.c_double),
        ("achieved_lufs", ctypes.c_double),
        ("achieved_true_peak", ctypes.c_double),
        ("shortfall_lu", ctypes.c_double),
        ("limited_by", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class MgxDeliveryLimitPlan(ctypes.Structure):
    """mgx_delivery_limit_plan (include/mgx.h)."""

    _fields_ = [
        ("pre_gain_db", ctypes.c_double),
        ("ceiling", ctypes.c_double),
        ("run", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class MgxNoiseShaper(ctypes.Structure):
    """mgx_noise_shaper (include/mgx.h)."""

    _fields_ = [
        ("taps", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("c", ctypes.c_double * 16),
    ]


class MgxEqShape(ctypes.Structure):
    """mgx_eq_shape (include/mgx.h)."""

    _fields_ = [
        ("amount", ctypes.c_double),
        ("max_boost_db", ctypes.c_double),
        ("max_cut_db", ctypes.c_double),
        ("phase", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


EQ_BANDS_MAX = 8                # MGX_EQ_BANDS_MAX


class MgxEqBand(ctypes.Structure):
    """mgx_eq_band (include/mgx.h)."""

    _fields_ = [
        ("kind", ctypes.c_int32),
        ("channels", ctypes.c_int32),
        ("hz", ctypes.c_double),
        ("gain_db", ctypes.c_double),
        ("q", ctypes.c_double),
    ]


class MgxEqTone(ctypes.Structure):
    """mgx_eq_tone (include/mgx.h)."""

    _fields_ = [
        ("low_hz", ctypes.c_double),
        ("high_hz", ctypes.c_double),
        ("range_octaves", ctypes.c_double),
        ("side_amount", ctypes.c_double),
        ("mono_below_hz", ctypes.c_double),
        ("mono_octaves", ctypes.c_double),
        ("tilt_db_per_octave", ctypes.c_double),
        ("tilt_pivot_hz", ctypes.c_double),
        ("band_count", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("bands", MgxEqBand * EQ_BANDS_MAX),
    ]


PROFILE_MAGIC = 0x5250474D      # MGX_PROFILE_MAGIC
PROFILE_VERSION = 1             # MGX_PROFILE_VERSION
PROFILE_MERGE_MAX = 64          # MGX_PROFILE_MERGE_MAX
LIMIT_PASSES_MAX = 16           # MGX_LIMIT_PASSES_MAX
SHAPER_TAPS_MAX = 16            # MGX_SHAPER_TAPS_MAX
SHAPER_SEGMENT = 1024           # MGX_SHAPER_SEGMENT
SHAPER_WARMUP = 64              # MGX_SHAPER_WARMUP


# every symbol include/mgx.h declares: name -> (restype, argtypes)
_VP = ctypes.c_void_p
SYMBOLS = {
    "mgx_version": (ctypes.c_int, []),
    "mgx_last_error": (ctypes.c_char_p, []),
    "mgx_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "mgx_device_pci_bus_id": (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_int32]),
    "mgx_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_VP)]),
    "mgx_destroy": (ctypes.c_int, [_VP]),
    "mgx_config_default": (ctypes.c_int, [ctypes.POINTER(MgxConfig)]),
    "mgx_malloc": (ctypes.c_int, [_VP, ctypes.c_size_t, ctypes.POINTER(_VP)]),
    "mgx_free": (ctypes.c_int, [_VP, _VP]),
    "mgx_memcpy_h2d": (ctypes.c_int, [_VP, _VP, _VP, ctypes.c_size_t]),
    "mgx_memcpy_d2h": (ctypes.c_int, [_VP, _VP, _VP, ctypes.c_size_t]),
    "mgx_synchronize": (ctypes.c_int, [_VP]),
    "mgx_timer_start": (ctypes.c_int, [_VP]),
    "mgx_timer_stop": (ctypes.c_int, [_VP, c_float_p]),
    "mgx_master": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, _VP, ctypes.c_int64, ctypes.POINTER(MgxConfig),
                                  _VP, _VP, _VP, ctypes.POINTER(MgxReport)]),
    "mgx_master_with_fir": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, _VP, ctypes.c_int64, ctypes.POINTER(MgxConfig),
                                           _VP, _VP, _VP, _VP, ctypes.POINTER(MgxReport)]),
    "mgx_profile_bytes": (ctypes.c_int, [ctypes.POINTER(MgxConfig), ctypes.POINTER(ctypes.c_size_t)]),
    "mgx_reference_profile": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.POINTER(MgxConfig), _VP]),
    "mgx_master_with_profile": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, _VP, ctypes.POINTER(MgxConfig), _VP,
                                               _VP, _VP, _VP, ctypes.POINTER(MgxReport)]),
    "mgx_profile_merge": (ctypes.c_int, [_VP, ctypes.POINTER(_VP), c_int32_p, ctypes.c_int32, ctypes.POINTER(MgxConfig), _VP]),
    "mgx_analyze": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.POINTER(MgxConfig), ctypes.c_int,
                                   c_double_p, c_double_p, c_double_p, c_int32_p, c_int64_p,
                                   c_double_p, c_int32_p, c_double_p, c_double_p]),
    "mgx_design_fir": (ctypes.c_int, [ctypes.POINTER(MgxConfig), c_double_p, c_double_p, c_double_p,
                                      c_double_p, c_double_p]),
    "mgx_eq_shape_check": (ctypes.c_int, [ctypes.POINTER(MgxConfig), ctypes.POINTER(MgxEqShape)]),
    "mgx_shape_fir": (ctypes.c_int, [ctypes.POINTER(MgxConfig), ctypes.POINTER(MgxEqShape), c_double_p, c_double_p]),
    "mgx_master_shaped": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, _VP, ctypes.c_int64, _VP, ctypes.POINTER(MgxConfig),
                                         ctypes.POINTER(MgxEqShape), _VP, _VP, _VP, ctypes.POINTER(MgxReport)]),
    "mgx_eq_tone_default": (ctypes.c_int, [ctypes.POINTER(MgxEqTone)]),
    "mgx_eq_tone_check": (ctypes.c_int, [ctypes.POINTER(MgxConfig), ctypes.POINTER(MgxEqShape), ctypes.POINTER(MgxEqTone)]),
    "mgx_eq_tone_curve": (ctypes.c_int, [ctypes.POINTER(MgxConfig), ctypes.POINTER(MgxEqShape), ctypes.POINTER(MgxEqTone),
                                         ctypes.c_int32, c_double_p, c_double_p, c_double_p]),
    "mgx_tone_fir": (ctypes.c_int, [ctypes.POINTER(MgxConfig), ctypes.POINTER(MgxEqShape), ctypes.POINTER(MgxEqTone),
                                    ctypes.c_int32, c_double_p, c_double_p]),
    "mgx_master_eq": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, _VP, ctypes.c_int64, _VP, ctypes.POINTER(MgxConfig),
                                     ctypes.POINTER(MgxEqShape), ctypes.POINTER(MgxEqTone), _VP, _VP, _VP,
                                     ctypes.POINTER(MgxReport)]),
    "mgx_convolve": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, c_double_p, c_double_p, ctypes.c_int32,
                                    ctypes.c_double, _VP, _VP, c_double_p]),
    "mgx_host_alloc": (ctypes.c_int, [ctypes.c_size_t, ctypes.POINTER(_VP)]),
    "mgx_host_free": (ctypes.c_int, [_VP]),
    "mgx_memcpy_h2d_async": (ctypes.c_int, [_VP, _VP, _VP, ctypes.c_size_t]),
    "mgx_memcpy_d2h_async": (ctypes.c_int, [_VP, _VP, _VP, ctypes.c_size_t]),
    "mgx_stage_timing": (ctypes.c_int, [_VP, ctypes.c_int32]),
    "mgx_stage_times": (ctypes.c_int, [_VP, c_float_p]),
    "mgx_code_bytes": (ctypes.c_int, [c_int32_p, ctypes.c_int32]),
    "mgx_clipped_piece_sumsq": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                               ctypes.c_double, c_double_p]),
    "mgx_limit": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.POINTER(MgxConfig), ctypes.c_double,
                                 ctypes.c_double, _VP, c_int32_p]),
    "mgx_scale": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.c_double, _VP]),
    "mgx_peak_count": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, c_double_p, ctypes.POINTER(ctypes.c_int64)]),
    "mgx_pcm_decode": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.c_int32, _VP]),
    "mgx_pcm_encode": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.c_int32, _VP]),
    "mgx_resample": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _VP,
                                    ctypes.c_int64, c_int64_p]),
    "mgx_resample_plan": (ctypes.c_int, [_VP, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_VP), c_int32_p, c_int32_p,
                                         c_int64_p]),
    "mgx_convert_rate": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, _VP, ctypes.c_int64,
                                        c_int64_p]),
    "mgx_window_energy": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_double_p,
                                         ctypes.c_int64, c_int64_p]),
    "mgx_loudness": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(MgxLoudnessReport), c_double_p,
                                    ctypes.c_int64, c_int64_p]),
    "mgx_loudness_gate": (ctypes.c_int, [c_double_p, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(MgxLoudnessReport)]),
    "mgx_audit": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(MgxAuditLimits),
                                 ctypes.POINTER(MgxAuditReport), c_double_p, ctypes.c_int64, c_int64_p]),
    "mgx_audit_gate": (ctypes.c_int, [c_double_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                      ctypes.POINTER(MgxAuditReport)]),
    "mgx_declip_check": (ctypes.c_int, [ctypes.POINTER(MgxDeclipParams)]),
    "mgx_declip": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.POINTER(MgxDeclipParams), _VP,
                                  ctypes.POINTER(MgxDeclipReport)]),
    "mgx_declip_report_read": (ctypes.c_int, [_VP, ctypes.POINTER(MgxDeclipReport)]),
    "mgx_spectrogram_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.POINTER(MgxSpectrogramSpec), ctypes.POINTER(ctypes.c_int32),
                                            c_int64_p, ctypes.POINTER(ctypes.c_int32)]),
    "mgx_spectrogram": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.POINTER(MgxSpectrogramSpec),
                                       ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float), ctypes.c_int64, c_int64_p]),
    "mgx_overview": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_float), c_double_p]),
    "mgx_delivery_gain": (ctypes.c_int, [ctypes.POINTER(MgxDelivery), ctypes.POINTER(MgxLoudnessReport),
                                         ctypes.POINTER(MgxDeliveryResult)]),
    "mgx_deliver": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.c_double, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64,
                                   _VP]),
    "mgx_tp_limit": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_double,
                                    _VP, c_double_p]),
    "mgx_delivery_limit_step": (ctypes.c_int, [ctypes.POINTER(MgxDelivery), ctypes.POINTER(MgxLoudnessReport), ctypes.c_int32,
                                               c_double_p, c_double_p, ctypes.c_int32, ctypes.c_double,
                                               ctypes.POINTER(MgxDeliveryLimitPlan)]),
    "mgx_noise_shaper_preset": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(MgxNoiseShaper)]),
    "mgx_delivery_gain_shaped": (ctypes.c_int, [ctypes.POINTER(MgxDelivery), ctypes.POINTER(MgxNoiseShaper),
                                                ctypes.POINTER(MgxLoudnessReport), ctypes.POINTER(MgxDeliveryResult)]),
    "mgx_delivery_limit_step_shaped": (ctypes.c_int, [ctypes.POINTER(MgxDelivery), ctypes.POINTER(MgxNoiseShaper),
                                                      ctypes.POINTER(MgxLoudnessReport), ctypes.c_int32, c_double_p, c_double_p,
                                                      ctypes.c_int32, ctypes.c_double, ctypes.POINTER(MgxDeliveryLimitPlan)]),
    "mgx_deliver_shaped": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.c_double, ctypes.c_int32,
                                          ctypes.POINTER(MgxNoiseShaper), ctypes.c_uint64, _VP]),
    "mgx_preview_cut": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                       ctypes.c_double, _VP]),
    "mgx_last_fir": (ctypes.c_int, [_VP, ctypes.POINTER(_VP), c_int32_p]),
    "mgx_comm_unique_id": (ctypes.c_int, [_VP]),
    "mgx_comm_init": (ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int]),
    "mgx_comm_count": (ctypes.c_int, [_VP, c_int32_p]),
    "mgx_comm_broadcast_f32": (ctypes.c_int, [_VP, _VP, ctypes.c_int64, ctypes.c_int]),
    "mgx_comm_allgather_f32": (ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int64]),
    "mgx_comm_destroy": (ctypes.c_int, [_VP]),
}


# enum mgx_stage (include/mgx.h), in order
STAGES = ("analyze", "design_fir", "filter_spectra", "convolve", "correct_levels", "scale_outputs", "limit")


ERR_RETRY = -6          # enum mgx_status MGX_ERR_RETRY (include/mgx.h)
ERR_UNSUPPORTED = -4    # ... MGX_ERR_UNSUPPORTED
ERR_ARGUMENT = -1       # ... MGX_ERR_ARGUMENT


class MgxError(RuntimeError):
    """A libmgx call failed; ``code`` is the negative mgx_status."""

    def __init__(self, code, message):
        super().__init__(f"libmgx error {code}: {message}")
        self.code = code

    @property
    def retry(self):
        """The handle recovered from a device-side wait that expired (the GPU is shared): what was queued since the
        last synchronisation is lost, the same calls made again succeed (``MGX_ERR_RETRY``)."""
        return self.code == ERR_RETRY


_lib = None


def library():
    """Load (building first if needed) libmgx.so and declare every prototype."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.environ.get("MGX_LIB"):
        # build() compares a digest of csrc/ and include/mgx.h with the one the binary was made from
        # and returns at once when they agree: an edited kernel or struct never meets a stale binary
        from . import build as _build

        try:
            _build.build()
        except Exception as exc:               # noqa: BLE001 -- no hipcc on this host, a read-only tree ...
            if not os.path.exists(LIB_PATH):
                raise
            import warnings

            warnings.warn(f"libmgx.so could not be rebuilt from the sources beside it ({exc!r}); loading the "
                          f"existing binary, which may be older than they are", RuntimeWarning)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError here = header and library disagree
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(code):
    if code != 0:
        raise MgxError(code, library().mgx_last_error().decode("utf-8", "replace"))
