"""ctypes binding of include/tamcmc_accel.h.

There is no CPU fallback: if libtamcmc_accel.so is missing, or no HIP device is usable, every entry
point raises AccelError.  Build the library with ``python -c "import __graft_entry__ as g; g.build()"``
or ``make -C tamcmc-c-_amd/csrc``.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# error codes of tamcmc_accel.h
OK, E_INVALID, E_NODEVICE, E_HIP, E_MODEL_DISABLED, E_UNKNOWN_MODEL, E_NOMEM, E_NOVARS, E_NOGRAD = range(9)
CHAIN_OK, CHAIN_NAN, CHAIN_EMPTY_WINDOW = 0, 1, 2

EXPORTS = [
    "tamcmc_ctx_create", "tamcmc_ctx_set_vars", "tamcmc_ctx_set_spectra", "tamcmc_ctx_set_chain_spectrum",
    "tamcmc_eval_batch", "tamcmc_eval_batch_device",
    "tamcmc_eval_batch_begin", "tamcmc_eval_batch_end",
    "tamcmc_ctx_reserve",
    "tamcmc_eval_batch_arm", "tamcmc_eval_batch_fire", "tamcmc_eval_batch_disarm", "tamcmc_eval_batch_poll",
    "tamcmc_model_explicit", "tamcmc_ctx_set_stream", "tamcmc_ctx_synchronize", "tamcmc_ctx_profile",
    "tamcmc_ctx_kernel_time", "tamcmc_ctx_clock_probe_begin", "tamcmc_ctx_clock_probe_end", "tamcmc_ctx_geometry", "tamcmc_ctx_geometry_grad", "tamcmc_ctx_destroy", "tamcmc_device_count",
    "tamcmc_strerror", "tamcmc_last_hip_error", "tamcmc_version",
    "tamcmc_group_create", "tamcmc_group_eval", "tamcmc_group_eval_device", "tamcmc_group_set_stream",
    "tamcmc_group_synchronize", "tamcmc_group_destroy",
    "tamcmc_group_eval_begin", "tamcmc_group_eval_end", "tamcmc_group_eval_poll", "tamcmc_group_members",
    "tamcmc_summary_create", "tamcmc_summary_push", "tamcmc_summary_push_device", "tamcmc_summary_result",
    "tamcmc_summary_reset", "tamcmc_summary_destroy", "tamcmc_summary_profile", "tamcmc_summary_kernel_time",
    "tamcmc_summary_quantiles_begin", "tamcmc_summary_quantiles_step", "tamcmc_summary_quantiles_result",
    "tamcmc_summary_quantiles_end",
    "tamcmc_summary_loo_begin", "tamcmc_summary_loo_result", "tamcmc_summary_loo_end",
    "tamcmc_summary_loo_pit_begin", "tamcmc_summary_loo_pit_result", "tamcmc_summary_loo_pit_kernel_time",
    "tamcmc_summary_predictive_enable", "tamcmc_summary_predictive_result", "tamcmc_summary_predictive_kernel_time",
    "tamcmc_summary_window_enable", "tamcmc_summary_window_result", "tamcmc_summary_window_kernel_time",
    "tamcmc_summary_wloo_begin", "tamcmc_summary_wloo_result", "tamcmc_summary_wloo_pit_begin", "tamcmc_summary_wloo_pit_result",
    "tamcmc_summary_wloo_pit_kernel_time", "tamcmc_summary_wloo_end",
    "tamcmc_summary_scan_enable", "tamcmc_summary_scan_result", "tamcmc_summary_scan_regions", "tamcmc_summary_scan_kernel_time",
    "tamcmc_summary_ess_begin", "tamcmc_summary_ess_result", "tamcmc_summary_ess_acov", "tamcmc_summary_ess_end",
    "tamcmc_summary_bandess_begin", "tamcmc_summary_bandess_result", "tamcmc_summary_bandess_counts", "tamcmc_summary_bandess_end",
    "tamcmc_scan_null_create", "tamcmc_scan_null_run", "tamcmc_scan_null_replicates", "tamcmc_scan_null_result",
    "tamcmc_scan_null_line", "tamcmc_scan_null_pvalue", "tamcmc_scan_null_variates", "tamcmc_scan_null_profile",
    "tamcmc_scan_null_kernel_time", "tamcmc_scan_null_destroy",
    "tamcmc_modetable_create", "tamcmc_modetable_columns", "tamcmc_modetable_column", "tamcmc_modetable_derive",
    "tamcmc_modetable_push", "tamcmc_modetable_result", "tamcmc_modetable_quantiles", "tamcmc_modetable_reset",
    "tamcmc_modetable_destroy", "tamcmc_modetable_kernel_time",
    "tamcmc_modediag_ess", "tamcmc_modediag_acov", "tamcmc_modediag_cov", "tamcmc_modediag_corr", "tamcmc_modediag_kernel_time",
    "tamcmc_moderank_diag", "tamcmc_moderank_acov", "tamcmc_moderank_series", "tamcmc_moderank_kernel_time",
]
# what include/tamcmc_accel_seismic.h declares (tamcmc_accel.h includes it)
SEISMIC_EXPORTS = ["tamcmc_modetable_indices_enable", "tamcmc_modetable_indices_info", "tamcmc_modetable_index_terms",
                   "tamcmc_seismic_kernel_time"]
# what include/tamcmc_accel_pdf.h declares (tamcmc_accel.h includes it)
PDF_EXPORTS = ["tamcmc_modepdf_hist", "tamcmc_modepdf_hpd", "tamcmc_modepdf_hist2d", "tamcmc_modepdf_kernel_time"]
MODEPDF_MAX_BINS, MODEPDF_MAX_BINS2D, MODEPDF_MAX_PAIRS, MODEPDF_MAX_MASS, MODEPDF_RANGE = 4096, 128, 1024, 8, 1
# what include/tamcmc_accel_compare.h declares (tamcmc_accel.h includes it)
COMPARE_EXPORTS = ["tamcmc_compare_create", "tamcmc_compare_info", "tamcmc_compare_diff", "tamcmc_compare_bootstrap",
                   "tamcmc_compare_replicates", "tamcmc_compare_z", "tamcmc_compare_prob", "tamcmc_compare_interval",
                   "tamcmc_compare_weights", "tamcmc_compare_stacking", "tamcmc_compare_stacking_cadence", "tamcmc_compare_variates",
                   "tamcmc_compare_profile", "tamcmc_compare_kernel_time", "tamcmc_compare_destroy"]
COMPARE_MAX_FITS, COMPARE_MAX_REPLICATES, COMPARE_TILE, COMPARE_STACK_TILE = 8, 1 << 24, 2048, 4096
COMPARE_METHODS = {"pseudo_bma": 0, "pseudo_bma_plus": 1, "stacking": 2}


class CompareTotals(C.Structure):
    """tamcmc_compare_totals"""
    _fields_ = [("n_included", C.c_int64), ("n_excluded", C.c_int64), ("n_better", C.c_int64), ("n_worse", C.c_int64),
                ("n_k_high", C.c_int64), ("elpd_diff", C.c_double), ("se_diff", C.c_double), ("diff_k_high", C.c_double)]


class CompareStackingInfo(C.Structure):
    """tamcmc_compare_stacking_info"""
    _fields_ = [("iterations", C.c_int64), ("converged", C.c_int32), ("table", C.c_int32), ("gap", C.c_double), ("f", C.c_double)]


class SummaryTotals(C.Structure):
    """tamcmc_summary_totals"""
    _fields_ = [("n_used", C.c_int64), ("n_rejected", C.c_int64), ("lppd_total", C.c_double), ("p_waic", C.c_double),
                ("waic", C.c_double)]


class SummaryLooTotals(C.Structure):
    """tamcmc_summary_loo_totals"""
    _fields_ = [("n_used", C.c_int64), ("n_rejected", C.c_int64), ("elpd_loo", C.c_double), ("p_loo", C.c_double),
                ("looic", C.c_double), ("k_max", C.c_double), ("n_k_high", C.c_int64), ("n_k_inf", C.c_int64)]


PIT_CELLS = 20          # TAMCMC_SUMMARY_PIT_CELLS


class SummaryPredictiveTotals(C.Structure):
    """tamcmc_summary_predictive_totals"""
    _fields_ = [("n_used", C.c_int64), ("n_rejected", C.c_int64), ("ks_D", C.c_double), ("min_log_sf", C.c_double),
                ("min_log_cdf", C.c_double), ("bin_min_log_sf", C.c_int64), ("bin_min_log_cdf", C.c_int64),
                ("pit_hist", C.c_int64 * PIT_CELLS)]


class SummaryLooPitTotals(C.Structure):
    """tamcmc_summary_loo_pit_totals"""
    _fields_ = [("n_used", C.c_int64), ("n_rejected", C.c_int64), ("ks_D", C.c_double), ("min_log_sf", C.c_double),
                ("min_log_cdf", C.c_double), ("min_is_ess", C.c_double), ("bin_min_log_sf", C.c_int64),
                ("bin_min_log_cdf", C.c_int64), ("bin_min_is_ess", C.c_int64), ("pit_hist", C.c_int64 * PIT_CELLS)]


class SummaryWindowTotals(C.Structure):
    """tamcmc_summary_window_totals"""
    _fields_ = [("n_used", C.c_int64), ("n_rejected", C.c_int64), ("n_windows", C.c_int64), ("W", C.c_int64), ("first", C.c_int64),
                ("ks_D", C.c_double), ("min_log_sf", C.c_double), ("min_log_cdf", C.c_double),
                ("win_min_log_sf", C.c_int64), ("win_min_log_cdf", C.c_int64), ("pit_hist", C.c_int64 * PIT_CELLS)]


class SummaryWlooTotals(C.Structure):
    """tamcmc_summary_wloo_totals"""
    _fields_ = [("n_used", C.c_int64), ("n_rejected", C.c_int64), ("n_windows", C.c_int64), ("W", C.c_int64), ("first", C.c_int64),
                ("elpd_lwo", C.c_double), ("p_lwo", C.c_double), ("k_max", C.c_double), ("n_k_high", C.c_int64), ("n_k_inf", C.c_int64)]


class SummaryScanTotals(C.Structure):
    """tamcmc_summary_scan_totals"""
    _fields_ = [("n_used", C.c_int64), ("n_rejected", C.c_int64), ("W", C.c_int64), ("n_positions", C.c_int64),
                ("min_log_sf", C.c_double), ("min_log_cdf", C.c_double), ("pos_min_log_sf", C.c_int64), ("pos_min_log_cdf", C.c_int64)]


class SummaryScanRegion(C.Structure):
    """tamcmc_summary_scan_region"""
    _fields_ = [("pos_first", C.c_int64), ("pos_last", C.c_int64), ("bin_first", C.c_int64), ("bin_last", C.c_int64),
                ("pos_min", C.c_int64), ("min_log", C.c_double), ("mean_resid_at_min", C.c_double)]


class SummaryEssTotals(C.Structure):
    """tamcmc_summary_ess_totals"""
    _fields_ = [("n_used", C.c_int64), ("n_rejected", C.c_int64), ("lag", C.c_int64),
                ("min_ess_M", C.c_double), ("min_ess_l", C.c_double), ("max_rhat", C.c_double),
                ("bin_min_ess_M", C.c_int64), ("bin_min_ess_l", C.c_int64), ("bin_max_rhat", C.c_int64),
                ("n_truncated_M", C.c_int64), ("n_truncated_l", C.c_int64), ("n_rhat_high", C.c_int64)]


MAX_QUANTILES = 8       # TAMCMC_SUMMARY_MAX_QUANTILES


class SummaryBandEssTotals(C.Structure):
    """tamcmc_summary_bandess_totals"""
    _fields_ = [("n_used", C.c_int64), ("n_rejected", C.c_int64), ("lag", C.c_int64), ("n_thresholds", C.c_int64),
                ("min_ess", C.c_double * MAX_QUANTILES), ("bin_min_ess", C.c_int64 * MAX_QUANTILES),
                ("n_truncated", C.c_int64 * MAX_QUANTILES), ("n_constant", C.c_int64 * MAX_QUANTILES)]


class ModeTableCol(C.Structure):
    """tamcmc_modetable_col"""
    _fields_ = [("kind", C.c_int32), ("mult", C.c_int32), ("order", C.c_int32), ("l", C.c_int32), ("m", C.c_int32),
                ("param_index", C.c_int32)]


class ModeTableTotals(C.Structure):
    """tamcmc_modetable_totals"""
    _fields_ = [("n_used", C.c_int64), ("n_rejected", C.c_int64), ("n_cols", C.c_int64), ("n_mult", C.c_int64)]


class ModeDiagTotals(C.Structure):
    """tamcmc_modediag_totals"""
    _fields_ = [("n_used", C.c_int64), ("lag", C.c_int64), ("min_ess", C.c_double), ("max_rhat", C.c_double),
                ("col_min_ess", C.c_int64), ("col_max_rhat", C.c_int64), ("n_truncated", C.c_int64), ("n_constant", C.c_int64),
                ("n_rhat_high", C.c_int64)]


class ModeRankTotals(C.Structure):
    """tamcmc_moderank_totals"""
    _fields_ = [("n_used", C.c_int64), ("lag", C.c_int64), ("min_ess_bulk", C.c_double), ("min_ess_tail", C.c_double),
                ("max_rhat", C.c_double), ("col_min_ess_bulk", C.c_int64), ("col_min_ess_tail", C.c_int64),
                ("col_max_rhat", C.c_int64), ("n_truncated", C.c_int64), ("n_constant", C.c_int64), ("n_rhat_high", C.c_int64)]


class SeismicInfo(C.Structure):
    """tamcmc_seismic_info"""
    _fields_ = [("n_base_cols", C.c_int64), ("n_index_cols", C.c_int64), ("n_radial", C.c_int64), ("n_unassigned", C.c_int64),
                ("n_base", C.c_int64), ("dnu_ref", C.c_double), ("eps_ref", C.c_double)]


MODERANK_NOUT = 8           # TAMCMC_MODERANK_NOUT
MODERANK_NSERIES = 4        # TAMCMC_MODERANK_NSERIES
MODERANK_OUT = ("ess_bulk", "ess_tail", "rhat", "tau_bulk", "rhat_bulk", "rhat_fold", "ess_q05", "ess_q95")
MODERANK_SERIES = ("z", "zfold", "i05", "i95")


def moderank_col_bytes(n, lag):
    """Device bytes one column of a rank_diag chunk takes at n rows and lag L (tamcmc_accel.h, tamcmc_moderank_diag)."""
    P = 2
    while P < n:
        P *= 2
    return 16 * P + 32 * (n + lag + 5) + 44


MODEDIAG_MAX_LAG = 1023     # TAMCMC_MODEDIAG_MAX_LAG
MODEDIAG_MAX_COLS = 1024    # TAMCMC_MODEDIAG_MAX_COLS

# TAMCMC_MODETABLE_* kind codes, in order
MODETABLE_KINDS = ("inclination", "eta", "a3", "asymmetry", "freq", "width", "height", "amplitude", "splitting",
                   "window_lo", "window_hi", "nu_m", "h_m")
# ... and those of the seismic indices (tamcmc_accel_seismic.h), which follow them
SEISMIC_KINDS = ("dnu_fit", "epsilon", "numax", "dnu_nl", "d2nu", "d02", "d13", "d01", "d10", "r02", "r01", "r13", "r10")


class AccelError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        super().__init__(f"{where}: error {code}: {detail}")


def library_path():
    """In-tree library; TAMCMC_ACCEL_LIB overrides it (developer knob for A/B builds)."""
    return os.environ.get("TAMCMC_ACCEL_LIB") or os.path.join(_HERE, "libtamcmc_accel.so")


def load_library():
    """Load the HIP library (once).  Raises AccelError if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise AccelError(-1, "load_library", f"{path} not found: build it first (no CPU fallback exists)")
    lib = C.CDLL(path)
    dp = C.POINTER(C.c_double)
    ip = C.POINTER(C.c_int32)
    vp = C.c_void_p
    lib.tamcmc_ctx_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_double, ip, C.c_int64, dp, dp, dp]
    lib.tamcmc_ctx_set_vars.argtypes = [vp, C.c_int32, ip]
    lib.tamcmc_eval_batch.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp, C.c_int32, ip, dp, ip]
    lib.tamcmc_eval_batch_device.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp]
    lib.tamcmc_model_explicit.argtypes = [vp, C.c_int32, dp, dp, ip]
    lib.tamcmc_ctx_reserve.argtypes = [vp, C.c_int32]
    lib.tamcmc_ctx_set_stream.argtypes = [vp, vp]
    lib.tamcmc_ctx_synchronize.argtypes = [vp]
    lib.tamcmc_ctx_profile.argtypes = [vp, C.c_int]
    lib.tamcmc_ctx_kernel_time.argtypes = [vp, dp, C.POINTER(C.c_int64)]
    lib.tamcmc_ctx_clock_probe_begin.argtypes = [vp, C.c_double]
    lib.tamcmc_ctx_clock_probe_end.argtypes = [vp, dp, dp]
    lib.tamcmc_ctx_geometry.argtypes = [vp, ip, ip, ip, ip]
    lib.tamcmc_ctx_geometry_grad.argtypes = [vp, ip, ip]
    lib.tamcmc_ctx_destroy.argtypes = [vp]
    lib.tamcmc_device_count.argtypes = []
    lib.tamcmc_strerror.argtypes = [C.c_int]
    lib.tamcmc_strerror.restype = C.c_char_p
    lib.tamcmc_last_hip_error.restype = C.c_char_p
    lib.tamcmc_version.restype = C.c_char_p
    lib.tamcmc_group_create.argtypes = [C.POINTER(vp), C.c_int32, C.POINTER(vp)]
    lib.tamcmc_group_eval.argtypes = [vp, ip, ip, dp, dp, dp, ip]
    lib.tamcmc_group_eval_device.argtypes = [vp, ip, ip, vp, vp, vp, vp]
    lib.tamcmc_group_set_stream.argtypes = [vp, vp]
    lib.tamcmc_group_synchronize.argtypes = [vp]
    lib.tamcmc_group_destroy.argtypes = [vp]
    lib.tamcmc_group_eval_begin.argtypes = [vp, ip, ip, dp, dp]
    lib.tamcmc_group_eval_end.argtypes = [vp, dp, ip]
    lib.tamcmc_group_eval_poll.argtypes = [vp, C.c_int32, C.c_int32, dp, ip]
    lib.tamcmc_group_members.argtypes = [vp, ip, ip, ip]
    lib.tamcmc_summary_create.argtypes = [C.POINTER(vp), vp, C.c_int32]
    lib.tamcmc_summary_push.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, ip]
    lib.tamcmc_summary_push_device.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp]
    lib.tamcmc_summary_result.argtypes = [vp, C.POINTER(SummaryTotals), dp, dp, dp, dp, dp, dp, dp]
    lib.tamcmc_summary_reset.argtypes = [vp]
    lib.tamcmc_summary_destroy.argtypes = [vp]
    lib.tamcmc_summary_profile.argtypes = [vp, C.c_int]
    lib.tamcmc_summary_kernel_time.argtypes = [vp, dp, C.POINTER(C.c_int64)]
    lib.tamcmc_summary_quantiles_begin.argtypes = [vp, C.c_int32, dp, C.c_int32]
    lib.tamcmc_summary_quantiles_step.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.tamcmc_summary_quantiles_result.argtypes = [vp, C.POINTER(C.c_int64), dp, dp]
    lib.tamcmc_summary_quantiles_end.argtypes = [vp]
    lib.tamcmc_summary_loo_begin.argtypes = [vp]
    lib.tamcmc_summary_loo_result.argtypes = [vp, C.POINTER(SummaryLooTotals), dp, dp, dp, ip]
    lib.tamcmc_summary_loo_end.argtypes = [vp]
    lib.tamcmc_summary_loo_pit_begin.argtypes = [vp]
    lib.tamcmc_summary_loo_pit_result.argtypes = [vp, C.POINTER(SummaryLooPitTotals), dp, dp, dp, dp, dp]
    lib.tamcmc_summary_loo_pit_kernel_time.argtypes = [vp, dp, C.POINTER(C.c_int64)]
    lib.tamcmc_summary_predictive_enable.argtypes = [vp]
    lib.tamcmc_summary_predictive_result.argtypes = [vp, C.POINTER(SummaryPredictiveTotals), dp, dp, dp, dp]
    lib.tamcmc_summary_predictive_kernel_time.argtypes = [vp, dp, C.POINTER(C.c_int64)]
    lib.tamcmc_summary_window_enable.argtypes = [vp, C.c_int32, C.c_int32, ip]
    lib.tamcmc_summary_window_result.argtypes = [vp, C.POINTER(SummaryWindowTotals), dp, dp, dp, dp]
    lib.tamcmc_summary_window_kernel_time.argtypes = [vp, dp, C.POINTER(C.c_int64)]
    lib.tamcmc_summary_wloo_begin.argtypes = [vp, C.c_int32, C.c_int32, ip]
    lib.tamcmc_summary_wloo_result.argtypes = [vp, C.POINTER(SummaryWlooTotals), dp, dp, dp, ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.tamcmc_summary_wloo_pit_begin.argtypes = [vp]
    lib.tamcmc_summary_wloo_pit_result.argtypes = [vp, C.POINTER(SummaryLooPitTotals), dp, dp, dp, dp, dp]
    lib.tamcmc_summary_wloo_pit_kernel_time.argtypes = [vp, dp, C.POINTER(C.c_int64)]
    lib.tamcmc_summary_wloo_end.argtypes = [vp]
    lib.tamcmc_summary_scan_enable.argtypes = [vp, C.c_int32, ip]
    lib.tamcmc_summary_scan_result.argtypes = [vp, C.c_int32, C.POINTER(SummaryScanTotals), dp, dp, dp, dp]
    lib.tamcmc_summary_scan_regions.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.POINTER(SummaryScanRegion), ip]
    lib.tamcmc_summary_scan_kernel_time.argtypes = [vp, dp, C.POINTER(C.c_int64)]
    lib.tamcmc_summary_ess_begin.argtypes = [vp, C.c_int32, ip]
    lib.tamcmc_summary_ess_result.argtypes = [vp, C.POINTER(SummaryEssTotals), dp, dp, dp, dp, ip, dp, dp, ip]
    lib.tamcmc_summary_ess_acov.argtypes = [vp, C.c_int32, dp]
    lib.tamcmc_summary_ess_end.argtypes = [vp]
    lib.tamcmc_summary_bandess_begin.argtypes = [vp, C.c_int32, dp, C.c_int32, ip]
    lib.tamcmc_summary_bandess_result.argtypes = [vp, C.POINTER(SummaryBandEssTotals), ip, dp, dp, dp, dp, ip]
    lib.tamcmc_summary_bandess_counts.argtypes = [vp, C.c_int32, ip, C.POINTER(C.c_int64)]
    lib.tamcmc_summary_bandess_end.argtypes = [vp]
    lp = C.POINTER(C.c_int64)
    lib.tamcmc_scan_null_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_double, C.c_int64, C.c_int32, ip, C.c_uint64, C.c_int64]
    lib.tamcmc_scan_null_run.argtypes = [vp, C.c_int64]
    lib.tamcmc_scan_null_replicates.argtypes = [vp, lp]
    lib.tamcmc_scan_null_result.argtypes = [vp, C.c_int32, C.c_int32, dp, lp, dp]
    lib.tamcmc_scan_null_line.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, C.c_int32, dp]
    lib.tamcmc_scan_null_pvalue.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, dp, dp]
    lib.tamcmc_scan_null_variates.argtypes = [vp, C.c_int64, dp]
    lib.tamcmc_scan_null_profile.argtypes = [vp, C.c_int]
    lib.tamcmc_scan_null_kernel_time.argtypes = [vp, dp, lp]
    lib.tamcmc_scan_null_destroy.argtypes = [vp]
    lib.tamcmc_modetable_create.argtypes = [C.POINTER(vp), vp, C.c_int64]
    lib.tamcmc_modetable_columns.argtypes = [vp, ip, ip]
    lib.tamcmc_modetable_column.argtypes = [vp, C.c_int32, C.POINTER(ModeTableCol)]
    lib.tamcmc_modetable_derive.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, ip]
    lib.tamcmc_modetable_push.argtypes = [vp, C.c_int32, C.c_int32, dp, ip, ip]
    lib.tamcmc_modetable_result.argtypes = [vp, C.POINTER(ModeTableTotals), dp, dp, dp, dp]
    lib.tamcmc_modetable_quantiles.argtypes = [vp, C.c_int32, dp, lp, dp]
    lib.tamcmc_modetable_reset.argtypes = [vp]
    lib.tamcmc_modetable_destroy.argtypes = [vp]
    lib.tamcmc_modetable_kernel_time.argtypes = [vp, dp, lp]
    lib.tamcmc_modediag_ess.argtypes = [vp, C.c_int32, C.POINTER(ModeDiagTotals), dp, dp, dp, dp, ip]
    lib.tamcmc_modediag_acov.argtypes = [vp, dp]
    lib.tamcmc_modediag_cov.argtypes = [vp, C.c_int32, ip, dp]
    lib.tamcmc_modediag_corr.argtypes = [vp, C.c_int32, ip, dp]
    lib.tamcmc_modediag_kernel_time.argtypes = [vp, dp, lp]
    lib.tamcmc_moderank_diag.argtypes = [vp, C.c_int32, C.c_int32, ip, C.c_int64, C.POINTER(ModeRankTotals), dp, ip]
    lib.tamcmc_moderank_acov.argtypes = [vp, C.c_int32, dp]
    lib.tamcmc_moderank_series.argtypes = [vp, C.c_int32, lp, lp, dp, dp, dp]
    lib.tamcmc_moderank_kernel_time.argtypes = [vp, dp, lp]
    lib.tamcmc_modetable_indices_enable.argtypes = [vp, C.c_int32, dp, C.POINTER(SeismicInfo)]
    lib.tamcmc_modetable_indices_info.argtypes = [vp, C.POINTER(SeismicInfo)]
    lib.tamcmc_modetable_index_terms.argtypes = [vp, C.c_int32, C.c_int32, ip, ip, ip, ip, dp, dp]
    lib.tamcmc_seismic_kernel_time.argtypes = [vp, dp, lp]
    lib.tamcmc_modepdf_hist.argtypes = [vp, C.c_int32, C.c_int32, ip, dp, dp, lp, lp, lp, dp, ip]
    lib.tamcmc_modepdf_hpd.argtypes = [vp, C.c_int32, dp, C.c_int32, ip, C.c_int64, lp, lp, dp, dp]
    lib.tamcmc_modepdf_hist2d.argtypes = [vp, C.c_int32, C.c_int32, ip, dp, dp, C.c_int32, dp, lp, lp, lp, ip]
    lib.tamcmc_modepdf_kernel_time.argtypes = [vp, dp, lp]
    lib.tamcmc_compare_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int32, C.c_int64, dp, dp, C.c_double, C.c_uint64, C.c_int64]
    lib.tamcmc_compare_info.argtypes = [vp, lp, lp]
    lib.tamcmc_compare_diff.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(CompareTotals)]
    lib.tamcmc_compare_bootstrap.argtypes = [vp, C.c_int64, C.c_int64]
    lib.tamcmc_compare_replicates.argtypes = [vp, lp]
    lib.tamcmc_compare_z.argtypes = [vp, C.c_int32, dp]
    lib.tamcmc_compare_prob.argtypes = [vp, C.c_int32, C.c_int32, lp, lp]
    lib.tamcmc_compare_interval.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, dp]
    lib.tamcmc_compare_weights.argtypes = [vp, C.c_int32, dp]
    lib.tamcmc_compare_stacking.argtypes = [vp, C.c_double, C.c_int64, C.c_int64, dp, C.POINTER(CompareStackingInfo)]
    lib.tamcmc_compare_stacking_cadence.argtypes = [vp, C.c_int32]
    lib.tamcmc_compare_variates.argtypes = [vp, C.c_int64, dp]
    lib.tamcmc_compare_profile.argtypes = [vp, C.c_int]
    lib.tamcmc_compare_kernel_time.argtypes = [vp, C.c_int32, dp, lp]
    lib.tamcmc_compare_destroy.argtypes = [vp]
    for name in EXPORTS + SEISMIC_EXPORTS + PDF_EXPORTS + COMPARE_EXPORTS:
        fn = getattr(lib, name)
        if fn.restype is not C.c_char_p:
            fn.restype = C.c_int
    _LIB = lib
    return lib


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


def _c64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


class _Handle:
    """What the classes that own one handle of the library share.  A subclass names the attribute that holds its handle (a
    C.c_void_p, set before the create call) in _HANDLE and the library's destroy function in _DESTROY; _lib is the loaded
    library.  close() keeps the handle when the library refuses to destroy it; where _DESTROY_CHECKED is False the refusal
    is not looked at."""

    _HANDLE = None
    _DESTROY = None
    _DESTROY_CHECKED = True

    def _check(self, rc, where):
        if rc != OK:
            detail = self._lib.tamcmc_strerror(rc).decode()
            if rc == E_HIP:
                detail += " | " + self._lib.tamcmc_last_hip_error().decode()
            raise AccelError(rc, where, detail)

    def close(self):
        h = getattr(self, self._HANDLE, None)
        if h is not None and h.value:
            rc = getattr(self._lib, self._DESTROY)(h)
            if self._DESTROY_CHECKED:
                self._check(rc, self._DESTROY)
            setattr(self, self._HANDLE, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _kernel_time(self, fn_name, *args):
        """(summed milliseconds, count) from the library's fn_name(handle, *args, &ms, &count)."""
        ms = C.c_double(0.0)
        n = C.c_int64(0)
        self._check(getattr(self._lib, fn_name)(getattr(self, self._HANDLE), *args, C.byref(ms), C.byref(n)), fn_name)
        return ms.value, n.value


class Accel(_Handle):
    """One context = one star (x, y[, sigma_y]) on one GPU, for one model / likelihood id."""

    def __init__(self, model_case, plength, x, y, sigma_y=None, likelihood_case=0, likelihood_p=1.0, device_id=0):
        self._lib = load_library()
        self._ctx = C.c_void_p()
        self.x = _c64(x)
        self.y = _c64(y, self.x.shape)
        sig = _c64(sigma_y, self.x.shape) if sigma_y is not None else None
        self.plength = np.ascontiguousarray(plength, dtype=np.int32)
        if self.plength.shape != (11,):
            raise ValueError("plength must have 11 entries")
        self.Nparams = int(self.plength.sum())
        self.Nx = int(self.x.size)
        self.Nvars = 0
        self.model_case = int(model_case)
        rc = self._lib.tamcmc_ctx_create(C.byref(self._ctx), int(device_id), int(model_case), int(likelihood_case),
                                         float(likelihood_p), _iptr(self.plength), self.Nx, _dptr(self.x), _dptr(self.y),
                                         _dptr(sig))
        self._check(rc, "tamcmc_ctx_create")

    # close() is refused (and the context kept) while a fit group holds it: close the Group first
    _HANDLE, _DESTROY = "_ctx", "tamcmc_ctx_destroy"

    # -- API ------------------------------------------------------------------------------------
    def set_vars(self, index_to_relax):
        idx = np.ascontiguousarray(index_to_relax, dtype=np.int32)
        self._check(self._lib.tamcmc_ctx_set_vars(self._ctx, idx.size, _iptr(idx)), "tamcmc_ctx_set_vars")
        self.Nvars = int(idx.size)

    def set_spectra(self, y, sigma_y=None):
        """Several spectra on the context's grid (rows of y); chains choose theirs with set_chain_spectrum."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.ndim != 2 or y.shape[1] != self.Nx:
            raise ValueError("y must be (Nspectra, Nx)")
        sg = None if sigma_y is None else np.ascontiguousarray(sigma_y, dtype=np.float64)
        if sg is not None and sg.shape != y.shape:
            raise ValueError("sigma_y must have the shape of y")
        self._check(self._lib.tamcmc_ctx_set_spectra(self._ctx, y.shape[0], _dptr(y), _dptr(sg)), "tamcmc_ctx_set_spectra")

    def set_chain_spectrum(self, spectrum_of_chain):
        m = np.ascontiguousarray(spectrum_of_chain, dtype=np.int32)
        self._check(self._lib.tamcmc_ctx_set_chain_spectrum(self._ctx, m.size, _iptr(m)), "tamcmc_ctx_set_chain_spectrum")

    def eval_batch(self, params, Tcoefs, grad=False, model_rows=None):
        """Returns (logL, status[, grad][, models])."""
        params = _c64(params)
        if params.ndim != 2 or params.shape[1] != self.Nparams:
            raise ValueError(f"params must be (Nchains, {self.Nparams})")
        n = params.shape[0]
        T = _c64(Tcoefs, (n,))
        logL = np.empty(n)
        status = np.empty(n, dtype=np.int32)
        g = np.empty((n, self.Nvars)) if grad else None
        rows = np.ascontiguousarray(model_rows, dtype=np.int32) if model_rows is not None else None
        models = np.empty((rows.size, self.Nx)) if rows is not None else None
        rc = self._lib.tamcmc_eval_batch(self._ctx, n, self.Nparams, _dptr(params), _dptr(T), _dptr(logL), _dptr(g),
                                         rows.size if rows is not None else 0, _iptr(rows), _dptr(models), _iptr(status))
        self._check(rc, "tamcmc_eval_batch")
        out = [logL, status]
        if grad:
            out.append(g)
        if rows is not None:
            out.append(models)
        return tuple(out)

    def reserve(self, nchains):
        self._check(self._lib.tamcmc_ctx_reserve(self._ctx, int(nchains)), "tamcmc_ctx_reserve")

    def begin(self, params, Tcoefs):
        """Likelihood evaluation of a batch, launched and not waited for (end() collects it)."""
        params = _c64(params)
        if params.ndim != 2 or params.shape[1] != self.Nparams:
            raise ValueError(f"expected (n, {self.Nparams}) params, got {params.shape}")
        T = _c64(Tcoefs, (params.shape[0],))
        self._check(self._lib.tamcmc_eval_batch_begin(self._ctx, params.shape[0], self.Nparams, _dptr(params), _dptr(T)), "tamcmc_eval_batch_begin")
        self._n_flight = params.shape[0]

    def end(self):
        n = self._n_flight
        logL = np.empty(n)
        st = np.empty(n, dtype=np.int32)
        self._check(self._lib.tamcmc_eval_batch_end(self._ctx, n, _dptr(logL), st.ctypes.data_as(C.POINTER(C.c_int32))), "tamcmc_eval_batch_end")
        return logL, st

    def poll(self, chain):
        """(logL, status) of one chain of the batch in flight, or None while it has not arrived."""
        L, st = C.c_double(), C.c_int32()
        rc = self._lib.tamcmc_eval_batch_poll(self._ctx, int(chain), C.byref(L), C.byref(st))
        if rc == -1:
            return None
        self._check(rc, "tamcmc_eval_batch_poll")
        return L.value, st.value

    def arm(self, nchains):
        """The launches of the next likelihood batch go into the stream now, behind a gate; fire() supplies the parameters."""
        self._check(self._lib.tamcmc_eval_batch_arm(self._ctx, int(nchains)), "tamcmc_eval_batch_arm")

    def fire(self, params, Tcoefs):
        params = _c64(params)
        if params.ndim != 2 or params.shape[1] != self.Nparams:
            raise ValueError(f"expected (n, {self.Nparams}) params, got {params.shape}")
        T = _c64(Tcoefs, (params.shape[0],))
        self._check(self._lib.tamcmc_eval_batch_fire(self._ctx, params.shape[0], self.Nparams, _dptr(params), _dptr(T)), "tamcmc_eval_batch_fire")
        self._n_flight = params.shape[0]

    def disarm(self):
        self._check(self._lib.tamcmc_eval_batch_disarm(self._ctx), "tamcmc_eval_batch_disarm")

    def eval_batch_device(self, nchains, d_params, d_T, d_logL, d_grad=0, d_status=0):
        """Device pointers (ints, e.g. torch.Tensor.data_ptr()); enqueued on the ctx stream, no sync."""
        rc = self._lib.tamcmc_eval_batch_device(self._ctx, int(nchains), self.Nparams, C.c_void_p(d_params),
                                                C.c_void_p(d_T), C.c_void_p(d_logL),
                                                C.c_void_p(d_grad) if d_grad else None,
                                                C.c_void_p(d_status) if d_status else None)
        self._check(rc, "tamcmc_eval_batch_device")

    def model_explicit(self, params):
        params = _c64(params, (self.Nparams,))
        out = np.empty(self.Nx)
        st = C.c_int32(0)
        self._check(self._lib.tamcmc_model_explicit(self._ctx, self.Nparams, _dptr(params), _dptr(out), C.byref(st)),
                    "tamcmc_model_explicit")
        return out, int(st.value)

    def set_stream(self, hip_stream):
        self._check(self._lib.tamcmc_ctx_set_stream(self._ctx, C.c_void_p(hip_stream) if hip_stream else None),
                    "tamcmc_ctx_set_stream")

    def synchronize(self):
        self._check(self._lib.tamcmc_ctx_synchronize(self._ctx), "tamcmc_ctx_synchronize")

    def profile(self, enable=True):
        self._check(self._lib.tamcmc_ctx_profile(self._ctx, int(enable)), "tamcmc_ctx_profile")

    def kernel_time(self):
        return self._kernel_time("tamcmc_ctx_kernel_time")

    def clock_probe_begin(self, milliseconds):
        self._check(self._lib.tamcmc_ctx_clock_probe_begin(self._ctx, float(milliseconds)), "tamcmc_ctx_clock_probe_begin")

    def clock_probe_end(self):
        """(core clock in GHz, seconds observed) of the probe started by clock_probe_begin."""
        ghz, sec = C.c_double(0.0), C.c_double(0.0)
        self._check(self._lib.tamcmc_ctx_clock_probe_end(self._ctx, C.byref(ghz), C.byref(sec)), "tamcmc_ctx_clock_probe_end")
        return ghz.value, sec.value

    def geometry(self):
        v = [C.c_int32(0) for _ in range(4)]
        self._check(self._lib.tamcmc_ctx_geometry(self._ctx, *[C.byref(e) for e in v]), "tamcmc_ctx_geometry")
        g = [C.c_int32(0) for _ in range(2)]
        self._check(self._lib.tamcmc_ctx_geometry_grad(self._ctx, *[C.byref(e) for e in g]), "tamcmc_ctx_geometry_grad")
        return dict(bins_per_tile=v[0].value, tiles=v[1].value, threads_per_block=v[2].value, n_multiplets=v[3].value,
                    tiles_grad=g[0].value, bins_per_tile_grad=g[1].value)


class Group(_Handle):
    """A fit group (tamcmc_accel.h, tamcmc_group_*): the likelihood batches of several Accel contexts -- different grids,
    model ids, layouts -- in one call.  Every chain's result equals its member's own eval_batch bit for bit.  The group
    keeps references to its members; a member cannot be closed while the group is open."""

    def __init__(self, accels):
        self._lib = load_library()
        self.members = list(accels)
        self._g = C.c_void_p()
        arr = (C.c_void_p * max(len(self.members), 1))(*[a._ctx.value for a in self.members])
        self._check(self._lib.tamcmc_group_create(C.byref(self._g), len(self.members), arr), "tamcmc_group_create")
        self.Nparams = np.array([a.Nparams for a in self.members], dtype=np.int32)

    _HANDLE, _DESTROY = "_g", "tamcmc_group_destroy"
    _DESTROY_CHECKED = False

    def _counts(self, P_list, T_list):
        if len(P_list) != len(self.members) or len(T_list) != len(self.members):
            raise ValueError(f"expected {len(self.members)} params / Tcoefs blocks")
        P = [_c64(p).reshape(-1, a.Nparams) for p, a in zip(P_list, self.members)]
        T = [_c64(t).reshape(-1) for t in T_list]
        n = np.array([p.shape[0] for p in P], dtype=np.int32)
        if any(t.size != k for t, k in zip(T, n)):
            raise ValueError("Tcoefs block sizes must match the params blocks")
        return P, T, n

    def eval(self, P_list, T_list):
        """P_list[k]: (n_k, Nparams_k) rows of member k (n_k may be 0).  Returns (list of logL, list of status)."""
        P, T, n = self._counts(P_list, T_list)
        Pc = np.ascontiguousarray(np.concatenate([p.ravel() for p in P])) if P else np.empty(0)
        Tc = np.ascontiguousarray(np.concatenate(T))
        logL = np.empty(int(n.sum()))
        st = np.empty(int(n.sum()), dtype=np.int32)
        self._check(self._lib.tamcmc_group_eval(self._g, _iptr(n), _iptr(self.Nparams), _dptr(Pc), _dptr(Tc), _dptr(logL),
                                                _iptr(st)), "tamcmc_group_eval")
        cut = np.cumsum(n)[:-1]
        return np.split(logL, cut), np.split(st, cut)

    def begin(self, P_list, T_list):
        """eval() in two halves: the batch is launched and not waited for (end() collects it, poll() looks at one chain)."""
        P, T, n = self._counts(P_list, T_list)
        Pc = np.ascontiguousarray(np.concatenate([p.ravel() for p in P])) if P else np.empty(0)
        Tc = np.ascontiguousarray(np.concatenate(T))
        self._check(self._lib.tamcmc_group_eval_begin(self._g, _iptr(n), _iptr(self.Nparams), _dptr(Pc), _dptr(Tc)),
                    "tamcmc_group_eval_begin")
        self._n_flight = n

    def end(self):
        n = getattr(self, "_n_flight", None)
        if n is None:
            n = np.zeros(len(self.members), dtype=np.int32)     # (the library refuses an _end without _begin)
        logL = np.empty(max(int(n.sum()), 1))
        st = np.empty(max(int(n.sum()), 1), dtype=np.int32)
        rc = self._lib.tamcmc_group_eval_end(self._g, _dptr(logL), _iptr(st))
        self._n_flight = None
        self._check(rc, "tamcmc_group_eval_end")
        cut = np.cumsum(n)[:-1]
        return np.split(logL[:int(n.sum())], cut), np.split(st[:int(n.sum())], cut)

    def poll(self, member, chain):
        """(logL, status) of one chain of one member of the batch in flight, or None while it has not arrived."""
        L, st = C.c_double(), C.c_int32()
        rc = self._lib.tamcmc_group_eval_poll(self._g, int(member), int(chain), C.byref(L), C.byref(st))
        if rc == -1:
            return None
        self._check(rc, "tamcmc_group_eval_poll")
        return L.value, st.value

    def eval_device(self, nchains, d_params, d_T, d_logL, d_status=0):
        """Device pointers (ints, e.g. torch.Tensor.data_ptr()) of the concatenated blocks; enqueued, no sync."""
        n = np.ascontiguousarray(nchains, dtype=np.int32).ravel()
        if n.size != len(self.members):
            raise ValueError(f"expected {len(self.members)} chain counts, got {n.size}")
        rc = self._lib.tamcmc_group_eval_device(self._g, _iptr(n), _iptr(self.Nparams), C.c_void_p(d_params), C.c_void_p(d_T),
                                                C.c_void_p(d_logL), C.c_void_p(d_status) if d_status else None)
        self._check(rc, "tamcmc_group_eval_device")

    def set_stream(self, hip_stream):
        self._check(self._lib.tamcmc_group_set_stream(self._g, C.c_void_p(hip_stream) if hip_stream else None),
                    "tamcmc_group_set_stream")

    def synchronize(self):
        self._check(self._lib.tamcmc_group_synchronize(self._g), "tamcmc_group_synchronize")


class Summary(_Handle):
    """Posterior summaries of a stored chain (tamcmc_accel.h, tamcmc_summary_*): per-bin running statistics of the model
    and of the pointwise log-likelihood over the parameter rows pushed so far, kept on the device.  Results do not depend,
    bit for bit, on block_chains or on how the rows are split over pushes.  quantiles() gives the exact per-bin quantiles
    of the model (credible bands) by pushing the same rows again a few times; loo() gives PSIS-LOO (elpd_loo and the
    Pareto k-hat per bin) by pushing them once more -- with pit=True a third time, for LOO-PIT and the PSIS weights' effective
    sample size per bin --, and ess() the effective sample size, Monte-Carlo standard error and
    split R-hat per bin by pushing them once more in the same order; band_ess() the quantiles together with the effective sample
    size of each of them (of the indicator M <= quantile), by one more pass after the selection; window_loo() PSIS-LOO and LOO-PIT with a
    whole window of bins left out, over the windows of the windowed check.  With predictive=True every fold pass also accumulates the
    posterior predictive check (predictive_result(): PIT and both log tail probabilities per bin), and with window=W or
    window=(W, first) the same check over disjoint windows of W bins (window_result()); with scan=W or scan=(W0, W1, ...) the
    windowed check at every start position for up to eight widths at once (scan_result(k), scan_regions(k)).  The Accel cannot be closed while
    the summary is open."""

    ARRAYS = ("mean_M", "var_M", "min_M", "max_M", "mean_l", "var_l", "lppd")

    def __init__(self, accel, block_chains=0, predictive=False, window=None, scan=None):
        self._lib = load_library()
        self.accel = accel
        self._s = C.c_void_p()
        self._check(self._lib.tamcmc_summary_create(C.byref(self._s), accel._ctx, int(block_chains)), "tamcmc_summary_create")
        try:
            if predictive:
                self.predictive_enable()
            if window is not None:
                self.window_enable(*np.atleast_1d(window).tolist())
            if scan is not None:
                self.scan_enable(scan)
        except (AccelError, TypeError, ValueError):
            self.close()
            raise

    _HANDLE, _DESTROY = "_s", "tamcmc_summary_destroy"

    def push(self, params):
        """params: (n, Nparams) rows.  Returns (logL, status) of these rows at T = 1."""
        params = _c64(params)
        if params.ndim != 2 or params.shape[1] != self.accel.Nparams:
            raise ValueError(f"params must be (Nsamples, {self.accel.Nparams})")
        n = params.shape[0]
        logL = np.empty(n)
        status = np.empty(n, dtype=np.int32)
        self._check(self._lib.tamcmc_summary_push(self._s, n, self.accel.Nparams, _dptr(params), _dptr(logL), _iptr(status)),
                    "tamcmc_summary_push")
        return logL, status

    def push_device(self, nsamples, d_params, d_logL=0, d_status=0):
        """Device pointers (ints, e.g. torch.Tensor.data_ptr()); enqueued on the context's stream, no sync."""
        rc = self._lib.tamcmc_summary_push_device(self._s, int(nsamples), self.accel.Nparams, C.c_void_p(d_params),
                                                  C.c_void_p(d_logL) if d_logL else None,
                                                  C.c_void_p(d_status) if d_status else None)
        self._check(rc, "tamcmc_summary_push_device")

    def result(self):
        """dict of the seven per-bin arrays and the totals n_used, n_rejected, lppd_total, p_waic, waic."""
        out = {k: np.empty(self.accel.Nx) for k in self.ARRAYS}
        t = SummaryTotals()
        self._check(self._lib.tamcmc_summary_result(self._s, C.byref(t), *[_dptr(out[k]) for k in self.ARRAYS]),
                    "tamcmc_summary_result")
        out.update(n_used=int(t.n_used), n_rejected=int(t.n_rejected), lppd_total=t.lppd_total, p_waic=t.p_waic, waic=t.waic)
        return out

    def reset(self):
        self._check(self._lib.tamcmc_summary_reset(self._s), "tamcmc_summary_reset")
        self._nq = 0                                            # reset leaves quantile mode
        self._loo = False                                       # and LOO mode
        self._ess_lag = 0                                       # and ESS mode
        self._band = None                                       # and band ESS mode
        self._wloo = 0                                          # and window-LOO mode

    def profile(self, enable=True):
        self._check(self._lib.tamcmc_summary_profile(self._s, int(enable)), "tamcmc_summary_profile")

    def kernel_time(self):
        """(summed milliseconds, launches) of the fold kernel since profile(True)."""
        return self._kernel_time("tamcmc_summary_kernel_time")

    # ---- quantiles: exact per-bin order statistics of the model over the accepted samples, a few bits per pass ----
    MAX_QUANTILES = 8

    def quantiles_begin(self, q, bits_per_pass=0):
        """Enters quantile mode for the quantiles q (1 ... 8 values in [0, 1]); bits_per_pass 1 ... 6, 0 = the library's
        default.  From here on push / push_device feed the selection: push the same rows again, then quantiles_step()."""
        q = _c64(np.atleast_1d(q))
        if q.ndim != 1:
            raise ValueError("q must be a sequence of quantiles")
        self._check(self._lib.tamcmc_summary_quantiles_begin(self._s, q.size, _dptr(q), int(bits_per_pass)),
                    "tamcmc_summary_quantiles_begin")
        self._nq = int(q.size)

    def quantiles_step(self):
        """Narrows every bracket by the pass just pushed; returns the largest number of unresolved bits (0: exact)."""
        left = C.c_int32(-1)
        self._check(self._lib.tamcmc_summary_quantiles_step(self._s, C.byref(left)), "tamcmc_summary_quantiles_step")
        return int(left.value)

    def quantiles_result(self):
        """dict: ranks (Nq), lo and hi (Nq, Nx) -- the bracket of every quantile of every bin; lo == hi where resolved."""
        nq = getattr(self, "_nq", 0) or self.MAX_QUANTILES
        ranks = np.zeros(nq, dtype=np.int64)
        lo, hi = np.empty((nq, self.accel.Nx)), np.empty((nq, self.accel.Nx))
        self._check(self._lib.tamcmc_summary_quantiles_result(self._s, ranks.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(lo), _dptr(hi)),
                    "tamcmc_summary_quantiles_result")
        return dict(ranks=ranks, lo=lo, hi=hi)

    def quantiles_end(self):
        self._check(self._lib.tamcmc_summary_quantiles_end(self._s), "tamcmc_summary_quantiles_end")
        self._nq = 0

    def quantiles(self, params, q, bits_per_pass=0, max_passes=None):
        """The quantiles q of the model over the rows already pushed, `params` being those rows: pushes them once per pass
        until every value is exact or max_passes passes are done, and always leaves quantile mode.  Returns a dict: q,
        ranks, lo, hi (Nq x Nx; equal where resolved), passes, bits_left."""
        q = _c64(np.atleast_1d(q))
        self.quantiles_begin(q, bits_per_pass)
        try:
            r = self.quantiles_result()
            passes = 0
            bits_left = 0 if np.array_equal(r["lo"].view(np.uint64), r["hi"].view(np.uint64)) else -1
            while bits_left != 0 and (max_passes is None or passes < max_passes):
                self.push(params)
                bits_left = self.quantiles_step()
                passes += 1
            if passes:
                r = self.quantiles_result()
            if bits_left < 0:                                   # max_passes = 0: not known without a step
                bits_left = None
            r.update(q=q.copy(), passes=passes, bits_left=bits_left)
            return r
        finally:
            if getattr(self, "_nq", 0):
                self.quantiles_end()

    # ---- PSIS-LOO: leave-one-out elpd and the Pareto k-hat per bin, one more pass over the same rows ----
    LOO_MAX_TAIL = 2048
    LOO_ARRAYS = ("elpd_loo", "pareto_k", "cutoff")
    LOO_TOTALS = ("n_used", "n_rejected", "elpd_loo_total", "p_loo", "looic", "k_max", "n_k_high", "n_k_inf")

    def loo_begin(self):
        """Enters LOO mode.  From here on push / push_device feed the tail kernel: push the same rows again, then
        loo_result()."""
        self._check(self._lib.tamcmc_summary_loo_begin(self._s), "tamcmc_summary_loo_begin")
        self._loo = True

    def loo_result(self):
        """dict: elpd_loo, pareto_k, cutoff (Nx doubles), tail_len (Nx int32) and the totals n_used, n_rejected,
        elpd_loo_total, p_loo, looic, k_max, n_k_high, n_k_inf."""
        out = {k: np.empty(self.accel.Nx) for k in self.LOO_ARRAYS}
        out["tail_len"] = np.empty(self.accel.Nx, dtype=np.int32)
        t = SummaryLooTotals()
        self._check(self._lib.tamcmc_summary_loo_result(self._s, C.byref(t), *[_dptr(out[k]) for k in self.LOO_ARRAYS],
                                                        _iptr(out["tail_len"])), "tamcmc_summary_loo_result")
        out.update(n_used=int(t.n_used), n_rejected=int(t.n_rejected), elpd_loo_total=t.elpd_loo, p_loo=t.p_loo, looic=t.looic,
                   k_max=t.k_max, n_k_high=int(t.n_k_high), n_k_inf=int(t.n_k_inf))
        return out

    def loo_end(self):
        self._check(self._lib.tamcmc_summary_loo_end(self._s), "tamcmc_summary_loo_end")
        self._loo = False

    def loo(self, params, pit=False):
        """PSIS-LOO over the rows already pushed, `params` being those rows: begin, one push, result, end.  Returns the
        dict of loo_result() and always leaves the mode.  pit=True: a third push for LOO-PIT, and the dict has the keys
        of loo_pit_result() as well (its n_used / n_rejected are the same numbers)."""
        self.loo_begin()
        try:
            self.push(params)
            out = self.loo_result()
            if pit:
                self.loo_pit_begin()
                self.push(params)
                out.update(self.loo_pit_result())
            return out
        finally:
            if getattr(self, "_loo", False):
                self.loo_end()

    # ---- LOO-PIT: the predictive tails under the PSIS weights, and the weights' ESS, a third pass in LOO mode ----
    LOO_PIT_ARRAYS = ("loo_pit", "loo_log_cdf", "loo_log_sf", "is_ess", "log_wsum")
    LOO_PIT_TOTALS = ("n_used", "n_rejected", "loo_ks_D", "min_loo_log_sf", "min_loo_log_cdf", "min_is_ess",
                      "bin_min_loo_log_sf", "bin_min_loo_log_cdf", "bin_min_is_ess")

    def loo_pit_begin(self):
        """In LOO mode, after a complete pass: sorts the top sets, fills the table of log weights.  From here on push /
        push_device feed the PIT kernel: push the same rows a third time, then loo_pit_result()."""
        self._check(self._lib.tamcmc_summary_loo_pit_begin(self._s), "tamcmc_summary_loo_pit_begin")

    def loo_pit_result(self):
        """dict: loo_pit, loo_log_cdf, loo_log_sf, is_ess, log_wsum (Nx doubles), loo_pit_hist (20 int64) and the totals
        n_used, n_rejected, loo_ks_D, min_loo_log_sf, min_loo_log_cdf, min_is_ess and the bins bin_min_*."""
        out = {k: np.empty(self.accel.Nx) for k in self.LOO_PIT_ARRAYS}
        t = SummaryLooPitTotals()
        self._check(self._lib.tamcmc_summary_loo_pit_result(self._s, C.byref(t), *[_dptr(out[k]) for k in self.LOO_PIT_ARRAYS]),
                    "tamcmc_summary_loo_pit_result")
        out.update(n_used=int(t.n_used), n_rejected=int(t.n_rejected), loo_ks_D=t.ks_D, min_loo_log_sf=t.min_log_sf,
                   min_loo_log_cdf=t.min_log_cdf, min_is_ess=t.min_is_ess, bin_min_loo_log_sf=int(t.bin_min_log_sf),
                   bin_min_loo_log_cdf=int(t.bin_min_log_cdf), bin_min_is_ess=int(t.bin_min_is_ess),
                   loo_pit_hist=np.array(list(t.pit_hist), dtype=np.int64))
        return out

    def loo_pit_kernel_time(self):
        """(summed milliseconds, launches) of the PIT kernel since profile(True)."""
        return self._kernel_time("tamcmc_summary_loo_pit_kernel_time")

    # ---- posterior predictive check: PIT and both log tail probabilities per bin, beside every fold pass ----
    PREDICTIVE_MAX_P = 64
    PIT_CELLS = PIT_CELLS
    PREDICTIVE_ARRAYS = ("pit", "log_cdf", "log_sf", "mean_resid")
    PREDICTIVE_TOTALS = ("n_used", "n_rejected", "ks_D", "min_log_sf", "min_log_cdf", "bin_min_log_sf", "bin_min_log_cdf")

    def predictive_enable(self):
        """Turns the check on for the life of the object; allowed only while it holds no sample and is in fold mode."""
        self._check(self._lib.tamcmc_summary_predictive_enable(self._s), "tamcmc_summary_predictive_enable")

    def predictive_result(self):
        """dict: pit, log_cdf, log_sf, mean_resid (Nx doubles), pit_hist (20 int64) and the totals n_used, n_rejected,
        ks_D, min_log_sf, min_log_cdf, bin_min_log_sf, bin_min_log_cdf."""
        out = {k: np.empty(self.accel.Nx) for k in self.PREDICTIVE_ARRAYS}
        t = SummaryPredictiveTotals()
        self._check(self._lib.tamcmc_summary_predictive_result(self._s, C.byref(t), *[_dptr(out[k]) for k in self.PREDICTIVE_ARRAYS]),
                    "tamcmc_summary_predictive_result")
        out.update(n_used=int(t.n_used), n_rejected=int(t.n_rejected), ks_D=t.ks_D, min_log_sf=t.min_log_sf, min_log_cdf=t.min_log_cdf,
                   bin_min_log_sf=int(t.bin_min_log_sf), bin_min_log_cdf=int(t.bin_min_log_cdf),
                   pit_hist=np.array(list(t.pit_hist), dtype=np.int64))
        return out

    def predictive_kernel_time(self):
        """(summed milliseconds, launches) of the predictive kernel since profile(True); kernel_time() stays the fold kernel's."""
        return self._kernel_time("tamcmc_summary_predictive_kernel_time")

    # ---- windowed predictive check: the same over disjoint windows of W bins, the first one `first` bins long ----
    WINDOW_MAX_BINS = 512
    WINDOW_MAX_SHAPE = 512
    WINDOW_ARRAYS = ("pit", "log_cdf", "log_sf", "mean_resid")
    WINDOW_TOTALS = ("n_used", "n_rejected", "n_windows", "W", "first", "ks_D", "min_log_sf", "min_log_cdf", "win_min_log_sf",
                     "win_min_log_cdf")

    def window_enable(self, W, first=0):
        """Turns the windowed check on for the life of the object (W bins per window, the first window `first` bins, 0 = W);
        allowed only while it holds no sample and is in fold mode.  Returns the number of windows."""
        nw = C.c_int32(0)
        self._check(self._lib.tamcmc_summary_window_enable(self._s, int(W), int(first), C.byref(nw)), "tamcmc_summary_window_enable")
        self._n_windows = int(nw.value)
        return self._n_windows

    def window_result(self):
        """dict: pit, log_cdf, log_sf, mean_resid (n_windows doubles), first_bin and last_bin (n_windows int64, inclusive),
        pit_hist (20 int64) and the totals n_used, n_rejected, n_windows, W, first, ks_D, min_log_sf, min_log_cdf,
        win_min_log_sf, win_min_log_cdf."""
        nw = max(getattr(self, "_n_windows", 0), 1)             # (not enabled: the library refuses before it writes)
        out = {k: np.empty(nw) for k in self.WINDOW_ARRAYS}
        t = SummaryWindowTotals()
        self._check(self._lib.tamcmc_summary_window_result(self._s, C.byref(t), *[_dptr(out[k]) for k in self.WINDOW_ARRAYS]),
                    "tamcmc_summary_window_result")
        out.update({k: (getattr(t, k) if k in ("ks_D", "min_log_sf", "min_log_cdf") else int(getattr(t, k))) for k in self.WINDOW_TOTALS})
        w = np.arange(nw, dtype=np.int64)
        out["first_bin"] = np.where(w == 0, 0, int(t.first) + (w - 1) * int(t.W))
        out["last_bin"] = np.minimum(int(t.first) + w * int(t.W), self.accel.Nx) - 1
        out["pit_hist"] = np.array(list(t.pit_hist), dtype=np.int64)
        return out

    def window_kernel_time(self):
        """(summed milliseconds, blocks) of the window kernels since profile(True); kernel_time() stays the fold kernel's."""
        return self._kernel_time("tamcmc_summary_window_kernel_time")

    # ---- window-LOO: PSIS-LOO and LOO-PIT with a window of bins left out, the windows of the windowed check ----
    WLOO_ARRAYS = ("elpd_lwo", "pareto_k", "cutoff")
    WLOO_TOTALS = ("n_used", "n_rejected", "n_windows", "W", "first", "elpd_lwo_total", "p_lwo", "k_max", "n_k_high", "n_k_inf")

    def wloo_begin(self, W, first=0):
        """Enters window-LOO mode (W bins per window, the first window `first` bins, 0 = W; window_enable is not needed).
        From here on push / push_device feed its kernels: push the same rows again, then wloo_result().  Returns the
        number of windows."""
        nw = C.c_int32(0)
        self._check(self._lib.tamcmc_summary_wloo_begin(self._s, int(W), int(first), C.byref(nw)), "tamcmc_summary_wloo_begin")
        self._wloo = int(nw.value)
        return self._wloo

    def wloo_result(self):
        """dict: elpd_lwo, pareto_k, cutoff (n_windows doubles), tail_len (int32), first_bin and last_bin (int64,
        inclusive) and the totals n_used, n_rejected, n_windows, W, first, elpd_lwo_total, p_lwo, k_max, n_k_high, n_k_inf."""
        nw = max(getattr(self, "_wloo", 0), 1)                  # (outside the mode the library refuses before it writes)
        out = {k: np.empty(nw) for k in self.WLOO_ARRAYS}
        out["tail_len"] = np.empty(nw, dtype=np.int32)
        out["first_bin"], out["last_bin"] = np.empty(nw, dtype=np.int64), np.empty(nw, dtype=np.int64)
        t = SummaryWlooTotals()
        lp = C.POINTER(C.c_int64)
        self._check(self._lib.tamcmc_summary_wloo_result(self._s, C.byref(t), *[_dptr(out[k]) for k in self.WLOO_ARRAYS],
                                                         _iptr(out["tail_len"]), out["first_bin"].ctypes.data_as(lp),
                                                         out["last_bin"].ctypes.data_as(lp)), "tamcmc_summary_wloo_result")
        out.update(n_used=int(t.n_used), n_rejected=int(t.n_rejected), n_windows=int(t.n_windows), W=int(t.W), first=int(t.first),
                   elpd_lwo_total=t.elpd_lwo, p_lwo=t.p_lwo, k_max=t.k_max, n_k_high=int(t.n_k_high), n_k_inf=int(t.n_k_inf))
        return out

    def wloo_pit_begin(self):
        """In window-LOO mode, after a complete pass: sorts the top sets, fills the table of log weights.  From here on
        push / push_device feed the sub-mode's kernels: push the same rows a third time, then wloo_pit_result()."""
        self._check(self._lib.tamcmc_summary_wloo_pit_begin(self._s), "tamcmc_summary_wloo_pit_begin")

    def wloo_pit_result(self):
        """dict with the keys of loo_pit_result(), per window: the arrays have n_windows entries and bin_min_* hold
        window indices."""
        nw = max(getattr(self, "_wloo", 0), 1)
        out = {k: np.empty(nw) for k in self.LOO_PIT_ARRAYS}
        t = SummaryLooPitTotals()
        self._check(self._lib.tamcmc_summary_wloo_pit_result(self._s, C.byref(t), *[_dptr(out[k]) for k in self.LOO_PIT_ARRAYS]),
                    "tamcmc_summary_wloo_pit_result")
        out.update(n_used=int(t.n_used), n_rejected=int(t.n_rejected), loo_ks_D=t.ks_D, min_loo_log_sf=t.min_log_sf,
                   min_loo_log_cdf=t.min_log_cdf, min_is_ess=t.min_is_ess, bin_min_loo_log_sf=int(t.bin_min_log_sf),
                   bin_min_loo_log_cdf=int(t.bin_min_log_cdf), bin_min_is_ess=int(t.bin_min_is_ess),
                   loo_pit_hist=np.array(list(t.pit_hist), dtype=np.int64))
        return out

    def wloo_pit_kernel_time(self):
        """(summed milliseconds, blocks) of the sub-mode's sums, tails and PIT kernels since profile(True)."""
        return self._kernel_time("tamcmc_summary_wloo_pit_kernel_time")

    def wloo_end(self):
        self._check(self._lib.tamcmc_summary_wloo_end(self._s), "tamcmc_summary_wloo_end")
        self._wloo = 0

    def window_loo(self, params, W, first=0, pit=False):
        """Leave-one-window-out PSIS-LOO over the rows already pushed, `params` being those rows: begin, one push, result,
        end.  Returns the dict of wloo_result() and always leaves the mode.  pit=True: a third push, and the dict has the
        keys of wloo_pit_result() as well."""
        self.wloo_begin(W, first)
        try:
            self.push(params)
            out = self.wloo_result()
            if pit:
                self.wloo_pit_begin()
                self.push(params)
                out.update(self.wloo_pit_result())
            return out
        finally:
            if getattr(self, "_wloo", 0):
                self.wloo_end()

    # ---- sliding-window predictive scan: the windowed check at every start position, several widths at once ----
    SCAN_MAX_WIDTHS = 8
    SCAN_ARRAYS = ("pit", "log_cdf", "log_sf", "mean_resid")
    SCAN_TOTALS = ("n_used", "n_rejected", "W", "n_positions", "min_log_sf", "min_log_cdf", "pos_min_log_sf", "pos_min_log_cdf")
    SCAN_REGION = ("pos_first", "pos_last", "bin_first", "bin_last", "pos_min", "min_log", "mean_resid_at_min")

    def scan_enable(self, widths):
        """Turns the scan on for the life of the object: widths is W or a strictly ascending sequence of up to eight W;
        allowed only while the object holds no sample and is in fold mode."""
        W = np.ascontiguousarray(np.atleast_1d(widths), dtype=np.int32)
        if W.ndim != 1:
            raise ValueError("widths must be an integer or a sequence of integers")
        self._check(self._lib.tamcmc_summary_scan_enable(self._s, int(W.size), _iptr(W) if W.size else None), "tamcmc_summary_scan_enable")
        self._scan_W = tuple(int(w) for w in W)

    def scan_result(self, k=0):
        """Width k of the list.  dict: pit, log_cdf, log_sf, mean_resid (n_positions doubles), first_bin and last_bin
        (n_positions int64, inclusive) and the totals n_used, n_rejected, W, n_positions, min_log_sf, min_log_cdf,
        pos_min_log_sf, pos_min_log_cdf."""
        W = getattr(self, "_scan_W", ())
        npos = max(self.accel.Nx - W[k] + 1, 1) if 0 <= k < len(W) else 1      # (otherwise the library refuses before it writes)
        out = {key: np.empty(npos) for key in self.SCAN_ARRAYS}
        t = SummaryScanTotals()
        self._check(self._lib.tamcmc_summary_scan_result(self._s, int(k), C.byref(t), *[_dptr(out[key]) for key in self.SCAN_ARRAYS]),
                    "tamcmc_summary_scan_result")
        out.update({key: (getattr(t, key) if key in ("min_log_sf", "min_log_cdf") else int(getattr(t, key))) for key in self.SCAN_TOTALS})
        out["first_bin"] = np.arange(npos, dtype=np.int64)
        out["last_bin"] = out["first_bin"] + (int(t.W) - 1)
        return out

    def scan_regions(self, k=0, which=0, log_below=None):
        """The maximal runs of positions of width k whose log_sf (which = 0: an excess) or log_cdf (which = 1: a deficit) is
        below log_below (None: log(0.01 W / Nx)), in position order: a list of dicts pos_first, pos_last, bin_first,
        bin_last, pos_min, min_log, mean_resid_at_min."""
        line = float("nan") if log_below is None else float(log_below)
        n = C.c_int32(0)
        self._check(self._lib.tamcmc_summary_scan_regions(self._s, int(k), int(which), line, 0, None, C.byref(n)), "tamcmc_summary_scan_regions")
        if n.value == 0:
            return []
        buf = (SummaryScanRegion * n.value)()
        cap = n.value
        self._check(self._lib.tamcmc_summary_scan_regions(self._s, int(k), int(which), line, cap, buf, C.byref(n)), "tamcmc_summary_scan_regions")
        return [{key: (getattr(r, key) if key in ("min_log", "mean_resid_at_min") else int(getattr(r, key))) for key in self.SCAN_REGION}
                for r in buf[:min(cap, n.value)]]

    def scan_kernel_time(self):
        """(summed milliseconds, blocks) of the scan kernels since profile(True); kernel_time() stays the fold kernel's."""
        return self._kernel_time("tamcmc_summary_scan_kernel_time")

    # ---- effective sample size, MCSE and split R-hat per bin, one more pass over the same rows in the same order ----
    ESS_MAX_LAG = 1023
    ESS_ARRAYS = ("ess_M", "tau_M", "mcse_M", "rhat_M", "cut_M", "ess_l", "r_eff", "cut_l")
    ESS_TOTALS = ("n_used", "n_rejected", "lag", "min_ess_M", "min_ess_l", "max_rhat", "bin_min_ess_M", "bin_min_ess_l",
                  "bin_max_rhat", "n_truncated_M", "n_truncated_l", "n_rhat_high")

    def ess_begin(self, max_lag=0):
        """Enters ESS mode with lags up to max_lag (0 = the library's default, 255); returns the lag limit L in use.  From
        here on push / push_device feed the ESS kernels: push the same rows again in the same order, then ess_result()."""
        lag = C.c_int32(0)
        self._check(self._lib.tamcmc_summary_ess_begin(self._s, int(max_lag), C.byref(lag)), "tamcmc_summary_ess_begin")
        self._ess_lag = int(lag.value)
        return self._ess_lag

    def ess_result(self):
        """dict: ess_M, tau_M, mcse_M, rhat_M, ess_l, r_eff (Nx doubles), cut_M, cut_l (Nx int32) and the totals n_used,
        n_rejected, lag, min_ess_M, min_ess_l, max_rhat with their bins, n_truncated_M, n_truncated_l, n_rhat_high."""
        out = {k: np.empty(self.accel.Nx, dtype=np.int32 if k.startswith("cut") else np.float64) for k in self.ESS_ARRAYS}
        t = SummaryEssTotals()
        args = [(_iptr if k.startswith("cut") else _dptr)(out[k]) for k in self.ESS_ARRAYS]
        self._check(self._lib.tamcmc_summary_ess_result(self._s, C.byref(t), *args), "tamcmc_summary_ess_result")
        kinds = dict(SummaryEssTotals._fields_)
        out.update({k: (getattr(t, k) if kinds[k] is C.c_double else int(getattr(t, k))) for k in self.ESS_TOTALS})
        return out

    def ess_acov(self, which):
        """The lag products A_0 ... A_L of a complete pass, (L + 1, Nx): which = 0 the model series, 1 the likelihood series."""
        acov = np.empty((max(getattr(self, "_ess_lag", 0), 0) + 1, self.accel.Nx))
        self._check(self._lib.tamcmc_summary_ess_acov(self._s, int(which), _dptr(acov)), "tamcmc_summary_ess_acov")
        return acov

    def ess_end(self):
        self._check(self._lib.tamcmc_summary_ess_end(self._s), "tamcmc_summary_ess_end")
        self._ess_lag = 0

    def ess(self, params, max_lag=0):
        """ESS, MCSE and split R-hat over the rows already pushed, `params` being those rows in the same order: begin, one
        push, result, end.  Returns the dict of ess_result() and always leaves the mode."""
        self.ess_begin(max_lag)
        try:
            self.push(params)
            return self.ess_result()
        finally:
            if getattr(self, "_ess_lag", 0):
                self.ess_end()

    # ---- ESS and MCSE of the credible-band edges: the indicator M <= threshold, one more pass in the same order ----
    BANDESS_ARRAYS = ("count_le", "p_hat", "ess", "tau", "mcse_p", "cut")
    BANDESS_TOTALS = ("n_used", "n_rejected", "lag", "n_thresholds", "min_ess", "bin_min_ess", "n_truncated", "n_constant")

    def bandess_begin(self, thr, max_lag=0):
        """Enters band ESS mode for the thresholds thr, (K, Nx) or (Nx,) doubles, 1 <= K <= 8, with lags up to max_lag (0 = the
        library's default, 255); returns the lag limit L in use.  From here on push / push_device feed the band kernels: push
        the same rows again in the same order, then bandess_result()."""
        thr = _c64(np.atleast_2d(thr))
        if thr.ndim != 2 or thr.shape[1] != self.accel.Nx:
            raise ValueError(f"thr must be (K, {self.accel.Nx})")
        lag = C.c_int32(0)
        self._check(self._lib.tamcmc_summary_bandess_begin(self._s, thr.shape[0], _dptr(thr), int(max_lag), C.byref(lag)),
                    "tamcmc_summary_bandess_begin")
        self._band = (int(thr.shape[0]), int(lag.value))
        return int(lag.value)

    def bandess_result(self):
        """dict: count_le, cut (K x Nx int32), p_hat, ess, tau, mcse_p (K x Nx doubles) and the totals n_used, n_rejected, lag,
        n_thresholds, and per threshold (K values each) min_ess, bin_min_ess, n_truncated, n_constant."""
        K = (getattr(self, "_band", None) or (MAX_QUANTILES, 0))[0]       # (outside the mode the library refuses before it writes)
        out = {k: np.empty((K, self.accel.Nx), dtype=np.int32 if k in ("count_le", "cut") else np.float64) for k in self.BANDESS_ARRAYS}
        t = SummaryBandEssTotals()
        args = [(_iptr if k in ("count_le", "cut") else _dptr)(out[k]) for k in self.BANDESS_ARRAYS]
        self._check(self._lib.tamcmc_summary_bandess_result(self._s, C.byref(t), *args), "tamcmc_summary_bandess_result")
        out.update(n_used=int(t.n_used), n_rejected=int(t.n_rejected), lag=int(t.lag), n_thresholds=int(t.n_thresholds),
                   min_ess=np.array(list(t.min_ess)[:K]), bin_min_ess=np.array(list(t.bin_min_ess)[:K], dtype=np.int64),
                   n_truncated=np.array(list(t.n_truncated)[:K], dtype=np.int64), n_constant=np.array(list(t.n_constant)[:K], dtype=np.int64))
        return out

    def bandess_counts(self, j):
        """(C, E) of threshold j after a complete pass: the lag counts C_k (int32) and the centred lag products times n^2, E_k
        (int64), each (L + 1, Nx)."""
        L = (getattr(self, "_band", None) or (0, 0))[1]
        Ck = np.empty((L + 1, self.accel.Nx), dtype=np.int32)
        Ek = np.empty((L + 1, self.accel.Nx), dtype=np.int64)
        self._check(self._lib.tamcmc_summary_bandess_counts(self._s, int(j), _iptr(Ck), Ek.ctypes.data_as(C.POINTER(C.c_int64))),
                    "tamcmc_summary_bandess_counts")
        return Ck, Ek

    def bandess_end(self):
        self._check(self._lib.tamcmc_summary_bandess_end(self._s), "tamcmc_summary_bandess_end")
        self._band = None

    def band_ess(self, params, q, max_lag=0, bits_per_pass=0):
        """The exact quantiles q of the model over the rows already pushed (`params` being those rows in the same order) and
        how well each is determined: quantiles() to exactness, then one band ESS pass at the values found.  Returns the
        dicts of quantiles() and bandess_result() merged, plus tail_ess (Nx): per bin the smaller of the ESS at the lowest and
        at the highest of q, NaN if either is.  Always leaves the mode."""
        r = self.quantiles(params, q, bits_per_pass)
        self.bandess_begin(r["lo"], max_lag)
        try:
            self.push(params)
            r.update(self.bandess_result())
        finally:
            if getattr(self, "_band", None):
                self.bandess_end()
        lo, hi = int(np.argmin(r["q"])), int(np.argmax(r["q"]))
        r["tail_ess"] = np.minimum(r["ess"][lo], r["ess"][hi])              # (np.minimum propagates NaN)
        return r


class ScanNull(_Handle):
    """Monte-Carlo null of the sliding-window scan (tamcmc_accel.h, tamcmc_scan_null_*): the law of the scan's extremes over
    every position of every width under a correctly specified model, simulated on the device, and the lines and p-values
    counted off it.  Bound to a device and to no Accel or chain: it depends on (likelihood_case, p, Nx, widths) alone.
    run(n) appends n replicates; line() is what Summary.scan_regions takes as log_below.  Replicate r of the object is global
    replicate first_replicate + r and does not depend on how the replicates are split over runs or objects."""

    MAX_REPLICATES = 1 << 24      # TAMCMC_SCAN_NULL_MAX_REPLICATES

    def __init__(self, likelihood_case, p, Nx, widths, seed, first_replicate=0, device_id=0):
        self._lib = load_library()
        self._h = C.c_void_p()
        W = np.ascontiguousarray(np.atleast_1d(widths), dtype=np.int32)
        if W.ndim != 1:
            raise ValueError("widths must be an integer or a sequence of integers")
        self.Nx = int(Nx)
        self.widths = tuple(int(w) for w in W)
        self._check(self._lib.tamcmc_scan_null_create(C.byref(self._h), int(device_id), int(likelihood_case), float(p), self.Nx, int(W.size),
                                                      _iptr(W) if W.size else None, int(seed), int(first_replicate)), "tamcmc_scan_null_create")

    _HANDLE, _DESTROY = "_h", "tamcmc_scan_null_destroy"

    def run(self, n):
        """Appends n replicates (synchronous); returns the number of replicates done."""
        self._check(self._lib.tamcmc_scan_null_run(self._h, int(n)), "tamcmc_scan_null_run")
        return self.replicates

    @property
    def replicates(self):
        R = C.c_int64(0)
        self._check(self._lib.tamcmc_scan_null_replicates(self._h, C.byref(R)), "tamcmc_scan_null_replicates")
        return int(R.value)

    def result(self, k, which):
        """Width k, side which (0: the maximum sum / excess, 1: the minimum sum / deficit): dict of ext_sum, pos (int64) and
        min_log, one entry per replicate."""
        R = self.replicates
        out = dict(ext_sum=np.empty(R), pos=np.empty(R, dtype=np.int64), min_log=np.empty(R))
        self._check(self._lib.tamcmc_scan_null_result(self._h, int(k), int(which), _dptr(out["ext_sum"]),
                                                      out["pos"].ctypes.data_as(C.POINTER(C.c_int64)), _dptr(out["min_log"])),
                    "tamcmc_scan_null_result")
        return out

    def line(self, k, which=0, alpha=0.01, joint=True):
        """The line at level alpha for width k: jointly over all widths and positions, or over the positions of this width."""
        v = C.c_double(0.0)
        self._check(self._lib.tamcmc_scan_null_line(self._h, int(k), int(which), float(alpha), int(bool(joint)), C.byref(v)),
                    "tamcmc_scan_null_line")
        return v.value

    def pvalue(self, k, which, value):
        """(p_width, p_joint) of a scan value (a log_sf for which = 0, a log_cdf for which = 1) of width k."""
        pw, pj = C.c_double(0.0), C.c_double(0.0)
        self._check(self._lib.tamcmc_scan_null_pvalue(self._h, int(k), int(which), float(value), C.byref(pw), C.byref(pj)),
                    "tamcmc_scan_null_pvalue")
        return pw.value, pj.value

    def variates(self, r):
        """The Nx variates of replicate r, generated on the device."""
        q = np.empty(self.Nx)
        self._check(self._lib.tamcmc_scan_null_variates(self._h, int(r), _dptr(q)), "tamcmc_scan_null_variates")
        return q

    def profile(self, enable=True):
        self._check(self._lib.tamcmc_scan_null_profile(self._h, int(enable)), "tamcmc_scan_null_profile")

    def kernel_time(self):
        """(summed milliseconds, chunks) of the kernels since profile(True)."""
        return self._kernel_time("tamcmc_scan_null_kernel_time")


class Compare(_Handle):
    """Comparison of K fits of one spectrum from their pointwise log predictive values (tamcmc_accel_compare.h,
    tamcmc_compare_*): elpd differences with their standard error, a Bayesian bootstrap of the differences on the device,
    pseudo-BMA, pseudo-BMA+ and stacking weights.  elpd is (K, N): row k the elpd_loo (or elpd_lwo, or lppd - var_l) of fit k
    per unit; pareto_k likewise or None; scale 1 for chi(2,2p), 0.5 for chi_square.  Units where any fit is not finite are
    excluded.  Fit 0 is the reference fit of the bootstrap.  Bound to a device and to no Accel or chain."""

    MAX_FITS = COMPARE_MAX_FITS
    MAX_REPLICATES = COMPARE_MAX_REPLICATES
    TILE = COMPARE_TILE
    STACK_TILE = COMPARE_STACK_TILE
    TOTALS = ("n_included", "n_excluded", "n_better", "n_worse", "n_k_high", "elpd_diff", "se_diff", "diff_k_high")

    def __init__(self, elpd, pareto_k=None, scale=1.0, seed=0, first_replicate=0, device_id=0):
        self._lib = load_library()
        self._h = C.c_void_p()
        e = np.ascontiguousarray(elpd, dtype=np.float64)
        if e.ndim != 2:
            raise ValueError("elpd must be (K, N)")
        kh = _c64(pareto_k, e.shape) if pareto_k is not None else None
        self.K, self.N = int(e.shape[0]), int(e.shape[1])
        self.scale = float(scale)
        self._check(self._lib.tamcmc_compare_create(C.byref(self._h), int(device_id), self.K, self.N, _dptr(e), _dptr(kh), self.scale,
                                                    int(seed), int(first_replicate)), "tamcmc_compare_create")
        inc, exc = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.tamcmc_compare_info(self._h, C.byref(inc), C.byref(exc)), "tamcmc_compare_info")
        self.n_included, self.n_excluded = int(inc.value), int(exc.value)

    _HANDLE, _DESTROY = "_h", "tamcmc_compare_destroy"

    @classmethod
    def from_loo(cls, *results, **kw):
        """From what Summary.loo (keys elpd_loo, pareto_k) or Summary.window_loo (elpd_lwo, pareto_k) returned, one dict per
        fit, all of one kind and one length."""
        key = "elpd_loo" if all("elpd_loo" in r for r in results) else "elpd_lwo"
        elpd = np.stack([np.asarray(r[key], dtype=np.float64) for r in results])
        kh = np.stack([np.asarray(r["pareto_k"], dtype=np.float64) for r in results]) if all("pareto_k" in r for r in results) else None
        return cls(elpd, kh, **kw)

    def diff(self, a, b):
        """dict of the pair (a, b): d_i = elpd[a][i] - elpd[b][i]; elpd_diff, se_diff, n_better, n_worse, n_k_high,
        diff_k_high, n_included, n_excluded."""
        t = CompareTotals()
        self._check(self._lib.tamcmc_compare_diff(self._h, int(a), int(b), C.byref(t)), "tamcmc_compare_diff")
        return {k: (int(getattr(t, k)) if k.startswith("n_") else float(getattr(t, k))) for k in self.TOTALS}

    def bootstrap(self, R, scratch_bytes=0):
        """Appends R replicates of the Bayesian bootstrap (synchronous); returns the number of replicates done."""
        self._check(self._lib.tamcmc_compare_bootstrap(self._h, int(R), int(scratch_bytes)), "tamcmc_compare_bootstrap")
        return self.replicates

    @property
    def replicates(self):
        R = C.c_int64(0)
        self._check(self._lib.tamcmc_compare_replicates(self._h, C.byref(R)), "tamcmc_compare_replicates")
        return int(R.value)

    def z(self, k):
        """z_rk of fit k over the replicates done (zeros for k = 0)."""
        out = np.empty(self.replicates)
        self._check(self._lib.tamcmc_compare_z(self._h, int(k), _dptr(out)), "tamcmc_compare_z")
        return out

    def prob(self, a, b):
        """(n_greater, n_equal, R): the counts of z_a > z_b and z_a == z_b over the R replicates."""
        gt, eq = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.tamcmc_compare_prob(self._h, int(a), int(b), C.byref(gt), C.byref(eq)), "tamcmc_compare_prob")
        return int(gt.value), int(eq.value), self.replicates

    def interval(self, a, b, q):
        """The order statistic of z_a - z_b at rank ceil(q R) - 1."""
        v = C.c_double(0.0)
        self._check(self._lib.tamcmc_compare_interval(self._h, int(a), int(b), float(q), C.byref(v)), "tamcmc_compare_interval")
        return v.value

    def weights(self, method="pseudo_bma_plus"):
        """K weights: "pseudo_bma", "pseudo_bma_plus" (after bootstrap) or "stacking" (what the last stacking() returned)."""
        w = np.empty(self.K)
        self._check(self._lib.tamcmc_compare_weights(self._h, COMPARE_METHODS[method] if isinstance(method, str) else int(method), _dptr(w)),
                    "tamcmc_compare_weights")
        return w

    def stacking(self, tol=1e-8, max_iter=100000, scratch_bytes=0, cadence=None):
        """Stacking weights by the EM fixed point: dict of w, iterations, converged, gap, f, table.  cadence (iterations
        between two looks of the host at the device's state) changes no bit of it."""
        if cadence is not None:
            self._check(self._lib.tamcmc_compare_stacking_cadence(self._h, int(cadence)), "tamcmc_compare_stacking_cadence")
        w = np.empty(self.K)
        info = CompareStackingInfo()
        self._check(self._lib.tamcmc_compare_stacking(self._h, float(tol), int(max_iter), int(scratch_bytes), _dptr(w), C.byref(info)),
                    "tamcmc_compare_stacking")
        return dict(w=w, iterations=int(info.iterations), converged=int(info.converged), gap=info.gap, f=info.f, table=int(info.table))

    def variates(self, r):
        """The N variates of replicate r, generated on the device."""
        e = np.empty(self.N)
        self._check(self._lib.tamcmc_compare_variates(self._h, int(r), _dptr(e)), "tamcmc_compare_variates")
        return e

    def profile(self, enable=True):
        self._check(self._lib.tamcmc_compare_profile(self._h, int(enable)), "tamcmc_compare_profile")

    def kernel_time(self, which=0):
        """(summed milliseconds, launches) since profile(True): which = 0 the bootstrap's chunks, 1 the stacking's launches."""
        return self._kernel_time("tamcmc_compare_kernel_time", int(which))


class ModeTable(_Handle):
    """The posterior mode table (tamcmc_accel.h, tamcmc_modetable_*): per params row the derived quantities of every
    multiplet and of the chain -- frequency, width, height, amplitude, splitting, truncation window, component frequencies
    and heights; inclination, eta, a3, asymmetry -- produced on the device by the derivation the kernels use, and their
    statistics over the rows pushed: count, mean, sd, min, max, and with max_samples > 0 (rows of the table kept on the
    device) exact quantiles.  No result bit depends on how the rows are split over pushes.  The Accel cannot be closed
    while the table is open."""

    KINDS = MODETABLE_KINDS + SEISMIC_KINDS
    ARRAYS = ("mean", "sd", "min", "max")
    COL_DTYPE = np.dtype([("kind", np.int32), ("mult", np.int32), ("order", np.int32), ("l", np.int32), ("m", np.int32),
                          ("param_index", np.int32)])

    def __init__(self, accel, max_samples=0):
        self._lib = load_library()
        self.accel = accel
        self._mt = C.c_void_p()
        self._check(self._lib.tamcmc_modetable_create(C.byref(self._mt), accel._ctx, int(max_samples)), "tamcmc_modetable_create")
        nc, nm = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.tamcmc_modetable_columns(self._mt, C.byref(nc), C.byref(nm)), "tamcmc_modetable_columns")
        self.n_cols, self.n_mult = int(nc.value), int(nm.value)
        self.max_samples = int(max_samples)

    _HANDLE, _DESTROY = "_mt", "tamcmc_modetable_destroy"

    def columns(self):
        """Structured array (kind, mult, order, l, m, param_index) of the n_cols columns; KINDS[kind] is the kind's name."""
        out = np.zeros(self.n_cols, dtype=self.COL_DTYPE)
        c = ModeTableCol()
        for k in range(self.n_cols):
            self._check(self._lib.tamcmc_modetable_column(self._mt, k, C.byref(c)), "tamcmc_modetable_column")
            out[k] = (c.kind, c.mult, c.order, c.l, c.m, c.param_index)
        return out

    def _params(self, params):
        params = _c64(params)
        if params.ndim != 2 or params.shape[1] != self.accel.Nparams:
            raise ValueError(f"params must be (Nsamples, {self.accel.Nparams})")
        return params

    def derive(self, params):
        """The plain map: (rows (n, n_cols), status (n)) of the params rows; nothing is accumulated."""
        params = self._params(params)
        n = params.shape[0]
        rows = np.empty((n, self.n_cols))
        status = np.empty(n, dtype=np.int32)
        self._check(self._lib.tamcmc_modetable_derive(self._mt, n, self.accel.Nparams, _dptr(params), _dptr(rows), _iptr(status)),
                    "tamcmc_modetable_derive")
        return rows, status

    def push(self, params, skip=None):
        """Derives the rows and folds the accepted ones (status 0, skip entry 0) into the statistics and the table.  Returns
        the status codes."""
        params = self._params(params)
        n = params.shape[0]
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(skip, dtype=np.int32)
            if sk.shape != (n,):
                raise ValueError(f"skip must have {n} entries")
        status = np.empty(n, dtype=np.int32)
        self._check(self._lib.tamcmc_modetable_push(self._mt, n, self.accel.Nparams, _dptr(params), _iptr(sk), _iptr(status)),
                    "tamcmc_modetable_push")
        return status

    def result(self):
        """dict: mean, sd, min, max (n_cols doubles) and the totals n_used, n_rejected, n_cols, n_mult."""
        out = {k: np.empty(self.n_cols) for k in self.ARRAYS}
        t = ModeTableTotals()
        self._check(self._lib.tamcmc_modetable_result(self._mt, C.byref(t), *[_dptr(out[k]) for k in self.ARRAYS]),
                    "tamcmc_modetable_result")
        out.update(n_used=int(t.n_used), n_rejected=int(t.n_rejected), n_cols=int(t.n_cols), n_mult=int(t.n_mult))
        return out

    def quantiles(self, q):
        """dict: q, ranks (Nq int64) and values (Nq, n_cols): the exact order statistics of every column over the accepted
        rows, by numpy's inverted_cdf rule."""
        q = _c64(np.atleast_1d(q))
        if q.ndim != 1:
            raise ValueError("q must be a sequence of probabilities")
        ranks = np.zeros(max(q.size, 1), dtype=np.int64)
        values = np.empty((max(q.size, 1), self.n_cols))
        self._check(self._lib.tamcmc_modetable_quantiles(self._mt, q.size, _dptr(q), ranks.ctypes.data_as(C.POINTER(C.c_int64)),
                                                         _dptr(values)), "tamcmc_modetable_quantiles")
        return dict(q=q.copy(), ranks=ranks[:q.size], values=values[:q.size])

    def reset(self):
        self._check(self._lib.tamcmc_modetable_reset(self._mt), "tamcmc_modetable_reset")

    def kernel_time(self):
        """(summed milliseconds, launches) of the derive and fold kernels since the object was created or reset."""
        return self._kernel_time("tamcmc_modetable_kernel_time")

    def enable_indices(self, ref_params):
        """Appends the seismic indices (tamcmc_modetable_indices_enable) as further columns: the plan is fixed from the
        params row ref_params.  Allowed once, on a table that has taken no sample.  Returns the info dict: n_base_cols,
        n_index_cols, n_radial, n_unassigned, n_base, dnu_ref, eps_ref; n_cols and columns() then cover all columns."""
        ref = _c64(ref_params)
        if ref.shape != (self.accel.Nparams,):
            raise ValueError(f"ref_params must have {self.accel.Nparams} entries")
        info = SeismicInfo()
        self._check(self._lib.tamcmc_modetable_indices_enable(self._mt, self.accel.Nparams, _dptr(ref), C.byref(info)),
                    "tamcmc_modetable_indices_enable")
        self.n_cols = int(info.n_base_cols + info.n_index_cols)
        return {k: (float if k.endswith("_ref") else int)(getattr(info, k)) for k, _ in SeismicInfo._fields_}

    def indices_info(self):
        """The info dict of enable_indices() again."""
        info = SeismicInfo()
        self._check(self._lib.tamcmc_modetable_indices_info(self._mt, C.byref(info)), "tamcmc_modetable_indices_info")
        return {k: (float if k.endswith("_ref") else int)(getattr(info, k)) for k, _ in SeismicInfo._fields_}

    def index_terms(self, col):
        """What index column col is: dict of n_num, n_den, src, wsrc (int32), coef (n_num + n_den entries each, the terms of
        num first) and offset; value = num / den - offset (tamcmc_accel_seismic.h)."""
        nn, nd = C.c_int32(0), C.c_int32(0)
        rc = self._lib.tamcmc_modetable_index_terms(self._mt, int(col), 0, C.byref(nn), C.byref(nd), None, None, None, None)
        if rc != E_INVALID or nn.value + nd.value < 1:
            self._check(rc if rc != OK else E_INVALID, "tamcmc_modetable_index_terms")
        n = nn.value + nd.value
        src, wsrc, coef = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty(n)
        off = C.c_double(0.0)
        self._check(self._lib.tamcmc_modetable_index_terms(self._mt, int(col), n, C.byref(nn), C.byref(nd), _iptr(src), _iptr(wsrc),
                                                           _dptr(coef), C.byref(off)), "tamcmc_modetable_index_terms")
        return dict(n_num=int(nn.value), n_den=int(nd.value), src=src, wsrc=wsrc, coef=coef, offset=float(off.value))

    def seismic_kernel_time(self):
        """(summed milliseconds, launches) of the indices kernel since the object was created or reset."""
        return self._kernel_time("tamcmc_seismic_kernel_time")

    DIAG_ARRAYS = ("ess", "tau", "mcse", "rhat")

    def ess(self, max_lag=0):
        """dict: ess, tau, mcse, rhat (n_cols doubles) and cut (n_cols int32) of every column over the accepted rows in the
        table (max_samples > 0, at least 4 rows), from the autocorrelation up to lag max_lag (0 ... 1023, 0: 255), and the
        totals n_used, lag, min_ess, col_min_ess, max_rhat, col_max_rhat, n_truncated, n_constant, n_rhat_high."""
        out = {k: np.empty(self.n_cols) for k in self.DIAG_ARRAYS}
        out["cut"] = np.empty(self.n_cols, dtype=np.int32)
        t = ModeDiagTotals()
        self._check(self._lib.tamcmc_modediag_ess(self._mt, int(max_lag), C.byref(t), *[_dptr(out[k]) for k in self.DIAG_ARRAYS],
                                                  _iptr(out["cut"])), "tamcmc_modediag_ess")
        out.update(n_used=int(t.n_used), lag=int(t.lag), min_ess=float(t.min_ess), col_min_ess=int(t.col_min_ess),
                   max_rhat=float(t.max_rhat), col_max_rhat=int(t.col_max_rhat), n_truncated=int(t.n_truncated),
                   n_constant=int(t.n_constant), n_rhat_high=int(t.n_rhat_high))
        self._diag_lag = int(t.lag)
        return out

    def acov(self):
        """(L + 1, n_cols): the lag products A_k of the last ess() call (refused after a push or a reset)."""
        out = np.empty((getattr(self, "_diag_lag", 0) + 1, self.n_cols))
        self._check(self._lib.tamcmc_modediag_acov(self._mt, _dptr(out)), "tamcmc_modediag_acov")
        return out

    def _selection(self, cols):
        """(n_sel, the columns as the library takes them -- None: the first n_sel --, the columns as a result names them)"""
        if cols is None:
            return self.n_cols, None, np.arange(self.n_cols, dtype=np.int32)
        sel = np.ascontiguousarray(cols, dtype=np.int32)
        if sel.ndim != 1:
            raise ValueError("cols must be a sequence of column indices")
        return sel.size, sel, sel.copy()

    def _between(self, fn, name, cols):
        n_sel, sel, _ = self._selection(cols)       # (None and more than 1024 columns: the library refuses)
        out = np.empty((max(n_sel, 1), max(n_sel, 1)))
        self._check(fn(self._mt, n_sel, _iptr(sel), _dptr(out)), name)
        return out

    def cov(self, cols=None):
        """(n_sel, n_sel) covariances (n - 1) of the columns `cols`, in that order; None: all columns (at most 1024)."""
        return self._between(self._lib.tamcmc_modediag_cov, "tamcmc_modediag_cov", cols)

    def corr(self, cols=None):
        """(n_sel, n_sel) correlations of the columns `cols`; NaN where a column is constant, 1.0 on the diagonal."""
        return self._between(self._lib.tamcmc_modediag_corr, "tamcmc_modediag_corr", cols)

    def diag_kernel_time(self):
        """(summed milliseconds, launches) of the lag, finish and covariance kernels since the object was created or reset."""
        return self._kernel_time("tamcmc_modediag_kernel_time")

    def rank_diag(self, max_lag=0, cols=None, scratch_bytes=0):
        """Rank-normalised diagnostics (tamcmc_moderank_diag) of the columns `cols`, in that order (None: all): dict of
        ess_bulk, ess_tail, rhat, tau_bulk, rhat_bulk, rhat_fold, ess_q05, ess_q95 (n_sel doubles each), cut (4, n_sel) of
        the series z, zfold, i05, i95, cols, and the totals n_used, lag, min_ess_bulk, col_min_ess_bulk, min_ess_tail,
        col_min_ess_tail, max_rhat, col_max_rhat, n_truncated, n_constant, n_rhat_high.  The columns are processed in
        chunks that fit scratch_bytes of device memory (0: 256 MiB); no result bit depends on it."""
        n_sel, sel, cols_out = self._selection(cols)
        arr = np.empty((MODERANK_NOUT, max(n_sel, 1)))
        cut = np.empty((MODERANK_NSERIES, max(n_sel, 1)), dtype=np.int32)
        t = ModeRankTotals()
        self._check(self._lib.tamcmc_moderank_diag(self._mt, int(max_lag), n_sel, _iptr(sel), int(scratch_bytes), C.byref(t),
                                                   _dptr(arr), _iptr(cut)), "tamcmc_moderank_diag")
        out = {k: arr[i].copy() for i, k in enumerate(MODERANK_OUT)}
        out["cut"] = cut
        out["cols"] = cols_out
        out.update({k: (float if k.startswith(("min_", "max_")) else int)(getattr(t, k)) for k, _ in ModeRankTotals._fields_})
        self._rank_lag, self._rank_nsel = int(t.lag), n_sel
        return out

    def rank_acov(self, series):
        """(L + 1, n_sel): the lag products of series `series` (0 ... 3 or "z", "zfold", "i05", "i95") of the last rank_diag()
        call (refused after a push or a reset)."""
        s = MODERANK_SERIES.index(series) if isinstance(series, str) else int(series)
        out = np.empty((getattr(self, "_rank_lag", 0) + 1, getattr(self, "_rank_nsel", 1)))
        self._check(self._lib.tamcmc_moderank_acov(self._mt, s, _dptr(out)), "tamcmc_moderank_acov")
        return out

    def rank_series(self, col):
        """One column recomputed by the rank kernels: dict of rank2, rank2_fold (n int64), series (4, n), mean (4) and
        med, q05, q95."""
        n = self.result()["n_used"]
        r2, r2f = np.empty(max(n, 1), dtype=np.int64), np.empty(max(n, 1), dtype=np.int64)
        series, mean, mq = np.empty((MODERANK_NSERIES, max(n, 1))), np.empty(MODERANK_NSERIES), np.empty(3)
        l64 = C.POINTER(C.c_int64)
        self._check(self._lib.tamcmc_moderank_series(self._mt, int(col), r2.ctypes.data_as(l64), r2f.ctypes.data_as(l64), _dptr(series),
                                                     _dptr(mean), _dptr(mq)), "tamcmc_moderank_series")
        return dict(rank2=r2, rank2_fold=r2f, series=series, mean=mean, med=float(mq[0]), q05=float(mq[1]), q95=float(mq[2]))

    def rank_kernel_time(self):
        """(summed milliseconds, launches) of the rank diagnostics' kernels since the object was created or reset."""
        return self._kernel_time("tamcmc_moderank_kernel_time")

    @staticmethod
    def _range(lo, hi, m):
        """(lo, hi) as m doubles each, or (None, None)"""
        if lo is None and hi is None:
            return None, None
        if lo is None or hi is None:
            raise ValueError("lo and hi go together")
        lo, hi = _c64(np.ravel(lo)), _c64(np.ravel(hi))
        if lo.size != m or hi.size != m:
            raise ValueError(f"lo and hi must have {m} entries each")
        return lo, hi

    def hist(self, bins, cols=None, lo=None, hi=None):
        """Marginal histograms (tamcmc_modepdf_hist) of the columns `cols`, in that order (None: all), in `bins` uniform
        classes over lo ... hi (n_sel doubles each; None: the column's min and max): dict of counts (n_sel, bins), below,
        above (n_sel) int64, range (n_sel, 2), status (n_sel int32; 1: a default range that is not finite, every count 0)
        and cols.  The class rule is that of tamcmc_accel_pdf.h; hist_edges() gives the edges for a plot."""
        n_sel, sel, cols_out = self._selection(cols)
        m, nb = max(n_sel, 1), max(int(bins), 1)
        lo, hi = self._range(lo, hi, n_sel)
        counts = np.zeros((m, nb), dtype=np.int64)
        below, above = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
        rng, status = np.zeros((m, 2)), np.zeros(m, dtype=np.int32)
        l64 = C.POINTER(C.c_int64)
        self._check(self._lib.tamcmc_modepdf_hist(self._mt, int(bins), n_sel, _iptr(sel), _dptr(lo), _dptr(hi), counts.ctypes.data_as(l64),
                                                  below.ctypes.data_as(l64), above.ctypes.data_as(l64), _dptr(rng), _iptr(status)),
                    "tamcmc_modepdf_hist")
        return dict(counts=counts, below=below, above=above, range=rng, status=status, cols=cols_out)

    @staticmethod
    def hist_edges(range, bins):
        """The bins + 1 plot edges lo + (hi - lo) * (b / bins) of one range (lo, hi), the last one hi exactly.  For plots:
        the counts follow the class rule, not these edges."""
        lo, hi = (float(v) for v in range)
        e = np.float64(lo) + (np.float64(hi) - np.float64(lo)) * (np.arange(bins + 1, dtype=np.float64) / np.float64(bins))
        e[bins] = hi
        return e

    def hpd(self, mass, cols=None, scratch_bytes=0):
        """Shortest intervals (tamcmc_modepdf_hpd) holding each of `mass` (in (0, 1]) of the columns `cols`: dict of mass,
        k (n_mass int64: the window lengths), start (n_mass, n_sel) int64, lo, hi (n_mass, n_sel) and cols.  The columns are
        sorted in chunks that fit scratch_bytes of device memory (0: 256 MiB); no result bit depends on it."""
        mass = _c64(np.atleast_1d(mass))
        if mass.ndim != 1:
            raise ValueError("mass must be a sequence of probabilities")
        n_sel, sel, cols_out = self._selection(cols)
        nm, m = max(mass.size, 1), max(n_sel, 1)
        k, start = np.zeros(nm, dtype=np.int64), np.zeros((nm, m), dtype=np.int64)
        lo, hi = np.zeros((nm, m)), np.zeros((nm, m))
        l64 = C.POINTER(C.c_int64)
        self._check(self._lib.tamcmc_modepdf_hpd(self._mt, mass.size, _dptr(mass), n_sel, _iptr(sel), int(scratch_bytes), k.ctypes.data_as(l64),
                                                 start.ctypes.data_as(l64), _dptr(lo), _dptr(hi)), "tamcmc_modepdf_hpd")
        return dict(mass=mass.copy(), k=k[:mass.size], start=start[:mass.size], lo=lo[:mass.size], hi=hi[:mass.size], cols=cols_out)

    def hist2d(self, pairs, bins, lo=None, hi=None, mass=()):
        """Pair densities (tamcmc_modepdf_hist2d) of the column pairs `pairs` (n_pairs, 2) in bins x bins classes over
        lo ... hi ((n_pairs, 2) each; None: the columns' min and max): dict of counts (n_pairs, bins, bins) int64, the first
        axis the pair's first column, outside (n_pairs), level (n_mass, n_pairs) int64 -- the contour levels of `mass` -- and
        status (n_pairs)."""
        pr = np.ascontiguousarray(pairs, dtype=np.int32)
        if pr.ndim != 2 or pr.shape[1] != 2:
            raise ValueError("pairs must be (n_pairs, 2) column indices")
        n_pairs = pr.shape[0]
        mass = _c64(np.atleast_1d(mass)) if np.size(mass) else np.zeros(0)
        lo, hi = self._range(lo, hi, 2 * n_pairs)
        m, nb = max(n_pairs, 1), max(int(bins), 1)
        counts = np.zeros((m, nb, nb), dtype=np.int64)
        outside, level = np.zeros(m, dtype=np.int64), np.zeros((max(mass.size, 1), m), dtype=np.int64)
        status = np.zeros(m, dtype=np.int32)
        l64 = C.POINTER(C.c_int64)
        self._check(self._lib.tamcmc_modepdf_hist2d(self._mt, int(bins), n_pairs, _iptr(pr), _dptr(lo), _dptr(hi), mass.size,
                                                    _dptr(mass) if mass.size else None, counts.ctypes.data_as(l64), outside.ctypes.data_as(l64),
                                                    level.ctypes.data_as(l64) if mass.size else None, _iptr(status)), "tamcmc_modepdf_hist2d")
        return dict(counts=counts, outside=outside, level=level[:mass.size], status=status, pairs=pr.copy())

    def pdf_kernel_time(self):
        """(summed milliseconds, launches) of the histogram, pair and HPD kernels, hpd's sort launches included, since the
        object was created or reset."""
        return self._kernel_time("tamcmc_modepdf_kernel_time")


def device_count():
    return int(load_library().tamcmc_device_count())


def version():
    return load_library().tamcmc_version().decode()
