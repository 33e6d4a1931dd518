"""ctypes binding of include/ffs_hip.h (one class per opaque handle)."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def lib_path() -> str:
    # FFS_HIP_LIB: an alternative build of the same library (A/B experiments); there is no fallback
    return os.environ.get("FFS_HIP_LIB") or os.path.join(_PKG, "libffs_hip.so")


class FfsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libffs_hip error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    """ffs_params (include/ffs_hip.h)."""
    _fields_ = [("min_count", C.c_int32), ("nsig_b", C.c_double), ("nsig_s", C.c_double),
                ("threshold", C.c_double), ("max_valid", C.c_int64),
                ("min_spot_size", C.c_uint32), ("min_spot_size_3d", C.c_uint32),
                ("max_peak_centroid_separation", C.c_float),
                ("want_reflections", C.c_int32), ("want_strong_list", C.c_int32),
                ("want_strong_mask", C.c_int32), ("algorithm", C.c_int32), ("extended_flavour", C.c_int32),
                ("kernel_half_x", C.c_int32), ("kernel_half_y", C.c_int32)]   # window half-sizes, 1..7 (0 = 3)


ALGO_DISPERSION, ALGO_DISPERSION_EXTENDED = 0, 1


class _Box(C.Structure):
    _fields_ = [("l", C.c_uint32), ("t", C.c_uint32), ("r", C.c_uint32), ("b", C.c_uint32),
                ("num_pixels", C.c_int32)]


class _Refl(C.Structure):
    _fields_ = [("x_min", C.c_uint32), ("x_max", C.c_uint32), ("y_min", C.c_uint32), ("y_max", C.c_uint32),
                ("z_min", C.c_int32), ("z_max", C.c_int32), ("num_pixels", C.c_int32),
                ("com_x", C.c_float), ("com_y", C.c_float), ("com_z", C.c_float),
                ("peak_x", C.c_uint32), ("peak_y", C.c_uint32), ("peak_z", C.c_int32),
                ("peak_intensity", C.c_uint32), ("peak_centroid_distance", C.c_float),
                ("flags", C.c_uint32), ("sum_intensity", C.c_uint64)]


class _FrameResult(C.Structure):
    _fields_ = [("frame_id", C.c_int64), ("num_strong_pixels", C.c_uint32),
                ("num_strong_pixels_filtered", C.c_uint32), ("n_components", C.c_uint32),
                ("n_boxes", C.c_uint32), ("boxes", C.POINTER(_Box)),
                ("n_reflections", C.c_uint32), ("reflections", C.POINTER(_Refl)),
                ("n_filtered_size", C.c_uint32), ("n_filtered_sep", C.c_uint32),
                ("strong_k", C.POINTER(C.c_uint32)), ("strong_intensity", C.POINTER(C.c_uint32)),
                ("strong_mask", C.POINTER(C.c_uint8))]


BOX_DT = np.dtype([("l", "<u4"), ("t", "<u4"), ("r", "<u4"), ("b", "<u4"), ("num_pixels", "<i4")])
REFL_DT = np.dtype([("x_min", "<u4"), ("x_max", "<u4"), ("y_min", "<u4"), ("y_max", "<u4"),
                    ("z_min", "<i4"), ("z_max", "<i4"), ("num_pixels", "<i4"),
                    ("com_x", "<f4"), ("com_y", "<f4"), ("com_z", "<f4"),
                    ("peak_x", "<u4"), ("peak_y", "<u4"), ("peak_z", "<i4"),
                    ("peak_intensity", "<u4"), ("peak_centroid_distance", "<f4"),
                    ("flags", "<u4"), ("sum_intensity", "<u8")])
assert REFL_DT.itemsize == C.sizeof(_Refl) and BOX_DT.itemsize == C.sizeof(_Box)


class _RadialProfile(C.Structure):   # ffs_radial_profile
    _fields_ = [("n_bins", C.c_uint32), ("count", C.POINTER(C.c_uint32)), ("sum", C.POINTER(C.c_uint64)), ("sum_sq", C.POINTER(C.c_uint64))]


RADIAL_NO_BIN = 0xFFFF   # a bin-map entry that is in no bin (Context.set_radial_bins)


class _PixelStats(C.Structure):   # ffs_pixel_stats
    _fields_ = [("n_frames", C.c_uint64), ("count", C.POINTER(C.c_uint32)), ("sum", C.POINTER(C.c_uint64)), ("sum_sq", C.POINTER(C.c_uint64)),
                ("max", C.POINTER(C.c_uint32))]


class _SpotBackground(C.Structure):   # ffs_spot_background
    _fields_ = [("n_pixels", C.c_uint32), ("n_overflow", C.c_uint32), ("q1", C.c_int32), ("median", C.c_int32), ("q3", C.c_int32),
                ("n_inliers", C.c_uint32), ("inlier_sum", C.c_uint64), ("status", C.c_uint32), ("reserved", C.c_uint32), ("mean", C.c_double)]


SPOT_BG_DT = np.dtype([("n_pixels", "<u4"), ("n_overflow", "<u4"), ("q1", "<i4"), ("median", "<i4"), ("q3", "<i4"), ("n_inliers", "<u4"),
                       ("inlier_sum", "<u8"), ("status", "<u4"), ("reserved", "<u4"), ("mean", "<f8")])
assert SPOT_BG_DT.itemsize == C.sizeof(_SpotBackground) == 48
# FFS_SPOT_BG_*: the status of a spot's background estimate
SPOT_BG_OK, SPOT_BG_NO_PIXELS, SPOT_BG_OVERFLOW, SPOT_BG_RANGE, SPOT_BG_NO_INLIERS = 0, 1, 2, 3, 4
# ... continued by the robust GLM model (ffs_stream_spot_backgrounds_glm)
SPOT_BG_FEW_PIXELS, SPOT_BG_DEGENERATE, SPOT_BG_NOT_CONVERGED = 5, 6, 7


class _SpotBackgroundGlm(C.Structure):   # ffs_spot_background_glm
    _fields_ = [("n_pixels", C.c_uint32), ("n_overflow", C.c_uint32), ("median", C.c_int32), ("n_iter", C.c_uint32), ("status", C.c_uint32),
                ("reserved", C.c_uint32), ("beta", C.c_double), ("mean", C.c_double)]


SPOT_BG_GLM_DT = np.dtype([("n_pixels", "<u4"), ("n_overflow", "<u4"), ("median", "<i4"), ("n_iter", "<u4"), ("status", "<u4"), ("reserved", "<u4"),
                           ("beta", "<f8"), ("mean", "<f8")])
assert SPOT_BG_GLM_DT.itemsize == C.sizeof(_SpotBackgroundGlm) == 40


# Summation integration of shoeboxes in Kabsch space (ffs_ctx_shoebox_begin, ffs_stream_shoebox_fold, ffs_ctx_get_shoebox_sums)
class _ScanGeometry(C.Structure):   # ffs_scan_geometry
    _fields_ = [("d_matrix", C.c_double * 9), ("pixel_size_mm", C.c_double * 2), ("wavelength", C.c_double), ("s0", C.c_double * 3),
                ("rot_axis", C.c_double * 3), ("osc_start_deg", C.c_double), ("osc_width_deg", C.c_double)]


SHOEBOX_DT = np.dtype([("s1", "<f8", (3,)), ("phi", "<f8"), ("x_min", "<i4"), ("x_max", "<i4"), ("y_min", "<i4"), ("y_max", "<i4"),
                       ("z_min", "<i4"), ("z_max", "<i4")])   # ffs_shoebox
SHOEBOX_SUM_DT = np.dtype([("fg_sum", "<u8"), ("m_x", "<u8"), ("m_y", "<u8"), ("m_z", "<u8"), ("fg_count", "<u4"), ("n_background", "<u4"),
                           ("n_overflow", "<u4"), ("flags", "<u4"), ("bg_status", "<u4"), ("reserved", "<u4"), ("bg_mean", "<f8"),
                           ("intensity", "<f8"), ("variance", "<f8")])   # ffs_shoebox_sum
assert C.sizeof(_ScanGeometry) == 160 and SHOEBOX_DT.itemsize == 56 and SHOEBOX_SUM_DT.itemsize == 80
SHOEBOX_ELLIPSOID, SHOEBOX_DIALS = 0, 1   # FFS_SHOEBOX_*: what Context.shoebox_begin takes ("ellipsoid" / "dials")
SHOEBOX_ALGORITHMS = {"ellipsoid": SHOEBOX_ELLIPSOID, "dials": SHOEBOX_DIALS}
SHOEBOX_FG_INVALID = 1                    # FFS_SHOEBOX_FG_INVALID, in a record's flags
SHOEBOX_BACKGROUNDS = {"tukey": 0, "glm": 1}


# Scan prediction for a rotation sweep (ffs_predict_scan_settings, ffs_ctx_predict)
class _Crystal(C.Structure):   # ffs_crystal
    _fields_ = [("a_matrix", C.c_double * 9), ("centring", C.c_int32), ("reserved", C.c_int32)]


# ffs_prediction: the ffs_shoebox first (its fields by their own names), then the predicted centre, the index and the flags
PREDICTION_DT = np.dtype(SHOEBOX_DT.descr + [("x_px", "<f8"), ("y_px", "<f8"), ("z", "<f8"), ("h", "<i4"), ("k", "<i4"), ("l", "<i4"), ("flags", "<u4")])
assert C.sizeof(_Crystal) == 80 and PREDICTION_DT.itemsize == 96
CENTRINGS = {"P": 0, "I": 1, "F": 2, "A": 3, "B": 4, "C": 5, "R": 6}   # FFS_CENTRING_*
PREDICT_ENTERING, PREDICT_CORNER_LOST, PREDICT_ZETA_SMALL, PREDICT_BOX_REFUSED = 1, 2, 4, 8   # FFS_PREDICT_*, in a record's flags


# The indexer's basis-vector search (ffs_index_*, ffs_ctx_index_*)
INDEX_PEAK_DT = np.dtype([("root", "<u4"), ("n_voxels", "<u4"), ("sum", "<i8", (3,)), ("frac", "<f8", (3,))])   # ffs_index_peak
INDEX_VECTOR_DT = np.dtype([("v", "<f8", (3,)), ("length", "<f8"), ("volume", "<u4"), ("reserved", "<u4")])   # ffs_index_vector


class _IndexGridStats(C.Structure):   # ffs_index_grid_stats
    _fields_ = [("sum", C.c_double), ("mean", C.c_double), ("rmsd", C.c_double), ("cutoff", C.c_double), ("n_selected", C.c_uint32), ("n_peaks", C.c_uint32)]


assert INDEX_PEAK_DT.itemsize == 56 and INDEX_VECTOR_DT.itemsize == 40 and C.sizeof(_IndexGridStats) == 40
# the stages of ffs_ctx_index_launch_ms, in its order (FFS_INDEX_LAUNCH_SPANS of them)
INDEX_LAUNCH_SPANS = ("fill_scatter", "fft_axis0", "fft_axis1", "fft_axis2_power", "sum_trees", "second_statistic", "selection", "union_flatten", "reduce_records")
INDEX_NOT_USED = 0xFFFFFFFF   # ffs_index_map: a spot that is not mapped
INDEX_RMSD_CUTOFF, INDEX_PEAK_VOLUME_CUTOFF, INDEX_MIN_CELL = 15.0, 0.15, 3.0   # the reference's constants (indexer.cc:234-245)
# Index assignment (ffs_index_select / settings / absence_* / reindex, ffs_ctx_index_assign)
INDEX_ABSENCE_TESTS, INDEX_ASSIGN_SINGULAR = 111, 1
INDEX_ASSIGNMENT_DT = np.dtype([("status", "<u4"), ("n_accepted", "<u4"), ("n_indexed", "<u4"), ("n_out_of_range", "<u4"), ("sum_lsq_q40", "<u8"),
                                ("absent0", "<u4", (INDEX_ABSENCE_TESTS,)), ("reserved", "<u4")])   # ffs_index_assignment
INDEX_ABSENCE_TEST_DT = np.dtype([("v", "<i4", (3,)), ("modularity", "<i4"), ("transform", "<i4", (9,)), ("reserved", "<i4")])   # ffs_index_absence_test
INDEX_SETTING_DT = np.dtype([("triple", "<u4", (3,)), ("reserved", "<u4"), ("axes", "<f8", (9,)), ("A", "<f8", (9,))])   # ffs_index_setting
assert INDEX_ASSIGNMENT_DT.itemsize == 472 and INDEX_ABSENCE_TEST_DT.itemsize == 56 and INDEX_SETTING_DT.itemsize == 160
INDEX_ASSIGN_LAUNCH_SPANS = ("assign", "duplicates", "reduce")   # the stages of ffs_ctx_index_assign_launch_ms, in its order
INDEX_ASSIGN_TOLERANCE, INDEX_ABSENCE_THRESHOLD, INDEX_MAX_COMBINATIONS = 0.3, 0.9, 1000   # the reference's defaults


# ffs_radial_shell: what the radial-profile threshold decided for one (frame, shell) -- Stream.radial_thresholds
RADIAL_SHELL_DT = np.dtype([("n_pixels", "<u4"), ("n_overflow", "<u4"), ("q1", "<i4"), ("median", "<i4"), ("q3", "<i4"), ("cutoff", "<u4"),
                            ("status", "<u4"), ("reserved", "<u4")])
assert RADIAL_SHELL_DT.itemsize == 32
RADIAL_THR_OK, RADIAL_THR_EMPTY, RADIAL_THR_OVERFLOW = 0, 1, 2   # FFS_RADIAL_THR_*
ALGO_RADIAL_PROFILE = 2   # FFS_ALGO_RADIAL_PROFILE: Context.set_params(algorithm=...), with a bin map of at most 128 bins set
RADIAL_BLUR_NONE, RADIAL_BLUR_NARROW, RADIAL_BLUR_WIDE = 0, 1, 2   # FFS_RADIAL_BLUR_*: what Context.set_radial_blur takes ("none" / "narrow" / "wide")
RADIAL_BLURS = {"none": RADIAL_BLUR_NONE, "narrow": RADIAL_BLUR_NARROW, "wide": RADIAL_BLUR_WIDE}


PIXEL_STATS_MODES = {"off": 0, "start": 1, "resume": 2}   # FFS_PIXEL_STATS_OFF / _START / _RESUME
# ffs_frame_result as a numpy record (offsets taken from the ctypes structure: pointers and padding included)
_FRAME_RESULT_DT = np.dtype({"names": ["frame_id", "num_strong_pixels", "num_strong_pixels_filtered", "n_components", "n_boxes", "n_reflections"],
                             "formats": ["<i8", "<u4", "<u4", "<u4", "<u4", "<u4"],
                             "offsets": [getattr(_FrameResult, f).offset for f in
                                         ("frame_id", "num_strong_pixels", "num_strong_pixels_filtered", "n_components", "n_boxes", "n_reflections")],
                             "itemsize": C.sizeof(_FrameResult)})

MAX_VALID_CENTRE, MAX_VALID_WINDOW = 0, 1   # FFS_MAX_VALID_*: what Context.set_max_valid_scope takes ("centre" / "window")

CODEC_BSLZ4 = 0         # FFS_CODEC_*: what Stream.submit_encoded / decode_only take
CODEC_BYTE_OFFSET = 1
CODEC_JUNGFRAU_RAW = 2  # raw Jungfrau words (uint16 arrays or bytes), converted with Context.set_jungfrau_calibration


class _JungfrauCalibration(C.Structure):   # ffs_jungfrau_calibration
    _fields_ = [("pedestal", C.c_void_p * 3), ("factor", C.c_void_p * 3)]


class _JungfrauPedestalStats(C.Structure):   # ffs_jungfrau_pedestal_stats
    _fields_ = [("n_frames", C.c_uint64), ("count", C.c_void_p * 3), ("sum", C.c_void_p * 3), ("sum_sq", C.c_void_p * 3)]

# every symbol include/ffs_hip.h declares (tests check the library exports them all)
EXPORTS = [
    "ffs_default_params", "ffs_device_count", "ffs_device_name", "ffs_device_total_mem",
    "ffs_ctx_create", "ffs_ctx_destroy", "ffs_last_error", "ffs_ctx_set_mask",
    "ffs_ctx_apply_resolution_mask", "ffs_ctx_get_mask", "ffs_ctx_set_params",
    "ffs_stream_create", "ffs_stream_destroy", "ffs_stream_host_buffer", "ffs_submit",
    "ffs_submit_device", "ffs_ctx_device_layout", "ffs_wait", "ffs_stream_batch_arrays", "ffs_stream_timings",
    "ffs_submit_compressed", "ffs_decode_only", "ffs_submit_encoded", "ffs_decode_only_encoded", "ffs_stream_spot_centres", "ffs_bench_threshold", "ffs_bench_hbm", "ffs_stream_debug_planes", "ffs_stream_debug_bitplane", "ffs_selftest_sqrt", "ffs_stack3d_create",
    "ffs_stack3d_destroy", "ffs_stack3d_add_batch", "ffs_stack3d_add_slice", "ffs_stack3d_finish", "ffs_stack3d_signals", "ffs_stack3d_last_finish_ms", "ffs_multi_init", "ffs_multi_transport",
    "ffs_ctx_set_tuning", "ffs_bench_pipeline", "ffs_device_numa_node", "ffs_stream_reserve_host", "ffs_stream_last_path", "ffs_multi_gather_rows",
    "ffs_ctx_set_max_valid_scope", "ffs_ctx_set_gain", "ffs_ctx_set_gain_map",
    "ffs_ctx_set_radial_bins", "ffs_stream_radial_profile", "ffs_bench_radial",
    "ffs_ctx_set_pixel_stats", "ffs_ctx_get_pixel_stats", "ffs_bench_pixel_stats",
    "ffs_stream_spot_backgrounds",
    "ffs_stream_spot_backgrounds_glm",
    "ffs_ctx_set_radial_threshold", "ffs_stream_radial_thresholds", "ffs_ctx_set_radial_blur",
    "ffs_ctx_set_jungfrau_calibration",
    "ffs_ctx_jungfrau_pedestal_begin", "ffs_ctx_jungfrau_pedestal_end", "ffs_stream_jungfrau_pedestal_fold", "ffs_ctx_get_jungfrau_pedestal",
    "ffs_jungfrau_pedestal_planes",
    "ffs_ctx_shoebox_begin", "ffs_ctx_shoebox_end", "ffs_stream_shoebox_fold", "ffs_ctx_get_shoebox_sums", "ffs_ctx_get_shoebox_histogram",
    "ffs_predict_scan_settings", "ffs_ctx_predict",
    "ffs_index_rlp", "ffs_index_defaults", "ffs_index_twiddles", "ffs_index_map", "ffs_index_basis_vectors",
    "ffs_ctx_index_grid", "ffs_ctx_index_load_grid", "ffs_ctx_index_peaks", "ffs_ctx_index_launch_ms",
    "ffs_index_select", "ffs_index_settings", "ffs_index_absence_table", "ffs_index_absence_detect", "ffs_index_reindex",
    "ffs_ctx_index_assign", "ffs_ctx_index_assign_launch_ms",
]

_lib = None


def load_library():
    """dlopen libffs_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        p = lib_path()
        if not os.path.exists(p):
            raise RuntimeError(f"{p} is missing: run `make hip` or __graft_entry__.build(). "
                               "There is no CPU fallback for the product path.")
        L = C.CDLL(p)
        L.ffs_last_error.restype = C.c_char_p
        L.ffs_last_error.argtypes = [C.c_void_p]
        L.ffs_ctx_create.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
                                     C.POINTER(C.c_void_p)]
        L.ffs_ctx_destroy.argtypes = [C.c_void_p]
        L.ffs_ctx_set_mask.argtypes = [C.c_void_p, C.c_void_p]
        L.ffs_ctx_get_mask.argtypes = [C.c_void_p, C.c_void_p]
        L.ffs_ctx_set_params.argtypes = [C.c_void_p, C.POINTER(Params)]
        L.ffs_ctx_set_tuning.argtypes = [C.c_void_p, C.c_char_p, C.c_longlong]
        L.ffs_ctx_set_max_valid_scope.argtypes = [C.c_void_p, C.c_int]
        L.ffs_ctx_set_gain.argtypes = [C.c_void_p, C.c_double]
        L.ffs_ctx_set_gain_map.argtypes = [C.c_void_p, C.c_void_p]
        L.ffs_ctx_set_jungfrau_calibration.argtypes = [C.c_void_p, C.POINTER(_JungfrauCalibration)]
        L.ffs_ctx_jungfrau_pedestal_begin.argtypes = [C.c_void_p]
        L.ffs_ctx_jungfrau_pedestal_end.argtypes = [C.c_void_p]
        L.ffs_stream_jungfrau_pedestal_fold.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_uint32, C.POINTER(C.c_float)]
        L.ffs_ctx_get_jungfrau_pedestal.argtypes = [C.c_void_p, C.POINTER(_JungfrauPedestalStats)]
        L.ffs_jungfrau_pedestal_planes.argtypes = [C.POINTER(_JungfrauPedestalStats), C.c_size_t, C.c_uint32, C.c_float, C.POINTER(C.c_void_p),
                                                   C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.ffs_ctx_set_radial_bins.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.ffs_stream_radial_profile.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(_RadialProfile)]
        L.ffs_bench_radial.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
        L.ffs_ctx_set_radial_threshold.argtypes = [C.c_void_p, C.c_double]
        L.ffs_ctx_set_radial_blur.argtypes = [C.c_void_p, C.c_int]
        L.ffs_stream_radial_thresholds.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
        L.ffs_ctx_set_pixel_stats.argtypes = [C.c_void_p, C.c_int]
        L.ffs_ctx_get_pixel_stats.argtypes = [C.c_void_p, C.POINTER(_PixelStats)]
        L.ffs_bench_pixel_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
        L.ffs_stream_spot_backgrounds.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
        L.ffs_stream_spot_backgrounds_glm.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
        L.ffs_ctx_shoebox_begin.argtypes = [C.c_void_p, C.POINTER(_ScanGeometry), C.c_void_p, C.c_uint32, C.c_int, C.c_double, C.c_double]
        L.ffs_ctx_shoebox_end.argtypes = [C.c_void_p]
        L.ffs_stream_shoebox_fold.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_float)]
        L.ffs_ctx_get_shoebox_sums.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.ffs_ctx_get_shoebox_histogram.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.ffs_predict_scan_settings.argtypes = [C.POINTER(_ScanGeometry), C.POINTER(_Crystal), C.c_uint32, C.c_void_p]
        L.ffs_ctx_predict.argtypes = [C.c_void_p, C.POINTER(_ScanGeometry), C.POINTER(_Crystal), C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_void_p,
                                      C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
        L.ffs_index_rlp.argtypes = [C.POINTER(_ScanGeometry), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ffs_index_defaults.argtypes = [C.c_void_p, C.c_uint32, C.c_double, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.ffs_index_twiddles.argtypes = [C.c_uint32, C.c_void_p]
        L.ffs_index_map.argtypes = [C.c_void_p, C.c_uint32, C.c_double, C.c_double, C.c_uint32, C.c_void_p, C.c_void_p]
        L.ffs_index_basis_vectors.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_uint32,
                                              C.POINTER(C.c_uint32)]
        L.ffs_ctx_index_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_double, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.ffs_ctx_index_load_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.ffs_ctx_index_peaks.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(_IndexGridStats), C.POINTER(C.c_float)]
        L.ffs_ctx_index_launch_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.ffs_index_select.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_double, C.c_void_p]
        L.ffs_index_settings.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.ffs_index_absence_table.argtypes = [C.c_void_p]
        L.ffs_index_absence_detect.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_int32)]
        L.ffs_index_reindex.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.ffs_ctx_index_assign.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_double, C.c_size_t, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
        L.ffs_ctx_index_assign_launch_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.ffs_bench_pipeline.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32,
                                         C.c_uint32, C.c_int64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.ffs_device_numa_node.argtypes = [C.c_int]
        L.ffs_stream_reserve_host.argtypes = [C.c_void_p, C.c_size_t]
        L.ffs_ctx_apply_resolution_mask.argtypes = [C.c_void_p] + [C.c_float] * 8
        L.ffs_ctx_device_layout.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.ffs_stream_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.ffs_stream_destroy.argtypes = [C.c_void_p]
        L.ffs_stream_host_buffer.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.ffs_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int64]
        L.ffs_submit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_int64]
        L.ffs_wait.argtypes = [C.c_void_p, C.POINTER(C.POINTER(_FrameResult)), C.POINTER(C.c_uint32)]
        L.ffs_stream_timings.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.ffs_stream_last_path.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.ffs_stream_batch_arrays.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32),
                                              C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
        L.ffs_bench_threshold.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32,
                                          C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.ffs_multi_init.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_char_p]
        L.ffs_multi_transport.restype = C.c_char_p
        L.ffs_bench_hbm.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.ffs_stream_debug_planes.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                              C.POINTER(C.c_size_t)]
        L.ffs_stream_spot_centres.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.ffs_submit_compressed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int64]
        L.ffs_decode_only.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                      C.POINTER(C.c_float), C.c_void_p]
        L.ffs_submit_encoded.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int64]
        L.ffs_decode_only_encoded.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                              C.POINTER(C.c_float), C.c_void_p]
        L.ffs_stack3d_signals.argtypes = [C.c_void_p] * 7
        L.ffs_stream_debug_bitplane.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
        L.ffs_selftest_sqrt.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
        L.ffs_device_name.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
        L.ffs_device_total_mem.argtypes = [C.c_int, C.POINTER(C.c_uint64)]
        L.ffs_stack3d_create.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
        L.ffs_stack3d_destroy.argtypes = [C.c_void_p]
        L.ffs_stack3d_add_batch.argtypes = [C.c_void_p, C.c_void_p]
        L.ffs_stack3d_add_slice.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint32]
        L.ffs_stack3d_finish.argtypes = [C.c_void_p, C.POINTER(C.POINTER(_Refl)), C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        _lib = L
    return _lib


def device_count() -> int:
    return load_library().ffs_device_count()


def device_name(device: int = 0) -> str:
    buf = C.create_string_buffer(256)
    rc = load_library().ffs_device_name(device, buf, 256)
    if rc != 0:
        raise FfsError(rc, "no such device")
    return buf.value.decode()


def default_params() -> Params:
    p = Params()
    load_library().ffs_default_params(C.byref(p))
    return p


@dataclass
class FrameResult:
    frame_id: int
    num_strong_pixels: int
    num_strong_pixels_filtered: int
    n_components: int
    boxes: np.ndarray                      # BOX_DT, label order
    reflections: np.ndarray | None         # REFL_DT, after both filters
    n_filtered_size: int
    n_filtered_sep: int
    strong_k: np.ndarray | None = None
    strong_intensity: np.ndarray | None = None
    strong_mask: np.ndarray | None = None
    extra: dict = field(default_factory=dict)

    @property
    def n_spots_total(self) -> int:        # JSON key, spotfinder.cc:1002
        return len(self.boxes)


def _copy_array(ptr, n, ctype_struct, dt):
    if n == 0 or not ptr:
        return np.zeros(0, dt)
    raw = C.string_at(C.cast(ptr, C.c_void_p), n * C.sizeof(ctype_struct))
    return np.frombuffer(raw, dtype=dt).copy()


class Context:
    def __init__(self, width: int, height: int, dtype=np.uint16, max_batch: int = 1,
                 device: int = 0, max_strong_per_frame: int = 0):
        self._lib = load_library()
        self.W, self.H = int(width), int(height)
        self.dtype = np.dtype(dtype)
        assert self.dtype in (np.dtype(np.uint16), np.dtype(np.uint32))
        self.max_batch = int(max_batch)
        self.device = device
        h = C.c_void_p()
        rc = self._lib.ffs_ctx_create(device, self.W, self.H, self.dtype.itemsize, self.max_batch,
                                      max_strong_per_frame, C.byref(h))
        if rc != 0:
            raise FfsError(rc, self._lib.ffs_last_error(None).decode())
        self._h = h
        self.params = default_params()

    def _check(self, rc):
        if rc != 0:
            raise FfsError(rc, self._lib.ffs_last_error(self._h).decode())

    def set_mask(self, mask: np.ndarray | None):
        if mask is None:
            self._check(self._lib.ffs_ctx_set_mask(self._h, None))
            return
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        assert m.shape == (self.H, self.W)
        self._check(self._lib.ffs_ctx_set_mask(self._h, m.ctypes.data_as(C.c_void_p)))

    def get_mask(self) -> np.ndarray:
        m = np.empty((self.H, self.W), np.uint8)
        self._check(self._lib.ffs_ctx_get_mask(self._h, m.ctypes.data_as(C.c_void_p)))
        return m

    def apply_resolution_mask(self, wavelength, distance_m, beam_center_x_px, beam_center_y_px,
                              pixel_size_x_m, pixel_size_y_m, dmin=-1.0, dmax=-1.0):
        self._check(self._lib.ffs_ctx_apply_resolution_mask(
            self._h, wavelength, distance_m, beam_center_x_px, beam_center_y_px,
            pixel_size_x_m, pixel_size_y_m, dmin, dmax))

    def set_params(self, **kw):
        for k, v in kw.items():
            if not hasattr(self.params, k):
                raise AttributeError(k)
            setattr(self.params, k, v)
        self._check(self._lib.ffs_ctx_set_params(self._h, C.byref(self.params)))

    def set_max_valid_scope(self, scope):
        """ffs_ctx_set_max_valid_scope: "centre" (default: only a centre pixel above max_valid is refused, the reference kernels'
        behaviour) or "window" (such a pixel is masked for its frame: out of every window's count and sums); or the constants
        MAX_VALID_CENTRE / MAX_VALID_WINDOW.  Kept across set_params; a batch takes it as it is at submit."""
        if isinstance(scope, str):
            names = {"centre": MAX_VALID_CENTRE, "window": MAX_VALID_WINDOW}
            if scope not in names:
                raise ValueError(f"max_valid scope must be 'centre' or 'window', not {scope!r}")
            scope = names[scope]
        self._check(self._lib.ffs_ctx_set_max_valid_scope(self._h, int(scope)))

    def set_gain(self, gain):
        """ffs_ctx_set_gain: the detector gain of the dispersion tests (DIALS spotfinder.threshold.dispersion.gain) -- a background
        window's variance is gain * mean.  0 = off (photon counts, the default); any finite g > 0 selects the gain form of
        baseline.cpp (the general-window kernel at every window).  Kept across set_params; a batch takes it as it is at submit.
        Refused (FfsError, state unchanged): negative, NaN, infinite; g > 0 with extended_flavour 1."""
        self._check(self._lib.ffs_ctx_set_gain(self._h, float(gain)))

    def set_gain_map(self, gain_map: np.ndarray | None):
        """ffs_ctx_set_gain_map: the detector gain per pixel (DIALS spotfinder.lookup.gain_map), an H x W array converted to
        C-contiguous float32, or None for no map.  The arithmetic of set_gain with the gain of the pixel being decided (the window's
        centre).  A property of the context like the mask: kept across set_params.  Refused (FfsError, state unchanged): an entry
        that is not finite or outside [2^-60, 2^60]; with a scalar gain > 0 set; with extended_flavour 1; while a batch is in
        flight.  A wrong shape is a ValueError."""
        if gain_map is None:
            self._check(self._lib.ffs_ctx_set_gain_map(self._h, None))
            return
        g = np.ascontiguousarray(gain_map, dtype=np.float32)
        if g.shape != (self.H, self.W):
            raise ValueError(f"the gain map must have shape (H, W) = {(self.H, self.W)}, not {g.shape}")
        self._check(self._lib.ffs_ctx_set_gain_map(self._h, g.ctypes.data_as(C.c_void_p)))

    def set_jungfrau_calibration(self, pedestal: np.ndarray | None, factor: np.ndarray | None = None):
        """ffs_ctx_set_jungfrau_calibration: what CODEC_JUNGFRAU_RAW converts raw words with -- pedestal and factor (photons per ADU,
        0 = no calibration for the pixel in that stage), each (3, H, W) for the stages G0, G1, G2, converted to C-contiguous float32;
        None drops the calibration.  A property of the context like the mask: kept across set_params, replaceable between batches.
        Refused (FfsError, state unchanged): a uint16 context; an entry that is not finite, a pedestal outside [-65536, 65536], a
        factor neither 0 nor of magnitude in [2^-30, 2^16] (the text names plane and index); while a batch is in flight.  A wrong
        shape is a ValueError."""
        if pedestal is None:
            self._check(self._lib.ffs_ctx_set_jungfrau_calibration(self._h, None))
            return
        p = np.ascontiguousarray(pedestal, dtype=np.float32)
        f = np.ascontiguousarray(factor, dtype=np.float32)
        if p.shape != (3, self.H, self.W) or f.shape != (3, self.H, self.W):
            raise ValueError(f"pedestal and factor must have shape (3, H, W) = {(3, self.H, self.W)}, not {p.shape} and {f.shape}")
        cal = _JungfrauCalibration()
        for s in range(3):
            cal.pedestal[s] = p[s].ctypes.data
            cal.factor[s] = f[s].ctypes.data
        self._check(self._lib.ffs_ctx_set_jungfrau_calibration(self._h, C.byref(cal)))

    def set_radial_bins(self, bins: np.ndarray | None, n_bins=None):
        """ffs_ctx_set_radial_bins: the bin map of the per-frame radial profile, an H x W array of bin indices (converted to
        C-contiguous uint16; RADIAL_NO_BIN = 0xFFFF is "in no bin"), or None for no map (the default).  n_bins (1..1024) defaults
        to max + 1 over the entries other than 0xFFFF (1 when there is none).  A property of the context like the mask: kept across
        set_params; a batch takes it at submit, and Stream.radial_profile reads its profile after wait().  Refused (FfsError, state
        unchanged): n_bins outside 1..1024; an entry >= n_bins that is not 0xFFFF; a map while a batch is in flight.  A wrong shape,
        or an entry that no uint16 holds, is a ValueError."""
        if bins is None:
            self._check(self._lib.ffs_ctx_set_radial_bins(self._h, None, 0))
            return
        a = np.asarray(bins)
        if a.shape != (self.H, self.W):
            raise ValueError(f"the bin map must have shape (H, W) = {(self.H, self.W)}, not {a.shape}")
        if a.dtype.kind not in "iu" or (a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFF)):
            raise ValueError("the bin map must hold integers in 0..65535 (0xFFFF = in no bin)")
        b = np.ascontiguousarray(a, dtype=np.uint16)
        if n_bins is None:
            used = b[b != RADIAL_NO_BIN]
            n_bins = int(used.max()) + 1 if used.size else 1
        self._check(self._lib.ffs_ctx_set_radial_bins(self._h, b.ctypes.data_as(C.c_void_p), int(n_bins)))

    def set_radial_threshold(self, n_iqr: float):
        """ffs_ctx_set_radial_threshold: n_iqr of the radial-profile threshold (set_params(algorithm=ALGO_RADIAL_PROFILE)) -- a pixel is
        strong above floor(median + n_iqr * iqr) of its shell.  Default 6.  Kept across set_params; a batch takes it as it is at submit.
        Refused (FfsError, state unchanged): NaN, infinite, below 0 or above 2^20."""
        self._check(self._lib.ffs_ctx_set_radial_threshold(self._h, float(n_iqr)))

    def set_radial_blur(self, blur):
        """ffs_ctx_set_radial_blur: "none" (default), "narrow" (3 x 3, (1 2 1) x (1 2 1) / 16) or "wide" (5 x 5, (1 4 6 4 1) x (1 4 6 4 1) / 256),
        or the integers RADIAL_BLUR_* -- the radial-profile threshold then decides on the image smoothed over its valid pixels, and a strong
        pixel also has p >= 1; everything behind the strong plane reads the raw pixels.  Kept across set_params, accepted under any
        algorithm; a batch takes it as it is at submit.  Refused (FfsError, state unchanged): any other value."""
        if isinstance(blur, str):
            if blur not in RADIAL_BLURS:
                raise ValueError('blur must be "none", "narrow" or "wide", got %r' % (blur,))
            blur = RADIAL_BLURS[blur]
        self._check(self._lib.ffs_ctx_set_radial_blur(self._h, int(blur)))

    def set_pixel_stats(self, mode: str):
        """ffs_ctx_set_pixel_stats: "start" (zero the per-pixel statistics and accumulate every frame submitted on the context from now
        on), "off" (stop; the values stay readable; accepted at any time) or "resume" (go on, values kept; a start if there was none).
        FfsError, state unchanged: "start" while a batch is in flight.  Any other word is a ValueError."""
        if mode not in PIXEL_STATS_MODES:
            raise ValueError(f"pixel statistics mode must be one of {sorted(PIXEL_STATS_MODES)}, not {mode!r}")
        self._check(self._lib.ffs_ctx_set_pixel_stats(self._h, PIXEL_STATS_MODES[mode]))

    def pixel_stats(self, planes=("count", "sum", "sum_sq", "max")):
        """ffs_ctx_get_pixel_stats: (n_frames, count uint32, sum uint64, sum_sq uint64 modulo 2^64, max uint32), H x W arrays over all frames
        folded in since the last start; a plane not named in `planes` is None (and is not copied).  FfsError before any start and while a
        batch is in flight."""
        out = _PixelStats()
        arrays = {}
        for name, dt, ct in (("count", np.uint32, C.c_uint32), ("sum", np.uint64, C.c_uint64), ("sum_sq", np.uint64, C.c_uint64), ("max", np.uint32, C.c_uint32)):
            if name in planes:
                arrays[name] = np.zeros((self.H, self.W), dt)
                setattr(out, name, arrays[name].ctypes.data_as(C.POINTER(ct)))
        self._check(self._lib.ffs_ctx_get_pixel_stats(self._h, C.byref(out)))
        return (int(out.n_frames), arrays.get("count"), arrays.get("sum"), arrays.get("sum_sq"), arrays.get("max"))

    def jungfrau_pedestal_begin(self):
        """ffs_ctx_jungfrau_pedestal_begin: allocate (first use) and zero the accumulators of the dark-frame fold (60 bytes a pixel) and the
        frame count.  FfsError, state unchanged: a uint16 context; while a batch or a fold is in flight."""
        self._check(self._lib.ffs_ctx_jungfrau_pedestal_begin(self._h))

    def jungfrau_pedestal_end(self):
        """ffs_ctx_jungfrau_pedestal_end: free the accumulators; idempotent.  FfsError while a batch or a fold is in flight."""
        self._check(self._lib.ffs_ctx_jungfrau_pedestal_end(self._h))

    def jungfrau_pedestal(self, planes=("count", "sum", "sum_sq")):
        """ffs_ctx_get_jungfrau_pedestal: (n_frames, count uint32, sum uint64, sum_sq uint64), each (3, H, W) for the stages G0, G1, G2, over
        every frame folded since the last begin (Stream.jungfrau_pedestal_fold); a plane set not named in `planes` is None (and is not
        copied).  What jungfrau_pedestal_planes takes.  FfsError before begin, after end and while a batch or a fold is in flight."""
        out = _JungfrauPedestalStats()
        arrays = {}
        for name, dt in (("count", np.uint32), ("sum", np.uint64), ("sum_sq", np.uint64)):
            if name in planes:
                arrays[name] = np.zeros((3, self.H, self.W), dt)
                for s in range(3):
                    getattr(out, name)[s] = arrays[name][s].ctypes.data
        self._check(self._lib.ffs_ctx_get_jungfrau_pedestal(self._h, C.byref(out)))
        return (int(out.n_frames), arrays.get("count"), arrays.get("sum"), arrays.get("sum_sq"))

    def shoebox_begin(self, geometry, shoeboxes, algorithm="ellipsoid", *, delta_b: float, delta_m: float):
        """ffs_ctx_shoebox_begin: open a summation-integration job.  geometry: a mapping (or object) with d_matrix (9, row-major),
        pixel_size_mm (2), wavelength, s0 (3), rot_axis (3), osc_start_deg, osc_width_deg; shoeboxes: a structured array of SHOEBOX_DT (s1,
        phi in radians, the half-open box); algorithm "ellipsoid" or "dials" (or FFS_SHOEBOX_*); delta_b, delta_m: n_sigma * sigma in
        radians.  FfsError (state unchanged): a batch in flight, a job already open, a delta that is not finite and positive, an unknown
        algorithm, a table entry the library names."""
        g = _scan_geometry(geometry)
        t = np.ascontiguousarray(shoeboxes, dtype=SHOEBOX_DT)
        algo = SHOEBOX_ALGORITHMS.get(algorithm, algorithm) if isinstance(algorithm, str) else algorithm
        if isinstance(algo, str):
            raise ValueError(f"algorithm must be one of {sorted(SHOEBOX_ALGORITHMS)}, not {algorithm!r}")
        self._check(self._lib.ffs_ctx_shoebox_begin(self._h, C.byref(g), t.ctypes.data_as(C.c_void_p) if len(t) else None, len(t), int(algo),
                                                    float(delta_b), float(delta_m)))

    def shoebox_end(self):
        """ffs_ctx_shoebox_end: free the job; idempotent."""
        self._check(self._lib.ffs_ctx_shoebox_end(self._h))

    def shoebox_sums(self, background="tukey"):
        """ffs_ctx_get_shoebox_sums: one record (SHOEBOX_SUM_DT) per shoebox in table order, from everything folded so far
        (Stream.shoebox_fold); background "tukey" or "glm" (or 0 / 1): the model the box's histogram is put through."""
        model = SHOEBOX_BACKGROUNDS.get(background, background) if isinstance(background, str) else background
        if isinstance(model, str):
            raise ValueError(f"background must be one of {sorted(SHOEBOX_BACKGROUNDS)}, not {background!r}")
        n = C.c_uint32()
        rc = self._lib.ffs_ctx_get_shoebox_sums(self._h, int(model), None, 0, C.byref(n))
        if rc != -4:   # FFS_ERR_OVERFLOW: the table's length is in n
            self._check(rc)
        out = np.zeros(n.value, SHOEBOX_SUM_DT)
        if n.value:
            self._check(self._lib.ffs_ctx_get_shoebox_sums(self._h, int(model), out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return out

    def shoebox_histogram(self, index: int) -> np.ndarray:
        """ffs_ctx_get_shoebox_histogram: the 256 raw bins of shoebox `index` (uint32)."""
        bins = np.zeros(256, np.uint32)
        self._check(self._lib.ffs_ctx_get_shoebox_histogram(self._h, int(index), bins.ctypes.data_as(C.c_void_p)))
        return bins

    def predict(self, geometry, a_matrix, n_images: int, dmin: float, delta_b: float, delta_m: float, centring="P", *, cap=None, want_ms: bool = False):
        """ffs_ctx_predict: the reflections of images 0 .. n_images - 1 of a rotation scan on this context's image and their shoeboxes, as a
        structured array of PREDICTION_DT in the order of candidate number, then image.  geometry: as Context.shoebox_begin takes it;
        a_matrix: 9 entries row-major, 1/Angstrom, r = A h at rotation angle 0; delta_b, delta_m: n_sigma * sigma in radians; centring: one
        of "PIFABCR" (or FFS_CENTRING_*).  cap (optional): at most that many records are fetched; FfsError -4 (FFS_ERR_OVERFLOW) when there
        are more -- its `records` and `n` attributes carry what was written and the full count.  want_ms: also return the kernels' time.
        May be called while batches of the context are in flight.  FfsError (nothing changed): what include/ffs_hip.h lists."""
        g, x = _scan_geometry(geometry), _crystal(a_matrix, centring)
        n, ms = C.c_uint32(), C.c_float()
        args = (self._h, C.byref(g), C.byref(x), int(n_images), float(dmin), float(delta_b), float(delta_m))
        if cap is None:
            rc = self._lib.ffs_ctx_predict(*args, None, 0, C.byref(n), None)
            if rc != -4:   # FFS_ERR_OVERFLOW: the count is in n
                self._check(rc)
            cap = n.value
        out = np.zeros(int(cap), PREDICTION_DT)
        rc = self._lib.ffs_ctx_predict(*args, out.ctypes.data_as(C.c_void_p) if cap else None, int(cap), C.byref(n), C.byref(ms))
        if rc == -4:
            err = FfsError(rc, self._lib.ffs_last_error(self._h).decode())
            err.records, err.n = out, n.value
            raise err
        self._check(rc)
        out = out[:n.value]
        return (out, ms.value) if want_ms else out

    def index_grid(self, rlp, dmin: float, b_iso: float, n_points: int = 256, *, want_power: bool = False, want_ms: bool = False):
        """ffs_ctx_index_grid: maps the reciprocal-lattice points (n, 3) on a grid of n_points a side, transforms it on the GPU and leaves the
        power grid resident for index_peaks.  Returns `used` (n bools: the spot was mapped), then the power grid (n_points^3 float64, flat)
        when want_power, then the launches' time when want_ms.  May be called while batches of the context are in flight."""
        r = np.ascontiguousarray(np.asarray(rlp, np.float64).reshape(-1, 3))
        used = np.zeros(len(r), np.uint8)
        power = np.empty(int(n_points) ** 3, np.float64) if want_power and 0 < int(n_points) <= 256 else None
        ms = C.c_float()
        self._check(self._lib.ffs_ctx_index_grid(self._h, r.ctypes.data_as(C.c_void_p) if len(r) else None, len(r), float(dmin), float(b_iso), int(n_points),
                                                 used.ctypes.data_as(C.c_void_p), power.ctypes.data_as(C.c_void_p) if power is not None else None, C.byref(ms)))
        out = (used.astype(bool),) + ((power,) if want_power else ()) + ((ms.value,) if want_ms else ())
        return out[0] if len(out) == 1 else out

    def index_load_grid(self, power, n_points: int):
        """ffs_ctx_index_load_grid: a caller's power grid (n_points^3 float64) in place of the resident one."""
        g = np.ascontiguousarray(np.asarray(power, np.float64).reshape(-1))
        if g.size != int(n_points) ** 3:
            raise ValueError(f"power must have n_points^3 = {int(n_points) ** 3} entries, not {g.size}")
        self._check(self._lib.ffs_ctx_index_load_grid(self._h, g.ctypes.data_as(C.c_void_p), int(n_points)))

    def index_peaks(self, rmsd_cutoff: float = INDEX_RMSD_CUTOFF, *, cap=None, want_ms: bool = False):
        """ffs_ctx_index_peaks: (records of INDEX_PEAK_DT in ascending order of root, the grid's statistics as a dict) of the resident grid.
        cap (optional): at most that many records are fetched; FfsError -4 (FFS_ERR_OVERFLOW) when there are more -- its `records`, `n`
        and `stats` attributes carry what was written.  want_ms: also return the kernels' time."""
        n, ms, st = C.c_uint32(), C.c_float(), _IndexGridStats()
        if cap is None:
            rc = self._lib.ffs_ctx_index_peaks(self._h, float(rmsd_cutoff), None, 0, C.byref(n), None, None)
            if rc != -4:   # FFS_ERR_OVERFLOW: the count is in n
                self._check(rc)
            cap = n.value
        out = np.zeros(int(cap), INDEX_PEAK_DT)
        rc = self._lib.ffs_ctx_index_peaks(self._h, float(rmsd_cutoff), out.ctypes.data_as(C.c_void_p) if cap else None, int(cap), C.byref(n), C.byref(st), C.byref(ms))
        stats = {k: getattr(st, k) for k, _ in _IndexGridStats._fields_}
        if rc == -4:
            err = FfsError(rc, self._lib.ffs_last_error(self._h).decode())
            err.records, err.n, err.stats = out, n.value, stats
            raise err
        self._check(rc)
        out = out[:n.value]
        return (out, stats, ms.value) if want_ms else (out, stats)

    def index_launch_ms(self) -> dict:
        """ffs_ctx_index_launch_ms: where the launches' time of the last index_grid and the last index_peaks went, in ms by stage."""
        out = (C.c_float * len(INDEX_LAUNCH_SPANS))()
        self._check(self._lib.ffs_ctx_index_launch_ms(self._h, out))
        return dict(zip(INDEX_LAUNCH_SPANS, (float(v) for v in out)))

    def index_basis(self, xyz_px, geometry, max_cell: float, dmin=None, n_points: int = 256):
        """The chain of the reference's indexer up to its candidate basis vectors (indexer.cc:171-245) with its constants (rmsd_cutoff 15.0,
        peak_volume_cutoff 0.15, min_cell 3.0): spot centres (n, 3) of (x_px, y_px, z in images) -> records of INDEX_VECTOR_DT in Angstrom,
        sorted by volume.  The map, the filter and the vectors are host arithmetic; the transform and the peak search run on the GPU."""
        rlp, _, _ = index_rlp(geometry, xyz_px)
        dmin, b_iso = index_defaults(rlp, max_cell, n_points, dmin)
        self.index_grid(rlp, dmin, b_iso, n_points)
        peaks, _ = self.index_peaks(INDEX_RMSD_CUTOFF)
        return index_basis_vectors(peaks, n_points, dmin, max_cell)

    def index_assign(self, rlp, phi, A, *, selected=None, tolerance: float = INDEX_ASSIGN_TOLERANCE, workspace_bytes: int = 0, want_hkl: bool = False,
                     want_lsq: bool = False, want_ms: bool = False):
        """ffs_ctx_index_assign: the spots (rlp (n, 3), phi (n) in radians) under every setting of A (m, 9): records of INDEX_ASSIGNMENT_DT, then
        hkl (m, n, 3) int32 when want_hkl, lsq (m, n) float64 when want_lsq, and the three stages' time in ms when want_ms.  selected: n
        bools or None (all).  May be called while batches of the context are in flight."""
        r = np.ascontiguousarray(np.asarray(rlp, np.float64).reshape(-1, 3))
        p = np.ascontiguousarray(np.asarray(phi, np.float64).reshape(-1))
        a = np.ascontiguousarray(np.asarray(A, np.float64).reshape(-1, 9))
        if len(p) != len(r):
            raise ValueError(f"phi must have one entry a spot: {len(p)} for {len(r)} spots")
        sel = None
        if selected is not None:
            sel = np.ascontiguousarray(np.asarray(selected).astype(bool).astype(np.uint8).reshape(-1))
            if len(sel) != len(r):
                raise ValueError(f"selected must have one entry a spot: {len(sel)} for {len(r)} spots")
        n, m = len(r), len(a)
        out = np.zeros(m, INDEX_ASSIGNMENT_DT)
        hkl = np.zeros((m, n, 3), np.int32) if want_hkl else None
        lsq = np.full((m, n), -1.0, np.float64) if want_lsq else None

        def ptr(x):
            return x.ctypes.data_as(C.c_void_p) if x is not None and x.size else None
        # (an empty hkl or lsq still says "wanted": a pointer to something)
        dummy = np.zeros(1, np.float64)
        self._check(self._lib.ffs_ctx_index_assign(self._h, ptr(r), ptr(p), ptr(sel), n, ptr(a), m, float(tolerance), int(workspace_bytes), ptr(out),
                                                   (ptr(hkl) or ptr(dummy)) if want_hkl else None, (ptr(lsq) or ptr(dummy)) if want_lsq else None))
        res = (out,) + ((hkl,) if want_hkl else ()) + ((lsq,) if want_lsq else ())
        if want_ms:
            ms = (C.c_float * 3)()
            self._check(self._lib.ffs_ctx_index_assign_launch_ms(self._h, ms))
            res += (dict(zip(INDEX_ASSIGN_LAUNCH_SPANS, (float(v) for v in ms))),)
        return res[0] if len(res) == 1 else res

    def index_correct(self, rlp, phi, A, *, selected=None, tolerance: float = INDEX_ASSIGN_TOLERANCE, threshold: float = INDEX_ABSENCE_THRESHOLD, workspace_bytes: int = 0):
        """The loop of non_primitive_basis.cc:188-225 without its Niggli step, for one setting A (9): assign, detect, reindex, assign again
        until no absence is detected.  Returns (A', record, hkl (n, 3), rounds); raises after 16 reindexings (each at least halves the cell)."""
        a = np.ascontiguousarray(np.asarray(A, np.float64).reshape(9))
        for rounds in range(17):
            rec, hkl = self.index_assign(rlp, phi, a, selected=selected, tolerance=tolerance, workspace_bytes=workspace_bytes, want_hkl=True)
            t = index_absence_detect(rec[0], threshold)
            if t < 0:
                return a, rec[0], hkl[0], rounds
            a = index_reindex(a, t)
        raise RuntimeError("index_correct: still an absence after 16 reindexings")

    def set_tuning(self, **kw):
        """ffs_ctx_set_tuning: A/B partners, fall-backs and capacities (same results either way); see include/ffs_hip.h."""
        for k, v in kw.items():
            self._check(self._lib.ffs_ctx_set_tuning(self._h, k.encode(), int(v)))

    def selftest_sqrt(self, begin: int, end: int) -> int:
        out = C.c_uint64()
        self._check(self._lib.ffs_selftest_sqrt(self._h, begin, end, C.byref(out)))
        return out.value

    def device_layout(self):
        pitch, stride = C.c_size_t(), C.c_size_t()
        self._check(self._lib.ffs_ctx_device_layout(self._h, C.byref(pitch), C.byref(stride)))
        return pitch.value, stride.value

    def stream(self) -> "Stream":
        return Stream(self)

    def close(self):
        if self._h:
            self._lib.ffs_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Stream:
    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._lib = ctx._lib
        h = C.c_void_p()
        ctx._check(self._lib.ffs_stream_create(ctx._h, C.byref(h)))
        self._h = h
        self._batch_wants = (False, False)

    def host_buffer(self) -> np.ndarray:
        """The stream's pinned staging area as a (max_batch, H, W) array."""
        p, n = C.c_void_p(), C.c_size_t()
        self.ctx._check(self._lib.ffs_stream_host_buffer(self._h, C.byref(p), C.byref(n)))
        frames = self.ctx.max_batch * self.ctx.H * self.ctx.W * self.ctx.dtype.itemsize  # (+ slack for chunks)
        assert n.value >= frames, "the staging area was reserved smaller than max_batch frames (reserve_host)"
        buf = (C.c_uint8 * frames).from_address(p.value)
        return np.frombuffer(buf, dtype=self.ctx.dtype).reshape(self.ctx.max_batch, self.ctx.H, self.ctx.W)

    def reserve_host(self, nbytes: int):
        """Size the pinned staging area before its first use (ffs_stream_reserve_host), e.g. for chunks instead of frames."""
        self.ctx._check(self._lib.ffs_stream_reserve_host(self._h, nbytes))

    def host_bytes(self) -> np.ndarray:
        """The same staging area as bytes, including its slack (for compressed chunks placed in it)."""
        p, n = C.c_void_p(), C.c_size_t()
        self.ctx._check(self._lib.ffs_stream_host_buffer(self._h, C.byref(p), C.byref(n)))
        return np.frombuffer((C.c_uint8 * n.value).from_address(p.value), dtype=np.uint8)

    def _chunk_args(self, chunks):
        # (an array of any item size counts in bytes: raw Jungfrau frames are uint16 arrays; one that is not contiguous is copied)
        keep = [np.frombuffer(c, np.uint8) if not isinstance(c, np.ndarray) else np.ascontiguousarray(c) for c in chunks]
        ptrs = (C.c_void_p * len(keep))(*[k.ctypes.data for k in keep])
        sizes = (C.c_size_t * len(keep))(*[k.nbytes for k in keep])
        return keep, ptrs, sizes

    def submit_compressed(self, chunks, first_frame_id: int = 0):
        """chunks: bitshuffle-LZ4 chunks (bytes / uint8 arrays, 12-byte header included), one per frame."""
        self._keep, ptrs, sizes = self._chunk_args(chunks)
        self.ctx._check(self._lib.ffs_submit_compressed(self._h, ptrs, sizes, len(self._keep), first_frame_id))
        self._snapshot()

    def process_compressed(self, chunks, first_frame_id: int = 0):
        self.submit_compressed(chunks, first_frame_id)
        return self.wait()

    def submit_encoded(self, chunks, codec: int, first_frame_id: int = 0):
        """chunks: one per frame, in `codec` (CODEC_BSLZ4: as submit_compressed; CODEC_BYTE_OFFSET: a CBF binary section, the
        bytes behind its marker; CODEC_JUNGFRAU_RAW: H x W raw words as a uint16 array or W*H*2 bytes, little-endian, on a uint32
        context with a calibration set)."""
        self._keep, ptrs, sizes = self._chunk_args(chunks)
        self.ctx._check(self._lib.ffs_submit_encoded(self._h, codec, ptrs, sizes, len(self._keep), first_frame_id))
        self._snapshot()

    def process_encoded(self, chunks, codec: int, first_frame_id: int = 0):
        self.submit_encoded(chunks, codec, first_frame_id)
        return self.wait()

    def jungfrau_pedestal_fold(self, chunks, want_ms: bool = False):
        """ffs_stream_jungfrau_pedestal_fold: dark frames -- H x W raw words each, a uint16 array or W*H*2 bytes -- folded into the context's
        pedestal accumulators (Context.jungfrau_pedestal_begin first).  Synchronous.  Returns the fold launches' milliseconds with want_ms."""
        keep, ptrs, sizes = self._chunk_args(chunks)
        ms = C.c_float()
        self.ctx._check(self._lib.ffs_stream_jungfrau_pedestal_fold(self._h, ptrs, sizes, len(keep), C.byref(ms) if want_ms else None))
        return ms.value if want_ms else None

    def decode_only(self, chunks, iters: int = 1, want_frames: bool = True, codec: int = CODEC_BSLZ4):
        """GPU decode alone: (average ms per decode -- one launch, byte-offset: its three --, decoded frames or None)."""
        keep, ptrs, sizes = self._chunk_args(chunks)
        ms = C.c_float()
        out = np.empty((len(keep), self.ctx.H, self.ctx.W), self.ctx.dtype) if want_frames else None
        self.ctx._check(self._lib.ffs_decode_only_encoded(self._h, codec, ptrs, sizes, len(keep), iters, C.byref(ms),
                                                          out.ctypes.data_as(C.c_void_p) if want_frames else None))
        return ms.value, out

    def submit(self, frames: np.ndarray, first_frame_id: int = 0):
        f = np.ascontiguousarray(frames, dtype=self.ctx.dtype)
        if f.ndim == 2:
            f = f[None]
        assert f.shape[1:] == (self.ctx.H, self.ctx.W), f.shape
        self._keep = f
        self.ctx._check(self._lib.ffs_submit(self._h, f.ctypes.data_as(C.c_void_p), f.shape[0], first_frame_id))
        self._snapshot()

    def submit_device(self, dev_ptr: int, pitch_bytes: int, frame_stride_bytes: int, n_frames: int,
                      first_frame_id: int = 0):
        self.ctx._check(self._lib.ffs_submit_device(self._h, C.c_void_p(dev_ptr), pitch_bytes,
                                                    frame_stride_bytes, n_frames, first_frame_id))
        self._snapshot()

    def _snapshot(self):
        """The library takes the batch's parameters at submit: so does wait() for the outputs it hands back (the context's
        parameters may have changed for another stream's batch by then)."""
        self._batch_wants = (bool(self.ctx.params.want_reflections), bool(self.ctx.params.want_strong_list))

    def wait(self, copy: bool = True) -> list[FrameResult]:
        """copy=False: the box / reflection arrays are views of the library's buffers, valid until the
        next wait() on this stream (what a C caller gets); copy=True detaches them."""
        res = C.POINTER(_FrameResult)()
        n = C.c_uint32()
        self.ctx._check(self._lib.ffs_wait(self._h, C.byref(res), C.byref(n)))
        # two copies for the whole batch, then per-frame views
        bp, rp = C.c_void_p(), C.c_void_p()
        nb, nr = C.c_uint32(), C.c_uint32()
        self.ctx._check(self._lib.ffs_stream_batch_arrays(self._h, C.byref(bp), C.byref(nb),
                                                          C.byref(rp), C.byref(nr)))
        def arr(ptr, count, dt):
            if not count:
                return np.zeros(0, dt)
            buf = (C.c_uint8 * (count * dt.itemsize)).from_address(ptr.value)
            a = np.frombuffer(buf, dt)
            return a.copy() if copy else a
        boxes, refls = arr(bp, nb.value, BOX_DT), arr(rp, nr.value, REFL_DT)
        self.last_batch_boxes, self.last_batch_reflections = boxes, refls   # whole-batch arrays
        want_refl, want_list = self._batch_wants
        out = []
        W, H = self.ctx.W, self.ctx.H
        b0 = r0 = 0
        for i in range(n.value):
            r = res[i]
            ns = r.num_strong_pixels
            fr = FrameResult(
                frame_id=r.frame_id, num_strong_pixels=ns,
                num_strong_pixels_filtered=r.num_strong_pixels_filtered,
                n_components=r.n_components,
                boxes=boxes[b0:b0 + r.n_boxes],
                reflections=refls[r0:r0 + r.n_reflections] if want_refl else None,
                n_filtered_size=r.n_filtered_size, n_filtered_sep=r.n_filtered_sep)
            b0 += r.n_boxes
            r0 += r.n_reflections
            if want_list:
                if ns and r.strong_k:
                    fr.strong_k = np.ctypeslib.as_array(r.strong_k, (ns,)).copy()
                    fr.strong_intensity = np.ctypeslib.as_array(r.strong_intensity, (ns,)).copy()
                else:
                    fr.strong_k = np.zeros(0, np.uint32)
                    fr.strong_intensity = np.zeros(0, np.uint32)
            if r.strong_mask:
                fr.strong_mask = np.ctypeslib.as_array(r.strong_mask, (H, W)).copy()
            out.append(fr)
        return out

    def wait_counts(self):
        """ffs_wait() for callers that want the batch's totals only: (frames, boxes, strong pixels), read from the library's
        result array in one vectorised pass -- no Python object per frame (32 FrameResult objects cost the caller ~100 us,
        which the last wait of a timed run pays on the clock).  The boxes and reflections are in the library's host arrays
        (ffs_stream_batch_arrays) until the next wait on this stream."""
        res = C.POINTER(_FrameResult)()
        n = C.c_uint32()
        self.ctx._check(self._lib.ffs_wait(self._h, C.byref(res), C.byref(n)))
        if not n.value:
            return 0, 0, 0
        raw = np.frombuffer((C.c_uint8 * (n.value * C.sizeof(_FrameResult))).from_address(C.addressof(res.contents)), _FRAME_RESULT_DT)
        self.last_frame_counts = raw     # per-frame view (n_boxes, num_strong_pixels, ...), valid until the next wait on this stream
        return int(n.value), int(raw["n_boxes"].sum()), int(raw["num_strong_pixels"].sum())

    def process(self, frames: np.ndarray, first_frame_id: int = 0) -> list[FrameResult]:
        self.submit(frames, first_frame_id)
        return self.wait()

    def timings(self):
        t = (C.c_float * 5)()
        self.ctx._check(self._lib.ffs_stream_timings(self._h, t))
        return dict(zip(("h2d", "threshold", "ccl", "d2h", "total"), list(t)))

    PATH_BITS = {"wave_logs": 1, "frame_chain": 2, "bands": 4, "runs": 8, "grid_kernels": 16, "extended": 32, "window": 64, "radial": 128, "pixel_stats": 256,
                 "radial_threshold": 512, "radial_blur": 1024}

    def last_path(self):
        """ffs_stream_last_path: (set of the launches the last batch took, times ffs_wait ran it again)."""
        bits, reruns = C.c_uint32(), C.c_uint32()
        self.ctx._check(self._lib.ffs_stream_last_path(self._h, C.byref(bits), C.byref(reruns)))
        return {k for k, v in self.PATH_BITS.items() if bits.value & v}, reruns.value

    def bench_threshold(self, dev_ptr: int, pitch_bytes: int, frame_stride_bytes: int, n_frames: int,
                        iters: int):
        a, b = C.c_float(), C.c_float()
        self.ctx._check(self._lib.ffs_bench_threshold(self._h, C.c_void_p(dev_ptr), pitch_bytes,
                                                      frame_stride_bytes, n_frames, iters,
                                                      C.byref(a), C.byref(b)))
        return a.value, b.value

    def radial_profile(self, frame_in_batch: int):
        """ffs_stream_radial_profile: (count uint32, sum uint64, sum_sq uint64 modulo 2^64), n_bins entries each, of one frame of the
        last batch wait() returned -- copies.  FfsError when that batch was submitted without a bin map or the frame is out of range."""
        out = _RadialProfile()
        self.ctx._check(self._lib.ffs_stream_radial_profile(self._h, int(frame_in_batch), C.byref(out)))
        n = out.n_bins
        return (np.ctypeslib.as_array(out.count, (n,)).copy(), np.ctypeslib.as_array(out.sum, (n,)).copy(),
                np.ctypeslib.as_array(out.sum_sq, (n,)).copy())

    def radial_thresholds(self, frame_in_batch: int):
        """ffs_stream_radial_thresholds: what the radial-profile threshold decided per shell of one frame of the last batch wait() returned,
        as a structured array (RADIAL_SHELL_DT: n_pixels, n_overflow, q1, median, q3, cutoff, status, reserved) of n_bins records -- a
        copy.  FfsError when that batch ran another algorithm or the frame is out of range."""
        p, n = C.c_void_p(), C.c_uint32()
        self.ctx._check(self._lib.ffs_stream_radial_thresholds(self._h, int(frame_in_batch), C.byref(p), C.byref(n)))
        return np.frombuffer((C.c_uint8 * (n.value * RADIAL_SHELL_DT.itemsize)).from_address(p.value), RADIAL_SHELL_DT).copy()

    def spot_backgrounds(self, border: int = 3, copy: bool = True, want_ms: bool = False):
        """ffs_stream_spot_backgrounds: the constant background of the ring of `border` (1..16) pixels around every reflection of the last
        batch wait() returned, as a structured array (SPOT_BG_DT: n_pixels, n_overflow, q1, median, q3, n_inliers, inlier_sum, status,
        reserved, mean) in the order of last_batch_reflections.  Between wait() and the next submit on this stream; the batch needs
        want_reflections.  copy=False: a view of the library's buffer, valid until the next call or the next wait().  want_ms: returns
        (array, the kernel's ms from HIP events).  spot_intensities() turns it into background-subtracted intensities."""
        p, n, ms = C.c_void_p(), C.c_uint32(), C.c_float()
        self.ctx._check(self._lib.ffs_stream_spot_backgrounds(self._h, int(border), C.byref(p), C.byref(n), C.byref(ms)))
        if n.value:
            a = np.frombuffer((C.c_uint8 * (n.value * SPOT_BG_DT.itemsize)).from_address(p.value), SPOT_BG_DT)
            a = a.copy() if copy else a
        else:
            a = np.zeros(0, SPOT_BG_DT)
        return (a, ms.value) if want_ms else a

    def shoebox_fold(self, first_image: int, want_ms: bool = False):
        """ffs_stream_shoebox_fold: fold the frames of the last batch wait() returned into the context's job (Context.shoebox_begin); frame f
        of the batch is image first_image + f of the scan.  Between wait() and the next submit on this stream; synchronous.  Folding an
        image twice counts it twice.  Returns the kernel's milliseconds with want_ms (0 when no box met the images)."""
        ms = C.c_float()
        self.ctx._check(self._lib.ffs_stream_shoebox_fold(self._h, int(first_image), C.byref(ms) if want_ms else None))
        return ms.value if want_ms else None

    def spot_backgrounds_glm(self, border: int = 3, copy: bool = True, want_ms: bool = False):
        """ffs_stream_spot_backgrounds_glm: the same ring under the robust Poisson GLM (constant mean, Huber's c = 1.345), as a structured
        array (SPOT_BG_GLM_DT: n_pixels, n_overflow, median, n_iter, status, reserved, beta, mean) in the order of last_batch_reflections;
        the device computes the whole record.  Conditions, copy and want_ms as for spot_backgrounds(); the buffer is this call's own, so a
        view (copy=False) survives a spot_backgrounds() call on the same batch and the other way round.  spot_intensities_glm() turns it
        into background-subtracted intensities."""
        p, n, ms = C.c_void_p(), C.c_uint32(), C.c_float()
        self.ctx._check(self._lib.ffs_stream_spot_backgrounds_glm(self._h, int(border), C.byref(p), C.byref(n), C.byref(ms)))
        if n.value:
            a = np.frombuffer((C.c_uint8 * (n.value * SPOT_BG_GLM_DT.itemsize)).from_address(p.value), SPOT_BG_GLM_DT)
            a = a.copy() if copy else a
        else:
            a = np.zeros(0, SPOT_BG_GLM_DT)
        return (a, ms.value) if want_ms else a

    def bench_radial(self, dev_ptr: int, pitch_bytes: int, frame_stride_bytes: int, n_frames: int, iters: int) -> float:
        """ffs_bench_radial: average ms of one batch's radial profile (its two launches), alone on resident frames."""
        ms = C.c_float()
        self.ctx._check(self._lib.ffs_bench_radial(self._h, C.c_void_p(dev_ptr), pitch_bytes, frame_stride_bytes, n_frames, iters, C.byref(ms)))
        return ms.value

    def bench_pixel_stats(self, dev_ptr: int, pitch_bytes: int, frame_stride_bytes: int, n_frames: int, iters: int) -> float:
        """ffs_bench_pixel_stats: average ms of one batch's per-pixel statistics launch, alone on resident frames.  Uses the context's
        accumulators and leaves them undefined: FfsError while accumulation is on or a batch is in flight."""
        ms = C.c_float()
        self.ctx._check(self._lib.ffs_bench_pixel_stats(self._h, C.c_void_p(dev_ptr), pitch_bytes, frame_stride_bytes, n_frames, iters, C.byref(ms)))
        return ms.value

    def bench_hbm(self, iters: int = 5):
        """(read-only GB/s, 2:1 read/write GB/s) measured on this stream's buffers (ffs_bench_hbm)."""
        a, b = C.c_float(), C.c_float()
        self.ctx._check(self._lib.ffs_bench_hbm(self._h, iters, C.byref(a), C.byref(b)))
        return a.value, b.value

    def pack_spot_centres(self, out: np.ndarray, cap: int) -> int:
        """Rows (frame_id, x, y, z) of the last batch's reflections into `out` ((cap + 1, 4) float32,
        last row = count); the layout dist.pack_spots produces."""
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size >= (cap + 1) * 4
        n = C.c_uint32()
        self.ctx._check(self._lib.ffs_stream_spot_centres(self._h, out.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return n.value

    def debug_bitplane(self, frame_in_batch: int, which: int) -> np.ndarray:
        """0 = strong plane, 1 = extended first pass, 2 = extended eroded signal region (H x W uint8)."""
        out = np.empty((self.ctx.H, self.ctx.W), np.uint8)
        self.ctx._check(self._lib.ffs_stream_debug_bitplane(self._h, frame_in_batch, which,
                                                            out.ctypes.data_as(C.c_void_p)))
        return out

    def close(self):
        if self._h:
            self._lib.ffs_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _scan_geometry(geometry) -> _ScanGeometry:
    """ffs_scan_geometry from a mapping (or object) with d_matrix (9, row-major), pixel_size_mm (2), wavelength, s0 (3), rot_axis (3),
    osc_start_deg, osc_width_deg."""
    get = geometry.get if hasattr(geometry, "get") else (lambda k: getattr(geometry, k))
    g = _ScanGeometry()
    for name, n in (("d_matrix", 9), ("pixel_size_mm", 2), ("s0", 3), ("rot_axis", 3)):
        v = np.asarray(get(name), np.float64).reshape(-1)
        if v.size != n:
            raise ValueError(f"geometry {name} must have {n} entries, not {v.size}")
        setattr(g, name, (C.c_double * n)(*v))
    for name in ("wavelength", "osc_start_deg", "osc_width_deg"):
        setattr(g, name, float(get(name)))
    return g


def _crystal(a_matrix, centring) -> _Crystal:
    a = np.asarray(a_matrix, np.float64).reshape(-1)
    if a.size != 9:
        raise ValueError(f"a_matrix must have 9 entries, not {a.size}")
    code = CENTRINGS.get(centring, centring) if isinstance(centring, str) else centring
    if isinstance(code, str):
        raise ValueError(f"centring must be one of {sorted(CENTRINGS)}, not {centring!r}")
    x = _Crystal()
    x.a_matrix = (C.c_double * 9)(*a)
    x.centring = int(code)
    return x


def predict_scan_settings(geometry, a_matrix, n_images: int, centring="P") -> np.ndarray:
    """ffs_predict_scan_settings: the scan-point settings A_k = R(phi_k) A, k = 0 .. n_images, as Context.predict computes them, (n_images + 1,
    9) float64.  On the host: no context, no GPU.  This is the one place libm's cos and sin enter the prediction."""
    lib = load_library()
    g, x = _scan_geometry(geometry), _crystal(a_matrix, centring)
    out = np.zeros((max(int(n_images), 0) + 1, 9), np.float64)
    rc = lib.ffs_predict_scan_settings(C.byref(g), C.byref(x), int(n_images), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise FfsError(rc, lib.ffs_last_error(None).decode())
    return out


def _index_check(lib, rc):
    if rc != 0:
        raise FfsError(rc, lib.ffs_last_error(None).decode())


def index_rlp(geometry, xyz_px):
    """ffs_index_rlp: spot centres (n, 3) of (x_px, y_px, z in images from the scan's first) -> (rlp, s1, xyz_mm), each (n, 3) float64;
    xyz_mm is (x_mm, y_mm, angle in radians).  On the host: no context, no GPU."""
    lib = load_library()
    g = _scan_geometry(geometry)
    xyz = np.ascontiguousarray(np.asarray(xyz_px, np.float64).reshape(-1, 3))
    out = [np.zeros((len(xyz), 3), np.float64) for _ in range(3)]
    _index_check(lib, lib.ffs_index_rlp(C.byref(g), xyz.ctypes.data_as(C.c_void_p) if len(xyz) else None, len(xyz), *(o.ctypes.data_as(C.c_void_p) for o in out)))
    return tuple(out)


def index_defaults(rlp, max_cell: float, n_points: int = 256, dmin=None):
    """ffs_index_defaults: (dmin, b_iso); dmin None (or 0) = max(5 max_cell / n_points, the highest resolution among rlp)."""
    lib = load_library()
    r = np.ascontiguousarray(np.asarray(rlp, np.float64).reshape(-1, 3))
    d, b = C.c_double(0.0 if dmin is None else float(dmin)), C.c_double()
    _index_check(lib, lib.ffs_index_defaults(r.ctypes.data_as(C.c_void_p) if len(r) else None, len(r), float(max_cell), int(n_points), C.byref(d), C.byref(b)))
    return d.value, b.value


def index_twiddles(n_points: int) -> np.ndarray:
    """ffs_index_twiddles: the FFT's table, (n_points / 2, 2) float64 of (cos, -sin)(2 pi k / n_points)."""
    lib = load_library()
    out = np.zeros(max(int(n_points), 0) if int(n_points) <= 256 else 0, np.float64)
    _index_check(lib, lib.ffs_index_twiddles(int(n_points), out.ctypes.data_as(C.c_void_p)))
    return out.reshape(-1, 2)


def index_map(rlp, dmin: float, b_iso: float, n_points: int = 256):
    """ffs_index_map: per spot (cell, weight); cell INDEX_NOT_USED where the spot is not mapped."""
    lib = load_library()
    r = np.ascontiguousarray(np.asarray(rlp, np.float64).reshape(-1, 3))
    cell, weight = np.zeros(len(r), np.uint32), np.zeros(len(r), np.float64)
    _index_check(lib, lib.ffs_index_map(r.ctypes.data_as(C.c_void_p) if len(r) else None, len(r), float(dmin), float(b_iso), int(n_points),
                                        cell.ctypes.data_as(C.c_void_p), weight.ctypes.data_as(C.c_void_p)))
    return cell, weight


def index_basis_vectors(peaks, n_points: int, dmin: float, max_cell: float, peak_volume_cutoff: float = INDEX_PEAK_VOLUME_CUTOFF, min_cell: float = INDEX_MIN_CELL):
    """ffs_index_basis_vectors: Context.index_peaks' records -> the candidate basis vectors (INDEX_VECTOR_DT, Angstrom), sorted by volume."""
    lib = load_library()
    p = np.ascontiguousarray(np.asarray(peaks, INDEX_PEAK_DT))
    out = np.zeros(len(p), INDEX_VECTOR_DT)
    n = C.c_uint32()
    _index_check(lib, lib.ffs_index_basis_vectors(p.ctypes.data_as(C.c_void_p) if len(p) else None, len(p), int(n_points), float(dmin), float(peak_volume_cutoff),
                                                  float(min_cell), float(max_cell), out.ctypes.data_as(C.c_void_p) if len(p) else None, len(p), C.byref(n)))
    return out[:n.value]


def index_select(rlp, phi, dmin: float, osc_start_deg: float = 0.0) -> np.ndarray:
    """ffs_index_select: n bools, False where 1 / |rlp| <= dmin or phi in degrees > osc_start_deg + 360 (indexer.cc:266-276)."""
    lib = load_library()
    r = np.ascontiguousarray(np.asarray(rlp, np.float64).reshape(-1, 3))
    p = np.ascontiguousarray(np.asarray(phi, np.float64).reshape(-1))
    if len(p) != len(r):
        raise ValueError(f"phi must have one entry a spot: {len(p)} for {len(r)} spots")
    out = np.zeros(len(r), np.uint8)
    none = len(r) == 0
    _index_check(lib, lib.ffs_index_select(None if none else r.ctypes.data_as(C.c_void_p), None if none else p.ctypes.data_as(C.c_void_p), len(r), float(dmin),
                                           float(osc_start_deg), None if none else out.ctypes.data_as(C.c_void_p)))
    return out.astype(bool)


def index_settings(vectors, max_combinations: int = INDEX_MAX_COMBINATIONS) -> np.ndarray:
    """ffs_index_settings: candidate settings (INDEX_SETTING_DT: triple, axes, A = inverse(axes)) from basis vectors: INDEX_VECTOR_DT records or an
    (m, 3) array in Angstrom (combinations.cc without the Niggli reduction)."""
    lib = load_library()
    v = np.asarray(vectors)
    v = np.ascontiguousarray((v["v"] if v.dtype.names else v).astype(np.float64).reshape(-1, 3))
    n = C.c_uint32()
    rc = lib.ffs_index_settings(v.ctypes.data_as(C.c_void_p) if len(v) else None, len(v), int(max_combinations), None, 0, C.byref(n))
    if rc != -4:   # FFS_ERR_OVERFLOW: the count is in n
        _index_check(lib, rc)
    out = np.zeros(n.value, INDEX_SETTING_DT)
    _index_check(lib, lib.ffs_index_settings(v.ctypes.data_as(C.c_void_p) if len(v) else None, len(v), int(max_combinations),
                                             out.ctypes.data_as(C.c_void_p) if len(out) else None, len(out), C.byref(n)))
    return out


def index_absence_table() -> np.ndarray:
    """ffs_index_absence_table: the 111 absence tests (INDEX_ABSENCE_TEST_DT)."""
    lib = load_library()
    out = np.zeros(INDEX_ABSENCE_TESTS, INDEX_ABSENCE_TEST_DT)
    _index_check(lib, lib.ffs_index_absence_table(out.ctypes.data_as(C.c_void_p)))
    return out


def index_absence_detect(assignment, threshold: float = INDEX_ABSENCE_THRESHOLD) -> int:
    """ffs_index_absence_detect: the first absence test a record of INDEX_ASSIGNMENT_DT passes, or -1."""
    lib = load_library()
    rec = np.ascontiguousarray(np.asarray(assignment, INDEX_ASSIGNMENT_DT).reshape(1))
    t = C.c_int32()
    _index_check(lib, lib.ffs_index_absence_detect(rec.ctypes.data_as(C.c_void_p), float(threshold), C.byref(t)))
    return t.value


def index_reindex(A, test: int) -> np.ndarray:
    """ffs_index_reindex: the setting A (9) after the transform of absence test `test`."""
    lib = load_library()
    a = np.ascontiguousarray(np.asarray(A, np.float64).reshape(9))
    out = np.zeros(9, np.float64)
    _index_check(lib, lib.ffs_index_reindex(a.ctypes.data_as(C.c_void_p), int(test), out.ctypes.data_as(C.c_void_p)))
    return out


def shoeboxes_of(predictions: np.ndarray, skip_refused: bool = True) -> np.ndarray:
    """The table Context.shoebox_begin takes (SHOEBOX_DT) from Context.predict's records, in their order; skip_refused leaves out the records
    flagged PREDICT_BOX_REFUSED, which ffs_ctx_shoebox_begin would refuse."""
    p = np.asarray(predictions)
    if skip_refused:
        p = p[(p["flags"] & PREDICT_BOX_REFUSED) == 0]
    out = np.zeros(len(p), SHOEBOX_DT)
    for name in SHOEBOX_DT.names:
        out[name] = p[name]
    return out


def jungfrau_pedestal_planes(stats, min_frames: int = 1, max_rms: float = 0.0):
    """ffs_jungfrau_pedestal_planes: the accumulators of the dark-frame fold -- stats = (count, sum, sum_sq), each (3, ...) of one shape, or the
    tuple Context.jungfrau_pedestal returns (its n_frames is ignored) -- as (pedestal float32, rms float32, ok bool) of that shape: per stage
    and pixel the mean and the noise of the ADC in float64, rounded to float32, and ok = count >= min_frames and (max_rms == 0 or rms <=
    max_rms).  On the host: no context, no GPU.  FfsError: min_frames 0, a negative or non-finite max_rms."""
    lib = load_library()
    if len(stats) == 4:
        stats = stats[1:]
    count = np.ascontiguousarray(stats[0], np.uint32)
    total = np.ascontiguousarray(stats[1], np.uint64)
    total_sq = np.ascontiguousarray(stats[2], np.uint64)
    if count.ndim < 1 or count.shape[0] != 3 or total.shape != count.shape or total_sq.shape != count.shape:
        raise ValueError(f"count, sum and sum_sq must share one shape (3, ...), not {count.shape}, {total.shape}, {total_sq.shape}")
    n_px = count[0].size
    st = _JungfrauPedestalStats()
    pedestal, rms, ok = np.zeros(count.shape, np.float32), np.zeros(count.shape, np.float32), np.zeros(count.shape, np.uint8)
    outs = [(C.c_void_p * 3)() for _ in range(3)]
    for s in range(3):
        st.count[s], st.sum[s], st.sum_sq[s] = count[s].ctypes.data, total[s].ctypes.data, total_sq[s].ctypes.data
        for o, a in zip(outs, (pedestal, rms, ok)):
            o[s] = a[s].ctypes.data
    rc = lib.ffs_jungfrau_pedestal_planes(C.byref(st), n_px, min_frames, max_rms, *outs)
    if rc != 0:
        raise FfsError(rc, lib.ffs_last_error(None).decode())
    return pedestal, rms, ok.astype(bool)


def spot_intensities(reflections: np.ndarray, backgrounds: np.ndarray):
    """Background-subtracted intensities of a batch's reflections (REFL_DT) from their backgrounds (Stream.spot_backgrounds, same order):
    intensity = sum_intensity - num_pixels * mean, and its variance under Poisson statistics, sum_intensity + num_pixels^2 * mean /
    n_inliers (the counts' own variance plus that of the estimated mean over the spot's pixels).  Both float64, NaN where status != 0."""
    assert len(reflections) == len(backgrounds)
    ok = backgrounds["status"] == SPOT_BG_OK
    s = reflections["sum_intensity"].astype(np.float64)
    k = reflections["num_pixels"].astype(np.float64)
    mean = backgrounds["mean"].astype(np.float64)
    ni = np.where(ok, backgrounds["n_inliers"], 1).astype(np.float64)
    intensity = np.where(ok, s - k * mean, np.nan)
    variance = np.where(ok, s + k * k * mean / ni, np.nan)
    return intensity, variance


def spot_intensities_glm(reflections: np.ndarray, backgrounds: np.ndarray):
    """The same from the GLM backgrounds (Stream.spot_backgrounds_glm, same order): intensity = sum_intensity - num_pixels * mean; the
    model puts all n_pixels ring pixels at the fitted mean, so the mean's variance is mean / n_pixels and the intensity's is sum_intensity
    + num_pixels^2 * mean / n_pixels.  Both float64, NaN where status != 0."""
    assert len(reflections) == len(backgrounds)
    ok = backgrounds["status"] == SPOT_BG_OK
    s = reflections["sum_intensity"].astype(np.float64)
    k = reflections["num_pixels"].astype(np.float64)
    mean = backgrounds["mean"].astype(np.float64)
    n = np.where(ok, backgrounds["n_pixels"], 1).astype(np.float64)
    intensity = np.where(ok, s - k * mean, np.nan)
    variance = np.where(ok, s + k * k * mean / n, np.nan)
    return intensity, variance


def bench_pipeline(streams, dev_ptr: int, pitch_bytes: int, frame_stride_bytes: int, n_frames: int, steps: int,
                   first_frame_id: int = 0):
    """ffs_bench_pipeline: `steps` batches through `streams` (one context), natively; -> (boxes, strong pixels) summed."""
    arr = (C.c_void_p * len(streams))(*[s._h for s in streams])
    nb, ns = C.c_uint64(), C.c_uint64()
    streams[0].ctx._check(load_library().ffs_bench_pipeline(arr, len(streams), C.c_void_p(dev_ptr), pitch_bytes, frame_stride_bytes,
                                                             n_frames, steps, first_frame_id, C.byref(nb), C.byref(ns)))
    return nb.value, ns.value


def device_numa_node(device: int = 0) -> int:
    return load_library().ffs_device_numa_node(device)


def multi_init(devices, transport=None) -> str:
    """ffs_multi_init: prepare the exchange between the contexts of several GPUs; returns the transport in use."""
    lib = load_library()
    arr = (C.c_int * len(devices))(*devices)
    rc = lib.ffs_multi_init(arr, len(devices), transport.encode() if transport else None)
    if rc != 0:
        raise FfsError(rc, lib.ffs_last_error(None).decode())
    return lib.ffs_multi_transport().decode()


def multi_gather_rows(streams, root: int = 0, cap: int = 1 << 20) -> np.ndarray:
    """ffs_multi_gather_rows: the centre rows of the streams' last batches through RCCL (counts by all-gather, rows by send / recv to
    the root's device, one copy to the host) -> (n, 4) float32, lane 0 = frame id bits, in the order of `streams`."""
    lib = load_library()
    lib.ffs_multi_gather_rows.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    arr = (C.c_void_p * len(streams))(*[s._h for s in streams])
    out = np.empty((cap, 4), np.float32)
    n = C.c_uint32()
    streams[root].ctx._check(lib.ffs_multi_gather_rows(arr, len(streams), root, out.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
    return out[:n.value].copy()


class Stack3D:
    """Rotation-sweep accumulator -> 3D connected components (ffs_stack3d_*)."""

    def __init__(self, ctx: Context, max_total_strong: int = 0):
        self.ctx = ctx
        self._lib = ctx._lib
        h = C.c_void_p()
        ctx._check(self._lib.ffs_stack3d_create(ctx._h, max_total_strong, C.byref(h)))
        self._h = h

    def add_batch(self, stream: Stream):
        self.ctx._check(self._lib.ffs_stack3d_add_batch(self._h, stream._h))

    def add_slice(self, frame_id: int, k: np.ndarray, intensity: np.ndarray):
        k = np.ascontiguousarray(k, dtype=np.uint32)
        it = np.ascontiguousarray(intensity, dtype=np.uint32)
        assert k.shape == it.shape
        self.ctx._check(self._lib.ffs_stack3d_add_slice(self._h, frame_id, k.ctypes.data_as(C.c_void_p),
                                                        it.ctypes.data_as(C.c_void_p), len(k)))

    def finish(self):
        """-> (reflections REFL_DT, n_calculated, n_filtered_size, n_filtered_sep)"""
        r = C.POINTER(_Refl)()
        n, nc, fs, fp = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        self.ctx._check(self._lib.ffs_stack3d_finish(self._h, C.byref(r), C.byref(n), C.byref(nc),
                                                     C.byref(fs), C.byref(fp)))
        return _copy_array(r, n.value, _Refl, REFL_DT), nc.value, fs.value, fp.value

    def last_finish_ms(self) -> float:
        ms = C.c_float()
        self.ctx._check(self._lib.ffs_stack3d_last_finish_ms(self._h, C.byref(ms)))
        return ms.value

    def signals(self):
        """Per-signal view of the last finish(): dict of x, y, z, intensity, reflection (-1 = filtered)."""
        px, py, pi = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
        pz, pr = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        n = C.c_uint64()
        self.ctx._check(self._lib.ffs_stack3d_signals(self._h, C.byref(px), C.byref(py), C.byref(pz), C.byref(pi),
                                                      C.byref(pr), C.byref(n)))
        def arr(p, dt):
            return np.ctypeslib.as_array(p, (n.value,)).astype(dt) if n.value else np.zeros(0, dt)
        return {"x": arr(px, np.uint32), "y": arr(py, np.uint32), "z": arr(pz, np.int32),
                "intensity": arr(pi, np.uint32), "reflection": arr(pr, np.int32)}

    def close(self):
        if self._h:
            self._lib.ffs_stack3d_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
