"""ffs_amd -- Python mirror of libffs_hip.so's C ABI (include/ffs_hip.h).

The library is the product; this package is the thin host-side binding used by
tests/, bench.py and __graft_entry__.py.  It fails loudly when the HIP library is
missing -- there is no CPU fallback.
"""
from . import synth  # noqa: F401
from .api import (Context, FrameResult, Params, Stack3D, Stream, device_count,  # noqa: F401
                  device_name, lib_path, load_library, FfsError, BOX_DT, REFL_DT,
                  ALGO_DISPERSION, ALGO_DISPERSION_EXTENDED, CODEC_BSLZ4, CODEC_BYTE_OFFSET, CODEC_JUNGFRAU_RAW, MAX_VALID_CENTRE, MAX_VALID_WINDOW, multi_init,
                  SPOT_BG_DT, spot_intensities, SPOT_BG_GLM_DT, spot_intensities_glm, jungfrau_pedestal_planes, ALGO_RADIAL_PROFILE, RADIAL_SHELL_DT,
                  RADIAL_BLUR_NONE, RADIAL_BLUR_NARROW, RADIAL_BLUR_WIDE,
                  SHOEBOX_DT, SHOEBOX_SUM_DT, SHOEBOX_ELLIPSOID, SHOEBOX_DIALS, SHOEBOX_FG_INVALID,
                  PREDICTION_DT, CENTRINGS, PREDICT_ENTERING, PREDICT_CORNER_LOST, PREDICT_ZETA_SMALL, PREDICT_BOX_REFUSED,
                  predict_scan_settings, shoeboxes_of,
                  INDEX_PEAK_DT, INDEX_VECTOR_DT, INDEX_NOT_USED, INDEX_LAUNCH_SPANS, INDEX_RMSD_CUTOFF, INDEX_PEAK_VOLUME_CUTOFF, INDEX_MIN_CELL,
                  index_rlp, index_defaults, index_twiddles, index_map, index_basis_vectors,
                  INDEX_ABSENCE_TESTS, INDEX_ASSIGN_SINGULAR, INDEX_ASSIGNMENT_DT, INDEX_ABSENCE_TEST_DT, INDEX_SETTING_DT, INDEX_ASSIGN_LAUNCH_SPANS,
                  INDEX_ASSIGN_TOLERANCE, INDEX_ABSENCE_THRESHOLD, INDEX_MAX_COMBINATIONS,
                  index_select, index_settings, index_absence_table, index_absence_detect, index_reindex)
