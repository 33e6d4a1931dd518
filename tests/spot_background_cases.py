"""Planted 37 x 29 frames for the per-spot background: each is built so that the spot finder returns a known bounding box and the ring
around it ends in a known status.  Shared by the CPU test (the committed oracle must find the planted boxes) and the GPU test."""
import numpy as np

import spot_background_oracle as B

W, H = 37, 29


def _constant_with_outliers(n_outliers):
    """Background 2, a 3 x 3 block of 1000 at x 17..19, y 13..15, and n_outliers (<= 19) of the 72 ring pixels of border 3 at 300: sixteen on
    the ring's outer rim, two pixels apart, and up to three one pixel further in, none of them touching the block or forming a spot of their own."""
    f = np.full((H, W), 2, np.uint16)
    f[13:16, 17:20] = 1000
    rim = [(x, 10) for x in range(14, 23, 2)] + [(x, 18) for x in range(14, 23, 2)] + [(14, y) for y in range(12, 17, 2)] + [(22, y) for y in range(12, 17, 2)]
    spots = rim + [(18, 11), (18, 17), (15, 14)]
    assert len(rim) == 16 and n_outliers <= len(spots)
    for x, y in spots[:n_outliers]:
        f[y, x] = 300
    return f


def cases():
    """name -> dict(frame, mask (None: all valid), box (x_min, x_max, y_min, y_max), status, and for some the whole record)."""
    rng = np.random.default_rng(2024)
    out = {}
    box = (17, 19, 13, 15)
    out["tie_18_of_72"] = dict(frame=_constant_with_outliers(18), mask=None, box=box, status=B.OK, only=True,
                               record=dict(n_pixels=72, n_overflow=18, q1=2, median=2, q3=2, n_inliers=54, inlier_sum=108, status=B.OK))
    out["tie_19_of_72"] = dict(frame=_constant_with_outliers(19), mask=None, box=box, status=B.OVERFLOW, only=True,
                               record=dict(n_pixels=72, n_overflow=19, q1=-1, median=-1, q3=-1, n_inliers=0, inlier_sum=0, status=B.OVERFLOW))
    f = np.concatenate([rng.poisson(5.0, (H, 19)), rng.poisson(200.0, (H, W - 19))], axis=1).astype(np.uint16)
    f[13:16, 17:20] = 5000      # on the seam between x = 18 and x = 19
    out["two_levels"] = dict(frame=f, mask=None, box=box, status=B.RANGE)
    f = rng.poisson(300.0, (H, W)).astype(np.uint16)
    f[13:16, 17:20] = 20000
    out["above_the_bins"] = dict(frame=f, mask=None, box=box, status=B.OVERFLOW)
    f = rng.poisson(3.0, (H, W)).astype(np.uint16)
    m = np.zeros((H, W), np.uint8)
    m[12:17, 16:21] = 1
    f[12:17, 16:21] = 1000
    f[13:16, 17:20] = 3
    f[12, 18] = 1200            # the peak at the middle of an edge: two pixels from the centroid, which the peak pulls towards itself
    out["island_in_the_mask"] = dict(frame=f, mask=m, box=(16, 20, 12, 16), status=B.NO_PIXELS, only=True,
                                     record=dict(n_pixels=0, n_overflow=0, q1=-1, median=-1, q3=-1, n_inliers=0, inlier_sum=0, status=B.NO_PIXELS))
    f = np.full((H, W), 2, np.uint16)
    f[14, :] = 500
    f[14, 18] = 600
    out["row_across_the_frame"] = dict(frame=f, mask=None, box=(0, W - 1, 14, 14), status=B.OK, only=True,
                                       record=dict(n_pixels=6 * W, n_overflow=0, q1=2, median=2, q3=2, n_inliers=6 * W, inlier_sum=12 * W, status=B.OK))
    f = np.full((H, W), 2, np.uint16)
    f[0:2, 0:2] = 500
    out["corner"] = dict(frame=f, mask=None, box=(0, 1, 0, 1), status=B.OK, only=True,
                         record=dict(n_pixels=21, n_overflow=0, q1=2, median=2, q3=2, n_inliers=21, inlier_sum=42, status=B.OK))
    f = rng.poisson(3.0, (H, W)).astype(np.uint16)
    f[13:16, 10:13] = 800
    f[13:16, 15:18] = 900
    out["neighbours"] = dict(frame=f, mask=None, box=(10, 12, 13, 15), box2=(15, 17, 13, 15), status=B.OK)
    return out
