"""GPU: the tables of tests/shoebox_seams.py through ffs_ctx_shoebox_begin, ffs_stream_shoebox_fold, ffs_ctx_get_shoebox_sums and
ffs_ctx_get_shoebox_histogram, bit for bit against tests/shoebox_oracle.py under both background models: foreground edges on the seams
between a wave's strips of 63 pixel columns, on a box's last corner column and its first and last corner row, one-pixel boxes, boxes of
1024 columns and rows and boxes wholly in the pad, corners whose decision is an exact tie, and launch lists of 1, 2, 3 and 5 boxes that
leave waves of the last workgroup without a box.  16-bit and 32-bit pixels, both algorithms, the mask of shoebox_cases.mask.
tests/test_shoebox_seams.py asserts without a GPU that the tables contain all this."""
import numpy as np
import pytest

import shoebox_oracle as O
import shoebox_seams as S
from test_gpu_shoebox import assert_matches, fold_batches, open_job

pytestmark = pytest.mark.gpu


def ids(jobs):
    return [j["name"] for j in jobs]


SEAM_JOBS = S.seam_and_tie_jobs()


@pytest.mark.parametrize("j", SEAM_JOBS, ids=ids(SEAM_JOBS))
def test_seams_and_ties_as_one_batch_and_image_by_image(ffs, j):
    n = j["n_images"]
    for batches in ([(0, n)], [(i, i + 1) for i in range(n)]):
        ctx = open_job(ffs, j, max_batch=n)
        fold_batches(ctx.stream(), j, batches)
        assert_matches(ctx, S.acc_of(j), f"{j['name']}, batches {batches}")
        ctx.shoebox_end()


LARGEST_JOBS = [S.largest_job(d, a) for d, a in S.LARGEST_COMBOS]


@pytest.mark.parametrize("j", LARGEST_JOBS, ids=ids(LARGEST_JOBS))
def test_the_largest_boxes_and_the_boxes_in_the_pad(ffs, j):
    ctx = open_job(ffs, j, max_batch=4)
    fold_batches(ctx.stream(), j, [(0, 1), (1, 3)])
    assert_matches(ctx, S.acc_of(j), j["name"])
    got = ctx.shoebox_sums()
    for i in j["in_pad"]:
        assert (got["flags"][i], got["fg_count"][i], got["n_background"][i]) == (O.FG_INVALID, 0, 0) and not ctx.shoebox_histogram(i).any()
    ctx.shoebox_end()
    # one column, one row more: refused, and no job is opened
    for box, word in S.refused_boxes(j["g"]):
        with pytest.raises(ffs.FfsError) as e:
            ctx.shoebox_begin(j["g"], np.array([j["boxes"][0], box], O.BOX_DT), j["algorithm"], delta_b=j["delta_b"], delta_m=j["delta_m"])
        assert e.value.code == -1 and "shoebox 1 " in str(e.value) and word in str(e.value), str(e.value)
    with pytest.raises(ffs.FfsError):
        ctx.shoebox_sums()


def test_a_box_of_1024_by_1024_over_two_images(ffs):
    j = S.square_job(*S.SQUARE_COMBO)
    ctx = open_job(ffs, j, max_batch=2)
    fold_batches(ctx.stream(), j, [(0, 2)])
    assert_matches(ctx, S.acc_of(j), j["name"])
    ctx.shoebox_end()


SHORT_JOBS = S.short_jobs()


@pytest.mark.parametrize("j", SHORT_JOBS, ids=ids(SHORT_JOBS))
def test_lists_shorter_than_a_workgroup(ffs, j):
    ctx = open_job(ffs, j)
    fold_batches(ctx.stream(), j, S.SHORT_BATCHES)   # batches of 1, 3 and 8
    assert_matches(ctx, S.acc_of(j), j["name"])
    ctx.shoebox_end()
