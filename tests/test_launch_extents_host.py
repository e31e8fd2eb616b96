"""The launch-extent arithmetic of the library (DESIGN.md "Launch extents"), no device.

A dispatch packet holds a grid axis in WORK-ITEMS in 32 bits, so one launch is legal while blocks x threads <= 2^32 - 1 (and the
grid's first axis holds at most 2^31 - 1 workgroups).  Every launcher folds its leading slices into grid.x and goes clip range by clip
range, `clips_per_launch(tiles_per_clip, threads)` clips at a time; smx_debug_clips_per_launch is that function.  The values here are
ones no GPU test can afford: the largest count that fits, and that one more does not."""
import pytest

from soundml_amd._lib import lib

ITEMS = 2 ** 32 - 1          # work-items of one launch along x
BLOCKS = 2 ** 31 - 1         # workgroups of one launch along x

TILES = [1, 3, 2 ** 24 - 1, 2 ** 24, 2 ** 31]
THREADS = [64, 256, 512, 1024]


def clips(tiles_per_clip, threads):
    return int(lib.smx_debug_clips_per_launch(tiles_per_clip, threads))


@pytest.mark.parametrize("threads,most", [(64, 67108863), (256, 16777215), (1024, 4194303)])
def test_the_largest_grid_of_a_workgroup_size(threads, most):
    """the table of the issue and of DESIGN.md: a clip of one workgroup"""
    assert clips(1, threads) == most == ITEMS // threads
    assert most * threads <= ITEMS < (most + 1) * threads


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("tiles", TILES)
def test_the_count_fits_and_one_more_clip_does_not(tiles, threads):
    n = clips(tiles, threads)
    assert n >= 0
    assert n * tiles * threads <= ITEMS < (n + 1) * tiles * threads
    assert n * tiles <= BLOCKS
    assert n == ITEMS // (tiles * threads)                       # at these widths the work-item bound is the tighter one
    assert (n == 0) == (tiles * threads > ITEMS)                 # 0: a single clip does not fit, the launcher refuses


def test_a_single_clip_that_does_not_fit():
    assert clips(2 ** 24, 256) == 0 and clips(2 ** 24 - 1, 256) == 1      # one workgroup of 256 per frame: 16 777 215 frames
    assert clips(2 ** 22, 1024) == 0 and clips(2 ** 22 - 1, 1024) == 1
    assert clips(2 ** 31, 64) == 0 and clips(2 ** 62, 64) == 0


def test_narrow_workgroups_meet_the_workgroup_bound():
    """below 3 threads a workgroup the 2^31 - 1 workgroups bind first"""
    assert clips(1, 1) == BLOCKS and clips(1, 2) == BLOCKS and clips(1, 3) == ITEMS // 3
    assert clips(2, 1) == BLOCKS // 2


def test_degenerate_arguments_hold_nothing():
    assert clips(0, 256) == 0 and clips(-1, 256) == 0 and clips(1, 0) == 0 and clips(1, -64) == 0
