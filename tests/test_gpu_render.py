"""The kernels of csrc/render.hip through p3d_debug_render_u8 (every device buffer between guards) against tests/render_ref.py,
tolerance 0 everywhere.  Shapes are the smallest at which each path can go wrong: under one 16-byte word and under one wave
(3 x 5), maps and buffers off the boundary, aligned alike and unalike (7 x 19, five maps, four offsets: 133 pixels a map shift
every next map), whole words (16 x 16), a halo larger than the map (2 x 3 at t = 4), clipping at all four borders (W = 17 and
H = 17, t = 1 .. 4), at least three blocks in every direction the plan tiles with the level set's edge along and across every seam,
one frame at 1080 x 1920, and a map of more tiles than the grid holds in x.  Each runs with a random, an opaque and a transparent table, with and without frames, with the
contour off and on."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import render_ref as R        # noqa: E402

CBGR = (250, 3, 77)           # (B, G, R) of the contour in the replay; the op takes (R, G, B)


def run(sal, frames, table, L=0, t=1, offset=0):
    from sap3d_tensorflow_amd import dataflow
    return dataflow.render_overlay(sal, frames, table, contour=L or None, thickness=t, contour_color=CBGR[::-1], offset=offset)


def check(sal, frames, L=128, ts=(1,), offset=0, what=""):
    """Every table, with and without frames, the contour off and on at every t of ts."""
    tabs = R.tables()
    for name in ("random", "opaque", "transparent"):
        for f in (frames, None):
            got = run(sal, f, tabs[name], 0, 1, offset)
            assert got.dtype == np.uint8 and got.shape == sal.shape + (3,)
            assert np.array_equal(got, R.render(sal, f, tabs[name])), (what, name, f is None, "no contour", offset)
            for t in ts:
                got = run(sal, f, tabs[name], L, t, offset)
                want = R.render(sal, f, tabs[name], L, t, CBGR)
                bad = np.argwhere(got != want)
                assert bad.size == 0, (what, name, f is None, "t", t, "offset", offset, len(bad), bad[:4])
    for t in ts:
        assert R.contour_mask(sal, L, t).any(), (what, t)                # the contour cases have contour pixels
    # the two ends of the opacity: the colour itself, the frame itself
    assert np.array_equal(run(sal, frames, tabs["transparent"], 0, 1, offset), frames)
    assert np.array_equal(run(sal, frames, tabs["opaque"], 0, 1, offset), run(sal, None, tabs["opaque"], 0, 1, offset))


def test_under_one_word_and_under_one_wave():
    sal = R.blob(1, 3, 5)
    check(sal, R.frames_for(sal), ts=(1, 2), what="3x5")
    m = R.contour_mask(sal[0], 128, 1)
    print("3x5: %d of %d pixels at or above 128 on the contour" % (m.sum(), (sal[0] >= 128).sum()))


@pytest.mark.parametrize("offset", [0, 1, 5, 15, 8])
def test_maps_off_the_16_byte_boundary(offset):
    """7 x 19 = 133 pixels a map: map m's saliency starts 5 m bytes, its frame and out 15 m bytes further past a boundary.
    Offsets 0 and 8 leave the three buffers aligned alike (whole words behind a head), the others unalike (every pixel single)."""
    sal = R.blob(5, 7, 19)
    check(sal, R.frames_for(sal), ts=(1, 3), offset=offset, what="7x19")
    m = R.contour_mask(sal[0], 128, 1)
    print("7x19: %d of %d pixels at or above 128 on the contour" % (m.sum(), (sal[0] >= 128).sum()))
    assert (sal >= 128).sum() > R.contour_mask(sal, 128, 1).sum() > 0      # some of the level set stays uncontoured


def test_whole_words():
    sal = R.blob(2, 16, 16)
    check(sal, R.frames_for(sal), ts=(1, 4), what="16x16")


def test_halo_larger_than_the_map():
    sal = np.array([[[200, 10, 130], [128, 127, 255]]], np.uint8)
    check(sal, R.frames_for(sal), ts=(4,), what="2x3")
    every = R.contour_mask(sal, 128, 4)
    assert np.array_equal(every, sal >= 128)               # every pixel of the level set sees a pixel below it


@pytest.mark.parametrize("shape", [(9, 17), (17, 9), (17, 17)])
def test_clipping_at_all_four_borders(shape):
    sal = R.blob(2, *shape)
    sal[1] = 255 - sal[1]                                  # the level set runs into all four borders
    assert (sal[1][0] >= 128).any() and (sal[1][-1] >= 128).any() and (sal[1][:, 0] >= 128).any() and (sal[1][:, -1] >= 128).any()
    check(sal, R.frames_for(sal), ts=(1, 2, 3, 4), what="%dx%d" % shape)


def _seamed(H, W, rows, cols, chunk, L, t):
    """A map whose level set's edge runs along and across every block seam, with one-pixel holes below L on a seam and t from it."""
    sal = R.blob(1, H, W, seed=7)[0]
    sal = np.minimum(sal, L - 1).astype(np.uint8)
    if cols:
        ys, xs = list(range(rows, H, rows)), list(range(cols, W, cols))
        for k, y in enumerate(ys):                         # bands whose edges are the seam rows themselves, and one across
            sal[y - (k % 2):y + 5, :] = 255
        for k, x in enumerate(xs):
            sal[:, x - (k % 2):x + 7] = 255
        holes = [(ys[0], xs[0]), (ys[0] + t, xs[0] + t), (ys[1] - 1, xs[1] - 1), (ys[0], xs[-1] + t), (ys[-1] - t, xs[0])]
    else:
        seams = list(range(chunk, H * W, chunk))
        flat = sal.reshape(-1)
        for k, p in enumerate(seams):
            flat[p - (k % 2) * 3:p + 29] = 255            # a run across the seam: its pixels' rows above and below stay low
        sal = flat.reshape(H, W)
        sal[:, W // 2:W // 2 + 9] = 255                    # a band that crosses every block
        holes = [divmod(seams[0], W), divmod(seams[0] + t, W), divmod(seams[-1] - 1, W)]
    for (y, x) in holes:
        sal[y, x] = 0
    return sal[None], holes


@pytest.mark.parametrize("t", [0, 1, 4])
def test_three_blocks_in_every_direction_with_the_edge_on_every_seam(t):
    from sap3d_tensorflow_amd import dataflow
    rows, cols, pixels = dataflow.render_plan(64, 64, thickness=t)
    if cols:
        H, W = 3 * rows + 5, 3 * cols + 11
    else:
        W = 251
        H = (3 * pixels + W - 1) // W + 2
    assert H * W <= 2 ** 20
    assert dataflow.render_plan(H, W, thickness=t) == (rows, cols, pixels)
    L = 128
    sal, holes = _seamed(H, W, rows, cols, pixels, L, max(t, 1))
    frames = R.frames_for(sal)
    check(sal, frames, L, ts=(max(t, 1),), what="seams of %r" % ((rows, cols, pixels),))
    if t == 0:                                             # the plain launch's flat runs once more, the buffers aligned unalike
        for f in (frames, None):
            assert np.array_equal(run(sal, f, R.tables()["random"], 0, 1, 5), R.render(sal, f, R.tables()["random"]))
    if t:
        a = sal[0] >= L
        m = R.contour_mask(sal[0], L, t)
        for (y, x) in holes:                               # a hole draws its ring, across the seam it sits on
            win = (slice(max(0, y - t), y + t + 1), slice(max(0, x - t), x + t + 1))
            assert not a[y, x] and a[win].sum() >= 2 * t and np.array_equal(m[win], a[win]), (y, x)
        assert m.any() and (a & ~m).any()                  # some pixels at or above L stay uncontoured


def test_more_blocks_than_the_grid_holds_in_x():
    """A map one pixel wide is one tile every 16 rows: 2^20 + 40 rows are 65539 tiles, three more than the launch puts into the
    grid's x, so the last three come from the second layer of z, whose other blocks must do nothing.  (At the limit of 2^28 rows
    there are 2^24 tiles, more threads than a grid dimension takes.)"""
    H = 2 ** 20 + 40
    sal = np.full((1, H, 1), 200, np.uint8)
    sal[0, ::4099] = 90                                    # holes down the map ...
    sal[0, 2 ** 20 - 3:2 ** 20 + 2] = 60                   # ... and one across the fold, rows below it in z = 1
    sal[0, -1] = 10
    frames = R.frames_for(sal)
    tab = R.tables()["random"]
    for f in (frames, None):
        for t in (1, 4):
            got = run(sal, f, tab, 128, t, 3)
            bad = np.argwhere(got != R.render(sal, f, tab, 128, t, CBGR))
            assert bad.size == 0, (f is None, t, len(bad), bad[:4])
    m = R.contour_mask(sal[0], 128, 4)
    assert m[2 ** 20 + 2:2 ** 20 + 6].all() and m[-5:-1].all() and not m[2 ** 20 + 6:2 ** 20 + 30].any()


def test_one_frame_at_1080_by_1920():
    sal = R.blob(1, 1080, 1920)
    frames = R.frames_for(sal)
    check(sal, frames, ts=(1,), what="1080x1920")
    assert np.array_equal(run(sal, frames, R.tables()["random"], 128, 4), R.render(sal, frames, R.tables()["random"], 128, 4, CBGR))
    m = R.contour_mask(sal[0], 128, 1)
    assert m.any() and ((sal[0] >= 128) & ~m).any()


def test_op_level_entry_equals_the_hook():
    """p3d_render_u8 (buffers carved from the stream's scratch) returns the hook's bytes; [H, W] maps come back as [H, W, 3]."""
    from sap3d_tensorflow_amd import dataflow
    sal = R.blob(3, 37, 53)
    frames = R.frames_for(sal)
    t = dataflow.render_table("jet", 0.6, "ramp", gate=30)
    for f in (frames, None):
        got = dataflow.render_overlay(sal, f, t, contour=100, thickness=2, contour_color=(9, 8, 7))
        assert np.array_equal(got, R.render(sal, f, t, 100, 2, (7, 8, 9)))
    one = dataflow.render_overlay(sal[0], frames[0], t)
    assert one.shape == (37, 53, 3) and np.array_equal(one, R.render(sal[0], frames[0], t))


def test_refusals():
    from sap3d_tensorflow_amd import P3dError, dataflow
    sal = R.blob(1, 3, 5)
    t = R.tables()["random"]
    for kw in (dict(contour=256), dict(contour=-1), dict(contour=10, thickness=0), dict(contour=10, thickness=5), dict(offset=16)):
        with pytest.raises(P3dError):
            dataflow.render_overlay(sal, None, t, **kw)
