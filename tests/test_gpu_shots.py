"""The kernels of csrc/shots.hip through p3d_debug_shot_distances_u8 (every device buffer, the scratch included, between guards) and
p3d_shot_cuts against tests/shots_ref.py, tolerance 0.  Shapes are the smallest at which each path can go wrong: one pixel, rows
shorter than a 16-byte word, rows whose channel phase changes from row to row (3 W = 99), rows of more than 64 words (W = 480: 90),
several blocks a frame, every corner of the grid, more frames than a chunk of tables holds, and two frames at the 32-bit headroom of
a 1080 x 1920 source."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import shots_ref as S          # noqa: E402

SHAPES = [(1, 1), (5, 7), (9, 33), (33, 70), (112, 112), (270, 480)]
GRIDS = [(1, 1), (1, 4), (4, 1), (4, 4), (2, 3)]


def run(frames, grid, offset=0, ballot=0):
    from sap3d_tensorflow_amd import dataflow
    return dataflow.shot_distances(frames, grid, offset=offset, ballot=ballot)


def grid_in(grid, H, W):
    return min(grid[0], H), min(grid[1], W)


def check(frames, grid, offset=0, what=""):
    want = S.distances(frames, *grid)
    for ballot in (0, 1):
        got = run(frames, grid, offset, ballot)
        assert got.dtype == np.uint32 and got.shape == want.shape
        assert np.array_equal(got, want), (what, frames.shape, grid, "offset", offset, "ballot", ballot, got[:6].tolist(), want[:6].tolist())
    return want


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", [1, 2, 17])
def test_shapes_and_frame_counts(shape, n):
    from sap3d_tensorflow_amd import dataflow
    H, W = shape
    frames = S.noise_frames(n, H, W, seed=n)
    if n == 17:
        frames[5] = frames[4]                              # equal frames: distance 0
        frames[9:] = frames[9:] // 2                       # and a cut
    for grid in ((1, 1), (2, 3), (4, 4)):
        g = grid_in(grid, H, W)
        want = check(frames, g, offset=(H + n) % 16, what="shapes")
        assert want[0] == 0 and (n < 17 or want[5] == 0)
    plan = dataflow.shots_plan(H, W, grid_in((4, 4), H, W), n)
    assert plan["frames_per_chunk"] == n and plan["rows_per_block"] >= 1
    if shape == (270, 480):
        assert plan["blocks_per_frame"] > 4                # more blocks than rows of cells: several blocks share a row of cells


@pytest.mark.parametrize("grid", GRIDS)
def test_every_corner_of_the_grid(grid):
    """33 x 70: cells of 8 and 9 rows, of 17 and 18 columns, whose boundaries fall inside 16-byte words."""
    frames = S.noise_frames(3, 33, 70, seed=sum(grid))
    frames[2, :, 35:] = 255 - frames[1, :, 35:]            # a change in the right half only
    want = check(frames, grid, offset=7, what="grids")
    assert want[1] > 0 and want[2] > 0
    # the cells see where the change is: a frame whose halves are swapped is the same frame to a 1 x 1 grid only
    swapped = np.stack([frames[0], frames[0][:, ::-1]])
    d = check(swapped, grid, offset=1, what="mirror")
    assert (d[1] == 0) == (grid[1] == 1)


def test_more_frames_than_a_chunk_holds():
    """The plan's chunk plus three: the first table of the second chunk is compared with the last of the first, which was carried
    over; a cut is planted exactly on the seam and another inside the second chunk."""
    from sap3d_tensorflow_amd import dataflow
    H, W, grid = 5, 7, (2, 3)
    chunk = dataflow.shots_plan(H, W, grid, 65535)["frames_per_chunk"]
    n = chunk + 3
    assert dataflow.shots_plan(H, W, grid, n)["frames_per_chunk"] == chunk < n
    assert dataflow.shots_plan(H, W, grid, n)["scratch_bytes"] == (chunk + 1) * 2 * 3 * 192 * 4
    base = S.noise_frames(3, H, W, seed=4)
    frames = np.empty((n, H, W, 3), np.uint8)
    frames[:chunk] = base[0]
    frames[chunk:] = base[1]
    frames[chunk + 2] = base[2]
    want = check(frames, grid, offset=3, what="chunks")
    assert np.flatnonzero(want).tolist() == [chunk, chunk + 2]


@pytest.mark.parametrize("offset", range(16))
def test_every_offset_off_the_16_byte_boundary(offset):
    """9 x 33: a row is 99 bytes, so the channel of a word's first byte changes from row to row and from frame to frame; the three
    channels hold different values, so a byte counted under the wrong channel or cell changes D."""
    rng = np.random.default_rng(offset)
    frames = np.empty((3, 9, 33, 3), np.uint8)
    frames[..., 0] = rng.integers(0, 64, (3, 9, 33))
    frames[..., 1] = rng.integers(64, 160, (3, 9, 33))
    frames[..., 2] = rng.integers(160, 256, (3, 9, 33))
    frames[2] = frames[1][:, :, ::-1]                      # B and R change places: every byte is the same, every channel is not
    for grid in ((2, 3), (4, 4)):
        want = check(frames, grid, offset=offset, what="9x33")
        assert want[2] == 4 * 9 * 33                       # B and R histograms are disjoint: 2 P each way


def test_the_32_bit_headroom():
    """Two 1080 x 1920 frames of 0 and of 255: every byte leaves its bin, D = 6 P."""
    H, W = 1080, 1920
    frames = np.zeros((2, H, W, 3), np.uint8)
    frames[1] = 255
    from sap3d_tensorflow_amd import dataflow
    for grid in ((1, 1), (4, 4)):
        assert dataflow.shot_distances(frames, grid).tolist() == [0, 6 * H * W]
    assert run(frames, (2, 2), offset=5, ballot=1).tolist() == [0, 6 * H * W]


def test_op_level_entry_equals_the_hook():
    from sap3d_tensorflow_amd import dataflow
    frames = S.fixture()
    for grid in ((1, 1), (2, 3), (4, 4)):
        want = S.distances(frames, *grid)
        assert np.array_equal(dataflow.shot_distances(frames, grid), want)
        starts = dataflow.shot_cuts(want, 24 * 40, **S.FIXTURE_RULE)
        assert starts.dtype == np.int32 and starts.tolist() == [0] + S.FIXTURE_CUTS


CUT_CASES = [
    ("tie at 256", [0, 10, 400, 400, 10, 149, 150, 10, 10, 500], 100, dict(threshold=250, window=1, ratio=256, min_length=1)),
    ("tie at 257", [0, 10, 400, 400, 10, 149, 150, 10, 10, 500], 100, dict(threshold=250, window=1, ratio=257, min_length=1)),
    ("too near the last cut and the end", [0, 10, 400, 400, 10, 149, 150, 10, 10, 500], 100, dict(threshold=250, window=0, ratio=256, min_length=2)),
    ("min_length longer than the video", [0, 600, 600, 600], 100, dict(threshold=1, window=0, ratio=256, min_length=9)),
    ("window past both ends", [0, 10, 400, 400, 10, 149, 150, 10, 10, 500], 100, dict(threshold=250, window=32, ratio=256, min_length=1)),
    ("one frame", [0], 100, dict(threshold=1, window=0, ratio=256, min_length=1)),
    ("two frames", [0, 600], 100, dict(threshold=1000, window=5, ratio=65535, min_length=1)),
    ("64-bit products", [0, 6 * 2 ** 28, 6 * 2 ** 28 - 1, 3], 2 ** 28, dict(threshold=1000, window=32, ratio=65535, min_length=1)),
    ("every frame a cut", [0] + [600] * 299, 100, dict(threshold=1000, window=0, ratio=256, min_length=1)),
]


@pytest.mark.parametrize("case", CUT_CASES, ids=[c[0] for c in CUT_CASES])
def test_the_decision(case):
    from sap3d_tensorflow_amd import dataflow
    _, D, P, rule = case
    want = S.cuts(D, P, **rule)
    got = dataflow.shot_cuts(np.array(D, np.uint32), P, **rule)
    assert got.tolist() == want, (case[0], got.tolist(), want)


def test_the_decision_on_random_signals():
    from sap3d_tensorflow_amd import dataflow
    rng = np.random.default_rng(11)
    for F, window, ratio, min_length in ((300, 2, 300, 3), (257, 32, 256, 1), (1000, 7, 1024, 10)):
        D = rng.integers(0, 150, F).astype(np.uint32)       # below 600 / 4: a lone spike passes every ratio used here
        D[0] = 0
        D[rng.integers(1, F, F // 10)] = 600                # spikes, some of them within a window of one another
        want = S.cuts(D, 100, 500, window, ratio, min_length)
        assert len(want) > 3
        assert dataflow.shot_cuts(D, 100, 500, window, ratio, min_length).tolist() == want


def test_a_small_cap_keeps_the_count():
    from sap3d_tensorflow_amd import _lib, dataflow
    D = np.array([0] + [600] * 9, np.uint32)
    cfg = dataflow.shots_cfg((1, 1), 1000, 0, 256, 1)
    starts, count = np.full(4, -7, np.int32), C.c_int(0)
    assert _lib.lib().p3d_shot_cuts(0, D.ctypes.data_as(_lib._u32p), 10, 100, cfg, starts.ctypes.data_as(_lib._i32p), 3, C.byref(count)) == 0
    assert count.value == 10 and starts.tolist() == [0, 1, 2, -7]


def test_refusals_launch_nothing():
    """Every refusal leaves p3d_last_error set, and happens ahead of any launch: the outputs keep what they held."""
    from sap3d_tensorflow_amd import _lib, dataflow
    lib = _lib.lib()
    frames = S.noise_frames(2, 5, 7)
    u8, u32, i32 = _lib._u8p, _lib._u32p, _lib._i32p

    def signal(n=2, H=5, W=7, gy=2, gx=3, offset=0, ballot=0, hook=False, fr=frames, with_out=True):
        D = np.full(2, 7, np.uint32)
        head = (0, None if fr is None else fr.ctypes.data_as(u8), n, H, W, gy, gx)
        out = D.ctypes.data_as(u32) if with_out else None
        rc = lib.p3d_debug_shot_distances_u8(*head, offset, ballot, out) if hook else lib.p3d_shot_distances_u8(*head, out)
        return rc, lib.p3d_last_error().decode(), bool((D == 7).all())

    for hook in (False, True):
        rc, _, untouched = signal(hook=hook)
        assert rc == 0 and not untouched
        for kw, word in ((dict(n=0), "frames"), (dict(n=65536), "frames"), (dict(H=0), "empty"), (dict(W=0), "empty"), (dict(H=2 ** 14, W=2 ** 14 + 1), "2^28"),
                         (dict(gy=0), "grid"), (dict(gy=5), "grid"), (dict(gx=0), "grid"), (dict(gx=5), "grid"), (dict(H=1, gy=2), "grid"),
                         (dict(W=2, gx=3), "grid"), (dict(fr=None), "null"), (dict(with_out=False), "null")):
            rc, err, untouched = signal(hook=hook, **kw)
            assert rc == -1 and word in err and untouched, (hook, kw, rc, err)
    for kw, word in ((dict(offset=16), "offset"), (dict(offset=-1), "offset"), (dict(ballot=2), "ballot")):
        rc, err, untouched = signal(hook=True, **kw)
        assert rc == -1 and word in err and untouched, (kw, rc, err)

    def decide(F=4, P=100, cap=4, with_starts=True, with_D=True, **rule):
        D = np.array([0, 600, 0, 600], np.uint32)
        starts, count = np.full(4, -7, np.int32), C.c_int(-7)
        r = dict(threshold=500, window=1, ratio=256, min_length=1)
        r.update(rule)
        rc = lib.p3d_shot_cuts(0, D.ctypes.data_as(u32) if with_D else None, F, P, dataflow.shots_cfg((1, 1), **r),
                               starts.ctypes.data_as(i32) if with_starts else None, cap, C.byref(count))
        return rc, lib.p3d_last_error().decode(), bool((starts == -7).all() and count.value == -7)

    rc, _, untouched = decide()
    assert rc == 0 and not untouched
    for kw, word in ((dict(F=0), "frames"), (dict(F=65536), "frames"), (dict(P=0), "2^28"), (dict(P=2 ** 28 + 1), "2^28"), (dict(cap=0), "room"),
                     (dict(threshold=0), "threshold"), (dict(threshold=1001), "threshold"), (dict(window=-1), "window"), (dict(window=33), "window"),
                     (dict(ratio=255), "ratio"), (dict(ratio=65536), "ratio"), (dict(min_length=0), "minimum length"),
                     (dict(with_starts=False), "null"), (dict(with_D=False), "null")):
        rc, err, untouched = decide(**kw)
        assert rc == -1 and word in err and untouched, (kw, rc, err)
    with pytest.raises(_lib.P3dError):
        dataflow.shots_plan(5, 7, (5, 1), 1)
