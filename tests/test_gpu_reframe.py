"""The kernels of csrc/reframe.hip through p3d_debug_reframe_u8 (every device buffer, the scratch included, between guards) against
tests/reframe_ref.py, tolerance 0 everywhere: the smoothed and the raw track, the three masses and the crop.  Shapes are the
smallest at which each path can go wrong: one pixel, one window, 1 x 1 windows, rows that straddle 16-byte words (W = 33, 70) and
64-lane rows of words (W = 130 with a shifted base), 3 wc a multiple of 16 (wc = 64) and not, more maps than a chunk of tables
holds, and one map at the 32-bit headroom."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import reframe_ref as F        # noqa: E402

SHAPES = [(1, 1, 1, 1), (5, 7, 5, 7), (5, 7, 1, 1), (9, 33, 4, 17), (33, 70, 16, 9), (64, 130, 37, 64)]


def run(sal, frames, hc, wc, gate=0, R=0, offset=0):
    from sap3d_tensorflow_amd import dataflow
    return dataflow.reframe(sal, frames, (hc, wc), gate=gate, smooth=R, offset=offset)


def check(sal, frames, hc, wc, gate=0, R=0, offset=0, what=""):
    """With the frames and without: tracks and masses are the same, the crop is the replay's."""
    want = F.reframe(sal, frames, hc, wc, gate, R)
    for f in (frames, None):
        t, raw, mass, crop = run(sal, f, hc, wc, gate, R, offset)
        tag = (what, sal.shape, hc, wc, "gate", gate, "R", R, "offset", offset, "frames", f is not None)
        assert t.dtype == np.int32 and raw.dtype == np.int32 and mass.dtype == np.uint32
        assert np.array_equal(raw, want[1]), tag + ("raw", raw[:4].tolist(), want[1][:4].tolist())
        assert np.array_equal(t, want[0]), tag + ("track", t[:4].tolist(), want[0][:4].tolist())
        assert np.array_equal(mass, want[2]), tag + ("mass", mass[:4].tolist(), want[2][:4].tolist())
        assert (mass[:, 1] <= mass[:, 0]).all() and (mass[:, 0] <= mass[:, 2]).all()
        if f is None:
            assert crop is None
        else:
            assert crop.dtype == np.uint8 and crop.shape == (len(sal), hc, wc, 3)
            bad = np.argwhere(crop != want[3])
            assert bad.size == 0, tag + ("crop", len(bad), bad[:4].tolist())
    return want


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", [1, 3, 17])
def test_shapes_and_map_counts(shape, n):
    """n = 17 is one map more than a chunk of summed-area tables holds (the plan says so): the last map runs in a chunk of its own
    and the track's filter reaches across the seam."""
    from sap3d_tensorflow_amd import dataflow
    H, W, hc, wc = shape
    plan = dataflow.reframe_plan(H, W, (hc, wc), n)
    assert plan["maps_per_chunk"] == min(n, 16) and plan["positions_per_block"] >= 1
    assert plan["search_blocks"] == -(-(H - hc + 1) * (W - wc + 1) // plan["positions_per_block"])
    sal = F.blobs(n, H, W, seed=3)
    frames = F.frames_for(sal)
    want = check(sal, frames, hc, wc, gate=0, R=0, what="plain")
    check(sal, frames, hc, wc, gate=128, R=1, offset=5, what="gated, smoothed, shifted")
    if n > 1 and (H - hc + 1) * (W - wc + 1) > 1:
        assert len(np.unique(want[1], axis=0)) > 1                     # the raw track moves


def test_more_than_one_block_of_positions_a_map():
    """(64, 130, 5, 7): 60 x 124 = 7440 positions are two blocks of the search, whose bests the pick folds; the best window is put
    into either block, and tied across the two."""
    from sap3d_tensorflow_amd import dataflow
    H, W, hc, wc = 64, 130, 5, 7
    plan = dataflow.reframe_plan(H, W, (hc, wc), 4)
    assert plan["search_blocks"] >= 2
    per = plan["positions_per_block"]
    Wp = W - wc + 1
    sal = np.zeros((4, H, W), np.uint8)
    first, second = divmod(per - 3, Wp), divmod(per + 200, Wp)         # windows in block 0 and in block 1
    sal[0, first[0]:first[0] + hc, first[1]:first[1] + wc] = 200
    sal[1, second[0]:second[0] + hc, second[1]:second[1] + wc] = 200
    for m in (2, 3):                                                   # both, equal: D, then y0, then x0 decide across the blocks
        sal[m, first[0]:first[0] + hc, first[1]:first[1] + wc] = 200
        sal[m, second[0]:second[0] + hc, second[1]:second[1] + wc] = 200
    sal[3] = sal[3, ::-1, ::-1]
    want = check(sal, F.frames_for(sal), hc, wc, R=1, offset=3, what="two blocks")
    assert tuple(want[1][0]) == first and tuple(want[1][1]) == second


@pytest.mark.parametrize("offset", range(16))
def test_every_offset_off_the_16_byte_boundary(offset):
    """33 x 70 maps, three of them: map m's bytes start 6 m past the call's offset, its rows 6 bytes further each; the frames and
    the crop (16 x 9 and 7 x 64 windows: rows of 27 and of 192 bytes) are shifted by 3 and 5 times the offset."""
    sal = F.blobs(3, 33, 70, seed=offset)
    frames = F.frames_for(sal)
    check(sal, frames, 16, 9, gate=1, R=1, offset=offset, what="33x70")
    check(sal, frames, 7, 64, gate=0, R=0, offset=offset, what="33x70, 3 wc = 192")


@pytest.mark.parametrize("gate", [0, 1, 128, 255])
@pytest.mark.parametrize("R", [0, 1, 5, 255])
def test_gates_and_radii(gate, R):
    sal = F.blobs(9, 9, 33, seed=gate + R)
    sal[4] = 255 - sal[4]
    sal[2, 3, 4:9] = 255                                               # something at or above every gate
    check(sal, F.frames_for(sal), 4, 17, gate=gate, R=R, offset=(gate + R) % 16, what="gates and radii")


def test_the_tie_cases():
    """All-zero, constant and all-below-gate maps give the centred window rounded towards the top-left; two equal blobs mirrored
    about the centre are decided by y0, then x0."""
    H, W = 6, 7
    sal = np.zeros((7, H, W), np.uint8)
    sal[1] = 77
    sal[2] = 99                                                        # below the gate of the second run
    sal[3, 1, 2] = sal[3, 4, 4] = 200                                  # mirrored about the centre (2.5, 3)
    sal[4, 2, 1] = sal[4, 3, 5] = 200
    sal[5, 1, 4] = sal[5, 4, 2] = 200
    sal[6, 0, 0] = sal[6, 3, 3] = 200                                  # D before y0
    frames = F.frames_for(sal)
    for (hc, wc) in ((3, 2), (1, 1), (2, 3), (6, 7)):
        want = check(sal, frames, hc, wc, gate=0, what="ties")
        centre = ((H - hc) // 2, (W - wc) // 2)
        assert tuple(want[1][0]) == centre and tuple(want[1][1]) == centre
        want = check(sal, frames, hc, wc, gate=100, R=2, what="ties, gated")
        assert tuple(want[1][2]) == centre and want[2][2].tolist() == [0, 0, 0]
    want = F.reframe(sal, None, 1, 1)
    assert want[1][3:].tolist() == [[1, 2], [2, 1], [1, 4], [3, 3]]


@pytest.mark.parametrize("shape", [(9, 33, 4, 17), (33, 70, 16, 9), (5, 7, 1, 1)])
def test_random_bytes_with_many_ties(shape):
    H, W, hc, wc = shape
    rng = np.random.default_rng(H * W)
    sal = rng.integers(0, 4, (5, H, W), dtype=np.uint8)
    frames = F.frames_for(sal)
    for gate in (0, 2):
        want = check(sal, frames, hc, wc, gate=gate, R=1, offset=9, what="values 0 .. 3")
    M, _ = F.masses(sal[0], hc, wc, 2)
    assert (M == M.max()).sum() > 1 or hc * wc > 50                    # the small windows tie


def test_the_32_bit_headroom():
    """One 2048 x 4096 map, all 255, the window the whole map: the mass is 255 * 2^23 exactly, in closed form."""
    H, W = 2048, 4096
    sal = np.full((1, H, W), 255, np.uint8)
    t, raw, mass, crop = run(sal, None, H, W, gate=255, R=3, offset=0)
    assert crop is None and t.tolist() == [[0, 0]] and raw.tolist() == [[0, 0]]
    assert mass.tolist() == [[255 * 2 ** 23] * 3] and 255 * 2 ** 23 < 2 ** 31


def test_op_level_entry_equals_the_hook():
    """p3d_reframe_u8 (buffers carved from the stream's scratch) returns what the hook returns."""
    from sap3d_tensorflow_amd import dataflow
    sal = F.blobs(19, 33, 70, seed=2)
    frames = F.frames_for(sal)
    want = F.reframe(sal, frames, 16, 9, 40, 2)
    for f in (frames, None):
        got = dataflow.reframe(sal, f, (16, 9), gate=40, smooth=2)
        for g, w in zip(got[:3], want[:3]):
            assert np.array_equal(g, w)
        assert (got[3] is None) if f is None else np.array_equal(got[3], want[3])
    pt, praw, pmass = dataflow.reframe_track(sal, (16, 9), gate=40, smooth=2)
    assert np.array_equal(pt, want[0]) and np.array_equal(praw, want[1]) and np.array_equal(pmass, want[2])


def test_refusals_launch_nothing():
    """Every refusal leaves p3d_last_error set, and happens ahead of any launch: the outputs keep what they held."""
    import ctypes as C
    from sap3d_tensorflow_amd import _lib
    lib = _lib.lib()
    sal = F.blobs(2, 5, 7)
    frames = F.frames_for(sal)
    u8, i32, u32 = _lib._u8p, _lib._i32p, _lib._u32p

    def call(n=2, H=5, W=7, hc=2, wc=3, gate=0, R=0, fr=frames, with_out=True, with_track=True, hook=False):
        track = np.full((2, 2), -7, np.int32)
        raw = np.full((2, 2), -7, np.int32)
        mass = np.full((2, 3), 7, np.uint32)
        out = np.full((2, 5, 7, 3), 7, np.uint8)
        cfg = _lib.P3dReframe(hc, wc, gate, R)
        head = (0, sal.ctypes.data_as(u8), None if fr is None else fr.ctypes.data_as(u8), n, H, W, C.byref(cfg))
        tail = (track.ctypes.data_as(i32) if with_track else None, raw.ctypes.data_as(i32), mass.ctypes.data_as(u32),
                out.ctypes.data_as(u8) if with_out else None)
        rc = lib.p3d_debug_reframe_u8(*head, 0, *tail) if hook else lib.p3d_reframe_u8(*head, *tail)
        untouched = (track == -7).all() and (raw == -7).all() and (mass == 7).all() and (out == 7).all()
        return rc, lib.p3d_last_error().decode(), untouched

    for hook in (False, True):
        rc, _, untouched = call(hook=hook)
        assert rc == 0 and not untouched                               # the valid call
        for kw, word in ((dict(hc=6), "window"), (dict(wc=8), "window"), (dict(hc=0), "window"), (dict(gate=256), "gate"),
                         (dict(gate=-1), "gate"), (dict(R=256), "radius"), (dict(R=-1), "radius"), (dict(H=2 ** 12, W=2 ** 11 + 1), "2^23"),
                         (dict(n=0), "maps"), (dict(n=65536), "maps"), (dict(fr=None), "out is given exactly when frames"),
                         (dict(with_out=False), "out is given exactly when frames"), (dict(with_track=False), "null")):
            rc, err, untouched = call(hook=hook, **kw)
            assert rc == -1 and word in err and untouched, (hook, kw, rc, err)
    rc, err, _ = call(hook=True)
    assert rc == 0
    cfg = _lib.P3dReframe(2, 3, 0, 0)
    track = np.zeros((2, 2), np.int32)
    assert lib.p3d_debug_reframe_u8(0, sal.ctypes.data_as(u8), None, 2, 5, 7, C.byref(cfg), 16, track.ctypes.data_as(i32), None, None, None) == -1
    assert "offset" in lib.p3d_last_error().decode()
