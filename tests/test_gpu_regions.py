"""The kernels of csrc/regions.hip through p3d_debug_regions_u8 (every device buffer, the scratch included, between guards) against
tests/regions_ref.py, tolerance 0 everywhere: the records, the counts and the label maps.  Shapes are the smallest at which each
path can go wrong: one pixel, rows that straddle 16-byte words and tile edges, one tile plus a row and a column, long union chains
across every tile border, more maps than a chunk of tables holds (with the link across the seam), and one map at the headroom."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import regions_ref as rr        # noqa: E402
from regions_ref import AREA, CX, CY, ID, MASS, OVERLAP, PEAK, PEAK_X, PEAK_Y, PREV, ROOT, X0, X1, Y0, Y1      # noqa: E402

SHAPES = [(5, 7), (9, 33), (33, 70), (64, 130)]


def run(sal, gate, conn=8, min_area=1, K=64, link=False, shots=None, labels=True, offset=0):
    from sap3d_tensorflow_amd import dataflow
    return dataflow.regions(sal, gate, connectivity=conn, min_area=min_area, max_regions=K, link=link, shots=shots, labels=labels, offset=offset)


def check(sal, gate, conn=8, min_area=1, K=64, link=False, shots=None, offset=0, what="", want=None):
    """With the label maps and without (under link the second keeps them in a ring of a chunk's maps): the same records."""
    want = rr.regions(sal, gate, conn, min_area, K, link, shots) if want is None else want
    for labels in (True, False):
        rec, counts, lab = run(sal, gate, conn, min_area, K, link, shots, labels, offset)
        tag = (what, sal.shape, "gate", gate, "c", conn, "a", min_area, "K", K, "link", link, "offset", offset, "labels", labels)
        assert rec.dtype == np.int32 and counts.dtype == np.int32 and rec.shape == (len(want[0]), K, rr.FIELDS)
        assert np.array_equal(counts, want[1]), tag + ("counts", counts[:4].tolist(), want[1][:4].tolist())
        bad = np.argwhere(rec != want[0])
        assert bad.size == 0, tag + ("records", len(bad), bad[:4].tolist(), [(int(rec[tuple(b)]), int(want[0][tuple(b)])) for b in bad[:4]])
        if labels:
            assert lab.dtype == np.uint8
            bad = np.argwhere(lab != want[2])
            assert bad.size == 0, tag + ("labels", len(bad), bad[:4].tolist())
        else:
            assert lab is None
    return want


@functools.lru_cache(maxsize=None)
def blob_case(n, H, W, gate, conn, link=True):
    sal = rr.blobs(n, H, W, seed=3)
    return sal, rr.regions(sal, gate, conn, 1, 64, link)


@pytest.mark.parametrize("value,gate,kept", [(0, 1, 0), (200, 200, 1), (200, 201, 0), (255, 255, 1)])
def test_one_pixel(value, gate, kept):
    want = check(np.full((1, 1, 1), value, np.uint8), gate, K=2)
    assert want[1].tolist() == [[kept, kept, kept]]


@pytest.mark.parametrize("shape", SHAPES)
def test_all_background_and_all_foreground(shape):
    H, W = shape
    want = check(np.zeros((1, H, W), np.uint8), 1, what="all background")
    assert want[1].tolist() == [[0, 0, 0]] and (want[0] == -1).all() and (want[2] == 255).all()
    want = check(np.full((1, H, W), 77, np.uint8), 77, conn=4, what="all foreground")
    assert want[0][0, 0, :CX + 1].tolist() == [0, H * W, 77 * H * W, 0, 0, H - 1, W - 1, 77, 0, 0, H // 2, W // 2]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", [1, 3])
def test_shapes(shape, n):
    H, W = shape
    for conn in (4, 8):
        sal, want = blob_case(n, H, W, 60, conn)
        check(sal, 60, conn=conn, link=True, what="blobs", want=want)


def test_one_tile_plus_a_row_and_a_column():
    from sap3d_tensorflow_amd import dataflow
    plan = dataflow.regions_plan(33, 70)
    H, W = plan["tile_h"] + 1, plan["tile_w"] + 1
    assert dataflow.regions_plan(H - 1, W - 1)["tiles_per_map"] == 1 and dataflow.regions_plan(H, W)["tiles_per_map"] == 4
    sal = rr.blobs(2, H, W, seed=5, count=7)
    sal[:, H - 2:, W - 3:] = 250                             # a region on the corner where the four tiles meet
    check(sal, 90, conn=4, link=True, what="2 x 2 tiles")
    check(sal, 90, conn=8, offset=9, what="2 x 2 tiles")


@pytest.mark.parametrize("offset", range(16))
def test_every_offset(offset):
    sal, want = blob_case(3, 33, 70, 60, 8)
    check(sal, 60, link=True, offset=offset, what="shifted", want=want)


def test_checkerboard():
    """c = 4: ceil(H W / 2) one-pixel components, the most a map holds, all of one mass: ROOT alone picks the K.  c = 8: one."""
    H, W = 33, 70
    s = rr.checkerboard(H, W)[None]
    want = check(s, 1, conn=4, K=64, what="checkerboard")
    assert want[1].tolist() == [[(H * W + 1) // 2, (H * W + 1) // 2, 64]]
    assert want[0][0, :, ROOT].tolist() == [2 * k for k in range(35)] + [W + 1 + 2 * k for k in range(29)]
    want = check(s, 1, conn=8, K=64, what="checkerboard")
    assert want[1].tolist() == [[1, 1, 1]] and want[0][0, 0, AREA] == (H * W + 1) // 2


@pytest.mark.parametrize("name", ["serpentine", "spiral", "comb"])
def test_long_chains_across_every_tile_border(name):
    from sap3d_tensorflow_amd import dataflow
    H, W = 67, 131
    assert dataflow.regions_plan(H, W)["tiles_per_map"] == 9
    s = getattr(rr, name)(H, W)[None]
    for conn in (4, 8):
        want = check(s, 1, conn=conn, K=3, offset=3, what=name)
        assert want[1].tolist() == [[1, 1, 1]]


@pytest.mark.parametrize("shape", [(11, 13), (40, 70)])
def test_ring_around_an_island(shape):
    s = rr.ring_island(*shape)[None]
    w4 = check(s, 50, conn=4, K=4, what="ring")
    w8 = check(s, 50, conn=8, K=4, what="ring")
    assert w4[1][0, 0] == 3 and w8[1][0, 0] == 2
    ring, island = w8[0][0, 0], w8[0][0, 1]
    assert ring[Y0] < island[Y0] and ring[X0] < island[X0] and ring[Y1] > island[Y1] and ring[X1] > island[X1]      # boxes nest
    assert w8[2][0, ring[CY], ring[CX]] != 0                 # the ring's centre is not one of its pixels


def test_equal_masses_more_components_than_k_and_min_area():
    s = np.zeros((1, 33, 70), np.uint8)
    for k, (y, x) in enumerate([(1, 1), (1, 60), (20, 30), (29, 5), (29, 64), (10, 40)]):
        s[0, y:y + 2, x:x + 3] = 100                         # six regions of one mass
    s[0, 15, 15] = 255                                       # and a single pixel, lighter than any
    want = check(s, 1, K=4, what="equal masses")
    assert want[1].tolist() == [[7, 7, 4]] and want[0][0, :, ROOT].tolist() == sorted(want[0][0, :, ROOT].tolist())
    want = check(s, 1, K=64, min_area=6, what="min_area at the area")
    assert want[1].tolist() == [[7, 6, 6]]
    want = check(s, 1, K=64, min_area=7, what="min_area above it")
    assert want[1].tolist() == [[7, 0, 0]] and (want[2] == 255).all()
    want = check(s, 1, K=1, min_area=1, what="K = 1")
    assert want[1].tolist() == [[7, 7, 1]] and want[0][0, 0, ROOT] == 71


def test_peak_ties():
    s = np.zeros((1, 9, 33), np.uint8)
    s[0, 2:6, 3:30] = 50
    s[0, 4, 20], s[0, 3, 25], s[0, 5, 4] = 90, 90, 90        # three equal peaks: the smallest linear index wins
    s[0, 7, 1:5] = 120                                       # a plateau: the peak is the root
    want = check(s, 1, K=2, what="peak ties")
    assert want[0][0, 0, [PEAK, PEAK_Y, PEAK_X]].tolist() == [90, 3, 25] and want[0][0, 1, [PEAK, PEAK_Y, PEAK_X]].tolist() == [120, 7, 1]


@pytest.mark.parametrize("gate", [1, 128, 255])
def test_gates(gate):
    sal = rr.blobs(2, 33, 70, seed=11).copy()
    sal[0, 5:8, 60:66] = 255
    sal[1, 30:33, 0:3] = 255
    want = check(sal, gate, link=True, what="gate")
    assert want[1][:, 2].min() >= 1


def test_one_map_more_than_a_chunk_links_across_the_seam():
    from sap3d_tensorflow_amd import dataflow
    H, W = 33, 70
    chunk = dataflow.regions_plan(H, W, 65535)["maps_per_chunk"]
    n = chunk + 1
    assert dataflow.regions_plan(H, W, n, link=True)["maps_per_chunk"] == chunk and chunk <= 16
    sal, want = blob_case(n, H, W, 60, 8)
    check(sal, 60, link=True, offset=7, what="chunk seam", want=want)
    assert (want[0][chunk, :, PREV] >= 0).any()              # the first frame of the second chunk inherits from the last of the first
    check(sal, 60, link=True, shots=[0, chunk], what="a shot starts at the seam")


def test_headroom():
    """2048 x 4096 bytes of 255: one component with the largest mass a map can have; its centre needs the 64-bit sums."""
    H, W = 2048, 4096
    rec, counts, lab = run(np.full((1, H, W), 255, np.uint8), 255, conn=4, K=1)
    mass = 255 * 2 ** 23
    sy, sx = 255 * W * (H * (H - 1) // 2), 255 * H * (W * (W - 1) // 2)
    assert counts.tolist() == [[1, 1, 1]]
    assert rec[0, 0].tolist() == [0, 2 ** 23, mass, 0, 0, H - 1, W - 1, 255, 0, 0, (2 * sy + mass) // (2 * mass), (2 * sx + mass) // (2 * mass), -1, -1, 0]
    assert (lab == 0).all()


def test_a_drifting_blob_keeps_its_id():
    yy, xx = np.mgrid[0:33, 0:70]
    sal = np.stack([np.where((yy - 16) ** 2 + (xx - 10 - 4 * f) ** 2 <= 36, 200, 0).astype(np.uint8) for f in range(8)])
    want = check(sal, 100, link=True, K=3, what="drift")
    assert want[0][:, 0, ID].tolist() == [0] * 8 and want[0][1:, 0, PREV].tolist() == [0] * 7 and (want[0][1:, 0, OVERLAP] > 0).all()


def test_merge_split_vanish_and_a_shot_start():
    sal = rr.merge_split()
    want = check(sal, 1, conn=4, K=2, link=True, what="merge and split")
    assert want[0][:, :, [ROOT, ID, PREV, OVERLAP]].tolist() == rr.MERGE_SPLIT_LINK
    want = check(sal, 1, conn=4, K=2, link=True, shots=[0, 2], what="merge and split in shots")
    assert want[0][:, :, [ROOT, ID, PREV, OVERLAP]].tolist() == rr.MERGE_SPLIT_LINK_SHOTS
    want = check(rr.heir_tie(), 1, K=4, link=True, what="ties of O")
    assert want[0][1, :2][:, [ROOT, ID, PREV, OVERLAP]].tolist() == rr.HEIR_TIE_LINK


@pytest.mark.parametrize("seed", [1, 2])
def test_invariants_on_blob_fields(seed):
    gate = 70
    sal = rr.blobs(4, 64, 130, seed=seed, count=12, drift=3.0)
    rec, counts, lab = run(sal, gate, K=8, link=True, min_area=2, offset=seed)
    for f in range(len(sal)):
        k = counts[f, 2]
        r = rec[f, :k]
        assert r[:, AREA].sum() <= (sal[f] >= gate).sum()
        for name_y, name_x in ((PEAK_Y, PEAK_X), (CY, CX)):
            assert (r[:, Y0] <= r[:, name_y]).all() and (r[:, name_y] <= r[:, Y1]).all()
            assert (r[:, X0] <= r[:, name_x]).all() and (r[:, name_x] <= r[:, X1]).all()
        assert [int((lab[f] == j).sum()) for j in range(k)] == r[:, AREA].tolist()
        assert (lab[f][sal[f] < gate] == 255).all() and set(np.unique(lab[f])) <= set(range(k)) | {255}
        assert len(set(r[:, ID].tolist())) == k and (r[:, ID] >= 0).all()
        assert (np.diff(r[:, MASS]) <= 0).all()
