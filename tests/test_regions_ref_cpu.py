"""tests/regions_ref.py, the numpy replay of "Salient regions of 8-bit maps" (include/p3d_hip.h), against two independent
statements -- scipy.ndimage where it is installed, a brute-force flood fill always -- and against planted maps whose tables are
written out by hand.  No GPU."""
import numpy as np
import pytest

import regions_ref as rr
from regions_ref import AREA, CX, CY, ID, MASS, OVERLAP, PEAK, PEAK_X, PEAK_Y, PREV, ROOT, X0, X1, Y0, Y1


def flood_roots(s, gate, conn):
    """Every pixel's ROOT by flood fill from each unvisited foreground pixel in linear order (the first pixel met is the root)."""
    H, W = s.shape
    out = np.full((H, W), -1, np.int64)
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 8 else [])
    for y0 in range(H):
        for x0 in range(W):
            if s[y0, x0] < gate or out[y0, x0] >= 0:
                continue
            out[y0, x0] = y0 * W + x0
            todo = [(y0, x0)]
            while todo:
                y, x = todo.pop()
                for dy, dx in steps:
                    v, u = y + dy, x + dx
                    if 0 <= v < H and 0 <= u < W and s[v, u] >= gate and out[v, u] < 0:
                        out[v, u] = y0 * W + x0
                        todo.append((v, u))
    return out


MAPS = [("blobs", rr.blobs(1, 33, 70, 3)[0], 60), ("blobs2", rr.blobs(1, 20, 31, 9, count=9)[0], 128), ("checker", rr.checkerboard(9, 33), 1),
        ("serpentine", rr.serpentine(17, 40), 1), ("spiral", rr.spiral(21, 30), 255 - 35), ("comb", rr.comb(12, 19), 100),
        ("ring", rr.ring_island(11, 13), 50), ("noise", np.random.RandomState(4).randint(0, 256, (24, 37)).astype(np.uint8), 140)]


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name,s,gate", MAPS, ids=[m[0] for m in MAPS])
def test_roots_equal_a_flood_fill(name, s, gate, conn):
    assert np.array_equal(rr.root_map(s, gate, conn), flood_roots(s, gate, conn))


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name,s,gate", MAPS, ids=[m[0] for m in MAPS])
def test_statistics_equal_scipy(name, s, gate, conn):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if conn == 8 else ndi.generate_binary_structure(2, 1)
    lab, count = ndi.label(s >= gate, structure=structure)
    roots = rr.root_map(s, gate, conn)
    st = rr.component_stats(s, roots)
    assert len(st) == count
    # scipy numbers components in the order of their first pixel, which is the order of ROOT
    ordered = sorted(st)
    boxes = ndi.find_objects(lab)
    sums = ndi.sum(s.astype(np.int64), lab, index=np.arange(1, count + 1)) if count else []
    areas = ndi.sum(np.ones_like(s, np.int64), lab, index=np.arange(1, count + 1)) if count else []
    peaks = ndi.maximum(s, lab, index=np.arange(1, count + 1)) if count else []
    for k, r in enumerate(ordered):
        v = st[r]
        assert np.array_equal(lab == k + 1, roots == r)
        assert (v[MASS], v[AREA], v[PEAK]) == (int(sums[k]), int(areas[k]), int(peaks[k]))
        assert (v[Y0], v[Y1] + 1, v[X0], v[X1] + 1) == (boxes[k][0].start, boxes[k][0].stop, boxes[k][1].start, boxes[k][1].stop)
        cy, cx = ndi.center_of_mass(s.astype(np.float64), lab, k + 1)
        assert abs(v[CY] - cy) <= 0.5 + 1e-9 and abs(v[CX] - cx) <= 0.5 + 1e-9
        assert s[v[PEAK_Y], v[PEAK_X]] == v[PEAK] and roots[v[PEAK_Y], v[PEAK_X]] == r


def test_two_planted_regions_by_hand():
    s = np.zeros((5, 7), np.uint8)
    s[0, 0], s[0, 1], s[1, 0], s[1, 1], s[4, 6] = 100, 100, 100, 200, 250
    s[2, 4] = 49                                              # below the gate
    rec, counts, lab = rr.regions(s, 50, conn=4, K=3)
    assert counts.tolist() == [[2, 2, 2]]
    assert rec[0, 0].tolist() == [0, 4, 500, 0, 0, 1, 1, 200, 1, 1, 1, 1, -1, -1, 0]
    assert rec[0, 1].tolist() == [34, 1, 250, 4, 6, 4, 6, 250, 4, 6, 4, 6, -1, -1, 0]
    assert rec[0, 2].tolist() == [-1] * 15
    want = np.full((5, 7), 255, np.uint8)
    want[0:2, 0:2] = 0
    want[4, 6] = 1
    assert np.array_equal(lab[0], want)
    # min_area 2 drops the heavy single pixel from the kept but not from the found; K = 1 then keeps what is left
    rec, counts, lab = rr.regions(s, 50, conn=4, min_area=2, K=1)
    assert counts.tolist() == [[2, 1, 1]] and rec[0, 0, ROOT] == 0 and (lab[0] == 1).sum() == 0


def test_a_diagonal_pair_by_hand():
    s = np.array([[9, 0], [0, 9]], np.uint8)
    rec, counts, _ = rr.regions(s, 1, conn=4, K=2)
    assert counts.tolist() == [[2, 2, 2]]
    assert rec[0, :, ROOT].tolist() == [0, 3]                 # equal masses: ROOT decides
    rec, counts, lab = rr.regions(s, 1, conn=8, K=2)
    assert counts.tolist() == [[1, 1, 1]]
    assert rec[0, 0].tolist() == [0, 2, 18, 0, 0, 1, 1, 9, 0, 0, 1, 1, -1, -1, 0]      # the centre (1, 1) is not a pixel of the region
    assert lab[0].tolist() == [[0, 255], [255, 0]]


MERGE_SPLIT = rr.merge_split()


def test_merge_split_and_vanish_by_hand():
    rec, counts, _ = rr.regions(MERGE_SPLIT, 1, conn=4, K=2, link=True)
    assert counts[:, 2].tolist() == [2, 1, 2, 0, 1]
    assert rec[:, :, [ROOT, ID, PREV, OVERLAP]].tolist() == rr.MERGE_SPLIT_LINK
    rec, _, _ = rr.regions(MERGE_SPLIT, 1, conn=4, K=2, link=True, shots=[0, 2])
    assert rec[:, :, [ROOT, ID, PREV, OVERLAP]].tolist() == rr.MERGE_SPLIT_LINK_SHOTS


def test_an_heir_tie_takes_the_smaller_rank():
    rec, counts, _ = rr.regions(rr.heir_tie(), 1, conn=8, K=4, link=True)
    assert counts[:, 2].tolist() == [1, 2]
    assert rec[1, :2][:, [ROOT, ID, PREV, OVERLAP]].tolist() == rr.HEIR_TIE_LINK


def test_link_off_leaves_the_three_fields_neutral():
    rec, counts, _ = rr.regions(MERGE_SPLIT, 1, K=2)
    for f in range(len(MERGE_SPLIT)):
        k = counts[f, 2]
        assert (rec[f, :k, ID] == -1).all() and (rec[f, :k, PREV] == -1).all() and (rec[f, :k, OVERLAP] == 0).all()
        assert (rec[f, k:] == -1).all()


def test_generators_are_what_their_names_say():
    assert rr.regions(rr.checkerboard(9, 33), 1, conn=4, K=64)[1].tolist() == [[149, 149, 64]]
    assert rr.regions(rr.checkerboard(9, 33), 1, conn=8, K=64)[1].tolist() == [[1, 1, 1]]
    for m in (rr.serpentine(33, 70), rr.spiral(33, 70), rr.comb(33, 70)):
        assert rr.regions(m, 1, conn=4, K=4)[1].tolist() == [[1, 1, 1]]
    ring = rr.ring_island(11, 13)
    assert rr.regions(ring, 50, conn=4, K=4)[1][0, 0] == 3 and rr.regions(ring, 50, conn=8, K=4)[1][0, 0] == 2
