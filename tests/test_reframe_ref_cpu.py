"""tests/reframe_ref.py (the numpy replay of include/p3d_hip.h's "Reframing around 8-bit maps") against cases worked by hand, the
product's host statements of the same law (dataflow.reframe_track / reframe_crop) against the replay, and the driver's
aspect-to-window rule.  No GPU."""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import reframe_ref as F        # noqa: E402


def one(s, hc, wc, gate=0):
    t, raw, mass, _ = F.reframe(np.asarray(s, np.uint8)[None], None, hc, wc, gate, 0)
    assert np.array_equal(t, raw)
    return tuple(int(v) for v in raw[0]), tuple(int(v) for v in mass[0])


def test_a_3_by_4_map_with_a_known_best_window():
    s = [[1, 2, 3, 4],
         [5, 6, 7, 8],
         [9, 1, 2, 3]]
    # 2 x 2 windows: (0,0) 14, (0,1) 18, (0,2) 22, (1,0) 21, (1,1) 16, (1,2) 20
    M, T = F.masses(np.array(s, np.uint8), 2, 2, 0)
    assert M.tolist() == [[14, 18, 22], [21, 16, 20]] and T == 51
    assert one(s, 2, 2) == ((0, 2), (22, 22, 51))
    # gate 5 keeps 5 6 7 8 9: (0,0) 11, (0,1) 13, (0,2) 15, (1,0) 20, (1,1) 13, (1,2) 15
    assert F.masses(np.array(s, np.uint8), 2, 2, 5)[0].tolist() == [[11, 13, 15], [20, 13, 15]]
    assert one(s, 2, 2, gate=5) == ((1, 0), (20, 20, 35))
    # the window the whole map: one position, M = T
    assert one(s, 3, 4) == ((0, 0), (51, 51, 51))
    # 1 x 1: the largest byte
    assert one(s, 1, 1) == ((2, 0), (9, 9, 51))


@pytest.mark.parametrize("H,W,hc,wc,centre", [(5, 7, 3, 3, (1, 2)), (6, 7, 3, 2, (1, 2)), (5, 8, 2, 3, (1, 2)), (4, 4, 1, 1, (1, 1)),
                                              (9, 9, 9, 9, (0, 0))])
def test_the_centred_window_rounded_towards_the_top_left(H, W, hc, wc, centre):
    """All-zero, constant and all-below-gate maps tie everywhere: the smallest D wins, and where H - hc (W - wc) is odd two rows
    (columns) tie in D and the smaller one wins.  (6, 7, 3, 2): H - hc = 3, y0 = 1 and 2 both give |2 y0 - 3| = 1 -> 1;
    W - wc = 5, x0 = 2 and 3 -> 2."""
    assert centre == ((H - hc) // 2, (W - wc) // 2)
    assert one(np.zeros((H, W)), hc, wc)[0] == centre
    assert one(np.full((H, W), 77), hc, wc) == (centre, (77 * hc * wc, 77 * hc * wc, 77 * H * W))
    assert one(np.full((H, W), 99), hc, wc, gate=100) == (centre, (0, 0, 0))
    rng = np.random.default_rng(0)
    assert one(rng.integers(0, 200, (H, W)), hc, wc, gate=200) == (centre, (0, 0, 0))


def test_two_equal_blobs_mirrored_about_the_centre():
    """Equal M and equal D: the smaller y0 decides, then the smaller x0."""
    s = np.zeros((7, 9), np.uint8)
    s[1, 2] = s[5, 6] = 200                       # mirror images about the centre (3, 4)
    # 1 x 1 windows at (1, 2) and (5, 6): D = |2 - 6| + |4 - 8| = 8 = |10 - 6| + |12 - 8|
    assert one(s, 1, 1) == ((1, 2), (200, 200, 400))
    s = np.zeros((7, 9), np.uint8)
    s[3, 1] = s[3, 7] = 200                       # the same row: x0 decides
    assert one(s, 1, 1) == ((3, 1), (200, 200, 400))
    s = np.zeros((7, 9), np.uint8)
    s[1, 6] = s[5, 2] = 200                       # the other diagonal: y0 before x0
    assert one(s, 1, 1) == ((1, 6), (200, 200, 400))
    # D before y0: a nearer blob lower down beats an equal one higher up
    s = np.zeros((7, 9), np.uint8)
    s[0, 0] = s[4, 4] = 200
    assert one(s, 1, 1) == ((4, 4), (200, 200, 400))
    # 3 x 3 windows round one pixel: nine windows hold it, the one nearest the centred window (2, 3) wins
    s = np.zeros((7, 9), np.uint8)
    s[0, 0] = 9
    assert one(s, 3, 3) == ((0, 0), (9, 9, 9))
    s[0, 0], s[3, 4] = 0, 9
    assert one(s, 3, 3) == ((2, 3), (9, 9, 9))


def test_gate_255():
    s = np.array([[255, 254, 0, 255], [254, 254, 254, 254], [0, 0, 255, 255]], np.uint8)
    assert F.weights(s, 255).tolist() == [[255, 0, 0, 255], [0, 0, 0, 0], [0, 0, 255, 255]]
    assert one(s, 1, 2, gate=255) == ((2, 2), (510, 510, 1020))
    assert one(s, 1, 2, gate=0) == ((2, 2), (510, 510, 255 * 4 + 254 * 5))        # four bytes of 255, five of 254
    assert one(s, 2, 2, gate=255)[1][0] == 510


def test_smoothing_of_a_step_track_by_hand():
    raw = [(0, 10)] * 3 + [(6, 4)] * 3
    # R = 1, 3 taps, (2 sum + 3) // 6:  y sums 0 0 6 12 18 18 -> 0 0 2 4 6 6; x sums 30 30 24 18 12 12 -> 10 10 8 6 4 4
    assert F.smooth(raw, 1) == [(0, 10), (0, 10), (2, 8), (4, 6), (6, 4), (6, 4)]
    # R = 2, 5 taps, (2 sum + 5) // 10: y sums 0 6 12 18 24 30 -> 0 1 2 4 5 6 (17 // 10, 29 // 10, 41 // 10, 53 // 10)
    #                                   x sums 50 44 38 32 26 20 -> 10 9 8 6 5 4 (93 // 10, 81 // 10, 69 // 10, 57 // 10)
    assert F.smooth(raw, 2) == [(0, 10), (1, 9), (2, 8), (4, 6), (5, 5), (6, 4)]
    # to the nearest (an odd number of taps has no half): two frames 0 1, R = 1: sums 0 + 0 + 1 = 1 and 0 + 1 + 1 = 2 ->
    # (2 + 3) // 6 = 0 for 1 / 3, (4 + 3) // 6 = 1 for 2 / 3
    assert F.smooth([(0, 0), (1, 1)], 1) == [(0, 0), (1, 1)]
    assert F.smooth([(0, 0), (3, 3)], 1) == [(1, 1), (2, 2)]          # sums 3 and 6: 9 // 6, 15 // 6
    # R >= n: every tap outside repeats an end.  n = 3, values 0 9 0, R = 5 (11 taps): frame 0 sees 0 x 6, then 0 9 0 and 0 x 2
    # -> sum 9 for every frame: (18 + 11) // 22 = 1
    assert F.smooth([(0, 0), (9, 9), (0, 0)], 5) == [(1, 1)] * 3
    # ... and an asymmetric one: 0 0 8, R = 3 (7 taps, (2 sum + 7) // 14).  Frame 0 reads frames c(-3 .. 3) = 0 0 0 0 1 2 2: sum 16
    # -> 39 // 14 = 2; frame 1 reads 0 0 0 1 2 2 2: sum 24 -> 55 // 14 = 3; frame 2 reads 0 0 1 2 2 2 2: sum 32 -> 71 // 14 = 5
    assert F.smooth([(0, 0), (0, 0), (8, 8)], 3) == [(2, 2), (3, 3), (5, 5)]
    # n = 1: the frame itself at every radius
    for R in (0, 1, 7, 255):
        assert F.smooth([(5, 3)], R) == [(5, 3)]
    assert F.smooth(raw, 0) == raw


def test_masses_are_ordered_on_random_maps():
    rng = np.random.default_rng(3)
    for (n, H, W, hc, wc, g, R) in ((6, 9, 11, 4, 5, 0, 2), (5, 8, 8, 3, 8, 100, 1), (9, 5, 13, 5, 4, 3, 255), (4, 6, 6, 1, 1, 0, 1)):
        sal = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
        t, raw, mass, crop = F.reframe(sal, F.frames_for(sal), hc, wc, g, R)
        assert (mass[:, 1] <= mass[:, 0]).all() and (mass[:, 0] <= mass[:, 2]).all()
        assert (t >= 0).all() and (t[:, 0] <= H - hc).all() and (t[:, 1] <= W - wc).all()
        assert crop.shape == (n, hc, wc, 3)
        assert not np.array_equal(t, raw) or n == 1
        if R:
            assert (mass[:, 1] < mass[:, 0]).any()                     # the smoothed window is somewhere else, and worse


@pytest.mark.parametrize("case", [(7, 9, 11, 4, 5, 0, 2), (3, 8, 8, 3, 8, 100, 1), (9, 5, 13, 5, 4, 3, 255), (1, 6, 7, 6, 7, 0, 0),
                                  (4, 5, 6, 1, 1, 255, 3), (5, 12, 10, 7, 3, 1, 0)])
def test_the_products_host_statements_equal_the_replay(case):
    from sap3d_tensorflow_amd import dataflow
    n, H, W, hc, wc, g, R = case
    rng = np.random.default_rng(sum(case))
    for top in (256, 4):                                               # bytes over the range, and with many ties
        sal = rng.integers(0, top, (n, H, W), dtype=np.uint8)
        if top == 4:
            sal[0] = 0
            g = min(g, 3)
        fr = F.frames_for(sal)
        t, raw, mass, crop = F.reframe(sal, fr, hc, wc, g, R)
        pt, praw, pmass = dataflow.reframe_track(sal, (hc, wc), gate=g, smooth=R)
        assert pt.dtype == np.int32 and praw.dtype == np.int32 and pmass.dtype == np.uint32
        assert np.array_equal(pt, t) and np.array_equal(praw, raw) and np.array_equal(pmass, mass), case
        assert np.array_equal(dataflow.reframe_crop(fr, pt, (hc, wc)), crop)
    one_map = dataflow.reframe_track(sal[0], (hc, wc), gate=g)
    assert np.array_equal(one_map[0], F.reframe(sal[:1], None, hc, wc, g, 0)[0])
    with pytest.raises(ValueError):
        dataflow.reframe_track(sal, (H + 1, wc))
    with pytest.raises(ValueError):
        dataflow.reframe_track(sal, (hc, wc), gate=256)
    with pytest.raises(ValueError):
        dataflow.reframe_crop(fr, np.full((n, 2), max(H, W)), (hc, wc))


def _driver():
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


def test_the_drivers_aspect_to_window_rule():
    gp = _driver()
    # 16:9 frames to 9:16: the full height, width 1080 * 9 / 16 = 607.5 -> 607 -> 606
    assert gp.aspect_window(1080, 1920, 9, 16) == (1080, 606)
    # the frame's own aspect: the whole frame; a wider aspect: the full width
    assert gp.aspect_window(1080, 1920, 16, 9) == (1080, 1920)
    assert gp.aspect_window(1080, 960, 16, 9) == (540, 960)
    assert gp.aspect_window(1080, 960, 1, 1) == (960, 960)
    assert gp.aspect_window(24, 40, 9, 16) == (24, 12)                 # 13.5 -> 13 -> 12
    assert gp.aspect_window(25, 41, 1, 1) == (24, 24)                  # odd sides round down to even
    assert gp.aspect_window(1, 50, 4, 1) == (1, 4) and gp.aspect_window(3, 3, 100, 1) == (1, 2)
    for (H, W, a, b) in ((1080, 960, 9, 16), (720, 1280, 4, 5), (33, 70, 3, 2), (64, 130, 21, 9), (7, 5, 1, 3)):
        hc, wc = gp.aspect_window(H, W, a, b)
        assert (hc, wc) == F.aspect_window(H, W, a, b)
        assert 1 <= hc <= H and 1 <= wc <= W and hc % 2 == 0 and wc % 2 == 0
        assert (hc + 2) * a > (wc - 2) * b or hc + 2 > H              # no larger even window of the aspect fits: within rounding
    # the flags
    ok = gp.parse_args(["--videos", "v", "--resident", "--reframe", "d", "--reframe-aspect", "4:5", "--reframe-gate", "30", "--reframe-smooth", "12"])
    assert ok.reframe_kw == dict(size=None, aspect=(4, 5), gate=30, smooth=12)
    ok = gp.parse_args(["--videos", "v", "--resident", "--reframe", "d", "--reframe-size", "20", "30", "--render", "r"])
    assert ok.reframe_kw == dict(size=(20, 30), aspect=None, gate=0, smooth=0) and ok.render_kw is not None
    assert gp.parse_args(["--videos", "v", "--resident", "--reframe", "d"]).reframe_kw["aspect"] == (9, 16)
    assert gp.parse_args(["--videos", "v"]).reframe_kw is None
    for bad in (["--reframe", "d"], ["--resident", "--reframe-gate", "3"], ["--resident", "--reframe", "d", "--reframe-gate", "256"],
                ["--resident", "--reframe", "d", "--reframe-smooth", "256"], ["--resident", "--reframe", "d", "--reframe-aspect", "9x16"],
                ["--resident", "--reframe", "d", "--reframe-aspect", "0:1"], ["--resident", "--reframe", "d", "--reframe-size", "0", "4"],
                ["--resident", "--reframe", "d", "--reframe-size", "4", "4", "--reframe-aspect", "1:1"]):
        with pytest.raises(SystemExit):
            gp.parse_args(["--videos", "v"] + bad)
