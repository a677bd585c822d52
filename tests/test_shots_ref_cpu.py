"""No-GPU checks of tests/shots_ref.py, the replay the shot tests compare against: it finds the planted cuts of the fixture video and
not a flash, its shot-aware filters reduce to temporal_ref.py and reframe_ref.py under one shot, and refl by hand."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import reframe_ref as F        # noqa: E402
import shots_ref as S          # noqa: E402
import temporal_ref as T       # noqa: E402

GRIDS = [(1, 1), (2, 3), (4, 4)]


@pytest.fixture(scope="module")
def video():
    v = S.fixture()
    assert v.shape == (40, 24, 40, 3) and v.dtype == np.uint8
    return v


@pytest.mark.parametrize("grid", GRIDS)
def test_the_planted_cuts_and_only_they(video, grid):
    D = S.distances(video, *grid)
    P = 24 * 40
    assert D[0] == 0 and D.dtype == np.uint32
    assert S.cuts(D, P, **S.FIXTURE_RULE) == [0] + S.FIXTURE_CUTS
    permille = D.astype(np.int64) * 1000 // (6 * P)
    inside = np.ones(len(D), bool)
    inside[S.FIXTURE_CUTS] = False
    assert permille[inside].max() <= 168 and permille[~inside].min() >= 378, (permille[inside].max(), permille[~inside].min())


@pytest.mark.parametrize("grid", GRIDS)
def test_a_flash_is_no_cut_under_the_peak_rule(video, grid):
    flash = video.copy()
    flash[10] = 255
    D = S.distances(flash, *grid)
    assert S.cuts(D, 24 * 40, **S.FIXTURE_RULE) == [0] + S.FIXTURE_CUTS
    # without the peak rule and the minimum length both sides of the white frame are cuts
    assert S.cuts(D, 24 * 40, threshold=250, window=0, ratio=256, min_length=1) == [0, 5, 10, 11, 21, 30, 33]


def test_the_decision_by_hand():
    P = 100                                                # 6 P = 600: 250 permille is 150
    D = [0, 10, 400, 400, 10, 149, 150, 10, 10, 500]
    assert S.cuts(D, P, 250, 0, 256, 1) == [0, 2, 3, 6, 9]
    assert S.cuts(D, P, 250, 1, 256, 1) == [0, 2, 3, 6, 9]          # a tie of two neighbours passes at ratio 256 ...
    assert S.cuts(D, P, 250, 1, 257, 1) == [0, 6, 9]                # ... and fails at 257
    assert S.cuts(D, P, 250, 0, 256, 2) == [0, 2, 6]                # 3 is too near 2, 9 too near the end
    assert S.cuts(D, P, 250, 32, 256, 1) == [0, 9]                  # the window reaches past both ends: only the largest
    assert S.cuts([0], P, 1, 0, 256, 1) == [0]
    assert S.cuts([0, 600], P, 1000, 5, 65535, 1) == [0, 1]         # D_0 is no neighbour: N = 0


def test_refl_by_hand():
    assert [S.refl(j, 1) for j in range(-3, 4)] == [0] * 7
    assert [S.refl(j, 2) for j in range(-3, 5)] == [1, 0, 1, 0, 1, 0, 1, 0]
    assert [S.refl(j, 3) for j in range(-5, 8)] == [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1]
    for L in (2, 3, 7):                                     # inside one period it is temporal_ref's rho
        assert [S.refl(j, L) for j in range(-(L - 1), 2 * L - 1)] == [T.rho(j, L) for j in range(-(L - 1), 2 * L - 1)]


@pytest.mark.parametrize("r", [1, 7, 24])
def test_one_shot_is_the_temporal_replay_bit_for_bit(r):
    rng = np.random.default_rng(r)
    v = rng.random((30, 11), dtype=np.float32)
    cfg = T.parse(T.GAUSS, sigma=2.5, radius=r)
    for first, n in ((0, 30), (7, 5), (29, 1)):
        want = T.gauss(v, cfg["w"], cfg["r"], first, n)
        got = S.temporal_shots(cfg, v, [0], first, n)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    cfg = T.parse(T.EMA, alpha=0.7)
    assert np.array_equal(S.temporal_shots(cfg, v, [0], 3, 20).view(np.uint32), T.ema(v, cfg["alpha"], 3, 20).view(np.uint32))


def test_shots_cut_the_temporal_filter():
    """Every shot is filtered as a video of its own and a partial read is the slice of a full one."""
    rng = np.random.default_rng(5)
    v = rng.random((20, 6), dtype=np.float32)
    starts = [0, 1, 3, 12]
    bounds = starts + [20]
    cfg = T.parse(T.GAUSS, sigma=1.5, radius=2)
    full = S.temporal_shots(cfg, v, starts)
    for lo, hi in zip(bounds, bounds[1:]):
        if hi - lo > cfg["r"]:                              # the replay of a whole video needs r <= F - 1
            assert np.array_equal(full[lo:hi].view(np.uint32), T.gauss(v[lo:hi], cfg["w"], cfg["r"]).view(np.uint32))
    one = cfg["w"][2] * v[0]                                # a shot of one frame: every tap reads the frame itself
    for d in (1, 2):
        one = one + cfg["w"][2 + d] * (v[0] + v[0])
    assert np.array_equal(full[0].view(np.uint32), one.view(np.uint32))
    assert np.array_equal(S.temporal_shots(cfg, v, starts, 2, 11).view(np.uint32), full[2:13].view(np.uint32))
    cfg = T.parse(T.EMA, alpha=0.5)
    full = S.temporal_shots(cfg, v, starts)
    for lo, hi in zip(bounds, bounds[1:]):
        assert np.array_equal(full[lo:hi].view(np.uint32), T.ema(v[lo:hi], cfg["alpha"]).view(np.uint32))
    assert np.array_equal(S.temporal_shots(cfg, v, starts, 5, 10).view(np.uint32), full[5:15].view(np.uint32))


@pytest.mark.parametrize("R", [0, 1, 5, 255])
def test_one_shot_is_the_reframe_replay(R):
    sal = F.blobs(17, 9, 33, seed=R)
    frames = F.frames_for(sal)
    want = F.reframe(sal, frames, 4, 17, 40, R)
    got = S.reframe_shots(sal, frames, 4, 17, 40, R, [0])
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_shots_cut_the_reframe_track():
    sal = F.blobs(17, 9, 33, seed=3)
    starts = [0, 1, 2, 9]
    bounds = starts + [17]
    track, raw, mass, crop = S.reframe_shots(sal, None, 4, 17, 0, 5, starts)
    assert crop is None
    for lo, hi in zip(bounds, bounds[1:]):
        t, r, m, _ = F.reframe(sal[lo:hi], None, 4, 17, 0, 5)
        assert np.array_equal(track[lo:hi], t) and np.array_equal(raw[lo:hi], r) and np.array_equal(mass[lo:hi], m)
    assert np.array_equal(track[:2], raw[:2])               # shots of one frame keep their raw window
