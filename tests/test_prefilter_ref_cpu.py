"""tests/prefilter_ref.py, the numpy replay of include/p3d_hip.h's "Pre-filtering frames by their 8-bit maps", against the
properties the contract states; no GPU.  The device tests (test_gpu_prefilter.py) hold the kernels to this replay."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import prefilter_ref as pr        # noqa: E402
import qpmap_ref as qr            # noqa: E402

LAW = pr.falling_law()


def inputs(n=3, H=21, W=26, seed=5):
    return qr.blobs(n, H, W, seed), pr.random_frames(n, H, W, seed + 1)


def test_a_zero_law_returns_the_frames():
    sal, frames = inputs()
    out, g, wn = pr.prefilter(sal, frames, np.zeros(256, np.int32), block=8, radius=3, passes=2)
    assert (g == 0).all() and (wn == 0).all() and np.array_equal(out, frames)


@pytest.mark.parametrize("value", [0, 1, 128, 255])
def test_a_constant_frame_returns_itself(value):
    sal, _ = inputs()
    frames = np.full(sal.shape + (3,), value, np.uint8)
    frames[..., 1] = 255 - value
    for R, P in ((1, 1), (5, 3), (16, 2)):
        out, _, wn = pr.prefilter(sal, frames, LAW, block=8, radius=R, passes=P)
        assert wn.max() > 0 and np.array_equal(out, frames)


def test_a_law_of_64_without_a_limiter_returns_low():
    sal, frames = inputs()
    out, g, wn = pr.prefilter(sal, frames, np.full(256, 64, np.int32), block=16, radius=2, passes=2)
    assert (g == 64).all() and (wn == 64 * 32 * 32).all()
    for f in range(len(frames)):
        assert np.array_equal(out[f], pr.low_pass(frames[f], 2, 2))
    assert not np.array_equal(out, frames)


def test_one_box_pass_window_by_window():
    H, W, R = 6, 5, 2
    frame = pr.random_frames(1, H, W, 9)[0].astype(np.int64)
    got = pr.box_pass(frame, R)
    A = (2 * R + 1) ** 2
    for y in range(H):
        for x in range(W):
            for k in range(3):
                total = sum(int(frame[min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1), k])
                            for dy in range(-R, R + 1) for dx in range(-R, R + 1))
                assert got[y, x, k] == (2 * total + A) // (2 * A), (y, x, k)


@pytest.mark.parametrize("B", pr.BLOCKS)
def test_a_constant_grid_gives_a_constant_weight(B):
    H, W = 37, 300
    for c in (0, 1, 37, 64):
        g = np.full((-(-H // B), -(-W // B)), c, np.int64)
        assert (pr.weight(g, H, W, B) == c * (2 * B) ** 2).all()


@pytest.mark.parametrize("B", [8, 32])
def test_the_weight_lies_between_its_four_grid_entries(B):
    H, W = 70, 101
    Hb, Wb = -(-H // B), -(-W // B)
    g = np.random.RandomState(B).randint(0, 65, (Hb, Wb)).astype(np.int64)
    wn = pr.weight(g, H, W, B)
    ja, jb, _ = pr.axis_terms(H, Hb, B)
    ia, ib, _ = pr.axis_terms(W, Wb, B)
    four = np.stack([g[ja][:, ia], g[ja][:, ib], g[jb][:, ia], g[jb][:, ib]])
    D2 = (2 * B) ** 2
    assert (wn >= four.min(0) * D2).all() and (wn <= four.max(0) * D2).all()
    assert ((wn > four.min(0) * D2) & (wn < four.max(0) * D2)).any()       # and it interpolates


def test_the_largest_numerator_at_the_largest_block():
    B, H, W = 128, 20, 24
    frame = np.full((H, W, 3), 255, np.uint8)
    for c in (0, 33, 64):
        wn = pr.weight(np.full((1, 1), c, np.int64), H, W, B)
        out, top = pr.blend(frame, pr.low_pass(frame, 4, 2), wn, B)
        assert top < 2 ** 31 and top == 255 * (1 << 22) + (1 << 21) and (out == 255).all()


def test_rise_does_not_cross_the_start_of_a_shot():
    sal, starts = qr.frames(6, 33, 40, seed=4, shots=[3])
    free = pr.grid(sal, LAW, block=8)
    slow = pr.grid(sal, LAW, block=8, rise=2, shots=starts)
    assert np.array_equal(slow[0], free[0]) and np.array_equal(slow[3], free[3])       # a shot's first frame: the unlimited strength
    assert (slow[1:3] <= slow[0:2] + 2).all() and (slow[4:6] <= slow[3:5] + 2).all()
    assert not np.array_equal(slow, free)                      # the limiter binds somewhere
    assert (slow[3] > slow[2] + 2).any()                       # and the cut is crossed freely
    uncut = pr.grid(sal, LAW, block=8, rise=2)
    assert not np.array_equal(uncut[3], free[3])


def test_config_ranges():
    sal, frames = inputs(1, 9, 9)
    good = dict(block=8, peak_weight=128, dilate=0, fall=0, rise=0, radius=1, passes=1)
    pr.prefilter(sal, frames, LAW, **good)
    for change in (dict(block=12), dict(peak_weight=257), dict(dilate=9), dict(fall=65), dict(rise=-1), dict(radius=0), dict(radius=17),
                   dict(passes=0), dict(passes=4)):
        with pytest.raises(ValueError):
            pr.prefilter(sal, frames, LAW, **dict(good, **change))
    for bad in (65, -1):
        law = LAW.copy()
        law[7] = bad
        with pytest.raises(ValueError):
            pr.prefilter(sal, frames, law, **good)
