"""No-GPU checks of tests/qpmap_ref.py, the numpy replay of include/p3d_hip.h's "QP maps of 8-bit maps", against cases worked by
hand, and of dataflow.qp_law, the host table that goes with it."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import qpmap_ref as qr        # noqa: E402


def shifted_law(zero=100):
    """law[v] = v - zero, clipped to -127 .. 127: a level reads as its own offset."""
    return np.clip(np.arange(256) - zero, -127, 127).astype(np.int32)


def test_one_pixel():
    # SUM = 200, AREA = 1: MEAN = 401 // 2 = 200, L = (128 * 200 + 128 * 200 + 128) >> 8 = 200
    sal = np.full((1, 1, 1), 200, np.uint8)
    qp, lev, st = qr.qpmap(sal, shifted_law(), block=8, balance_on=0)
    assert lev.tolist() == [[[200]]] and qp.tolist() == [[[100]]] and st.tolist() == [[100, 100, 100, 100]]
    # balanced: S1 = 100, A = 1, m = 201 // 2 = 100, q2 = 100 + (7 - 100)
    qp, _, st = qr.qpmap(sal, shifted_law(), block=8, balance_on=1, target=7)
    assert qp.tolist() == [[[7]]] and st.tolist() == [[7, 7, 100, 7]]


@pytest.mark.parametrize("B", qr.BLOCKS)
@pytest.mark.parametrize("v", [0, 37, 255])
def test_constant_map(B, v):
    law = qr.linear_law()
    sal = np.full((2, 33, 70), v, np.uint8)
    for pw in (0, 128, 256):
        qp, lev, st = qr.qpmap(sal, law, block=B, peak_weight=pw, dilate_r=1, balance_on=0)
        assert qp.shape == (2, -(-33 // B), -(-70 // B)) and (lev == v).all() and (qp == law[v]).all()
        assert (st == [law[v], law[v], 33 * 70 * law[v], 33 * 70 * law[v]]).all()
        qp, _, st = qr.qpmap(sal, law, block=B, peak_weight=pw, balance_on=1, target=-3)
        assert (qp == -3).all() and (st[:, 3] == -3 * 33 * 70).all()


def test_partial_edge_block_mean():
    # 3 x 10 at B = 8: block (0, 1) holds columns 8, 9 of three rows, AREA = 6; SUM = 22: MEAN = (44 + 6) // 12 = 4 (22 / 6 = 3.67)
    sal = np.zeros((1, 3, 10), np.uint8)
    sal[0, :, 8:] = [[1, 2], [3, 4], [5, 7]]
    assert qr.areas(3, 10, 8).tolist() == [[24, 6]]
    _, lev, _ = qr.qpmap(sal, qr.linear_law(), block=8, peak_weight=0)
    assert lev.tolist() == [[[0, 4]]]
    # the peak alone, and half of each: (128 * 7 + 128 * 4 + 128) >> 8 = 6
    assert qr.qpmap(sal, qr.linear_law(), block=8, peak_weight=256)[1].tolist() == [[[0, 7]]]
    assert qr.qpmap(sal, qr.linear_law(), block=8, peak_weight=128)[1].tolist() == [[[0, 6]]]
    # SUM = 21 of 6: MEAN = 48 // 12 = 4 (3.5 rounds up)
    sal[0, 2, 9] = 6
    assert qr.qpmap(sal, qr.linear_law(), block=8, peak_weight=0)[1].tolist() == [[[0, 4]]]


def test_dilate_clips_to_the_grid():
    sal = np.zeros((1, 24, 40), np.uint8)
    sal[0, 8:16, 16:24] = 90                                  # block (1, 2) of a 3 x 5 grid
    lev = lambda r: qr.qpmap(sal, qr.linear_law(), block=8, peak_weight=0, dilate_r=r)[1][0]      # noqa: E731
    assert lev(0).tolist() == [[0, 0, 0, 0, 0], [0, 0, 90, 0, 0], [0, 0, 0, 0, 0]]
    assert lev(1).tolist() == [[0, 90, 90, 90, 0]] * 3
    assert (lev(8) == 90).all()


def test_floor_division_on_a_negative_sum():
    assert qr.floor_mean(-5, 4) == -1 and qr.floor_mean(5, 4) == 1 and qr.floor_mean(-2, 4) == 0 and qr.floor_mean(-3, 4) == -1
    # 1 x 9 at B = 8: areas 8 and 1, q1 = (-1, 3): S1 = -5, A = 9, m = (-10 + 9) // 18 = -1 (truncation would say 0)
    sal = np.array([[[10] * 8 + [20]]], np.uint8)
    law = np.zeros(256, np.int32)
    law[10], law[20] = -1, 3
    qp, _, st = qr.qpmap(sal, law, block=8, peak_weight=0, balance_on=1, target=0)
    assert qp.tolist() == [[[0, 4]]] and st.tolist() == [[0, 4, -5, 4]]
    # saturation at lo and at hi; the statistics say what the mean became
    qp, _, st = qr.qpmap(sal, law, block=8, peak_weight=0, balance_on=1, target=0, lo=0, hi=3)
    assert qp.tolist() == [[[0, 3]]] and st.tolist() == [[0, 3, -5, 3]]
    qp, _, st = qr.qpmap(sal, law, block=8, peak_weight=0, balance_on=0, target=1, lo=0, hi=2)
    assert qp.tolist() == [[[0, 2]]] and st.tolist() == [[0, 2, -5, 2]]


def test_limiter_and_shot_starts():
    sal = np.array([100, 90, 120, 80], np.uint8).reshape(4, 1, 1)      # q0 = 0, -10, 20, -20
    run = lambda **k: qr.qpmap(sal, shifted_law(), block=8, balance_on=0, **k)[0].ravel().tolist()      # noqa: E731
    assert run() == [0, -10, 20, -20]
    assert run(fall=3, rise=5) == [0, -3, 2, -1]
    assert run(fall=3) == [0, -3, 20, 17] and run(rise=5) == [0, -10, -5, -20]
    assert run(fall=3, rise=5, shots=[0, 2]) == [0, -3, 20, 17]           # frame 2 starts a shot: q1 = q0 there
    assert run(fall=3, rise=5, shots=[0, 1, 2, 3]) == [0, -10, 20, -20]
    # the limiter's state is q1, never q2: a clamp does not feed back
    got = qr.qpmap(sal, shifted_law(), block=8, balance_on=0, fall=3, rise=5, lo=-2, hi=1)[0].ravel().tolist()
    assert got == [0, -2, 1, -1]


def test_replay_refuses_what_the_contract_excludes():
    sal = np.zeros((1, 4, 4), np.uint8)
    law = qr.linear_law()
    for kw in (dict(block=12), dict(peak_weight=257), dict(dilate_r=9), dict(fall=255), dict(rise=-1), dict(balance_on=2),
               dict(lo=3, hi=2, target=2), dict(target=5, hi=4), dict(lo=-128)):
        with pytest.raises(ValueError):
            qr.qpmap(sal, law, **kw)
    bad = law.copy()
    bad[7] = 128
    with pytest.raises(ValueError):
        qr.qpmap(sal, bad)


def test_input_makers():
    a, b = qr.blobs(3, 33, 70, seed=5), qr.blobs(3, 33, 70, seed=5)
    assert a.dtype == np.uint8 and a.shape == (3, 33, 70) and np.array_equal(a, b) and a.max() > 60 and not np.array_equal(a[0], a[1])
    f, starts = qr.frames(6, 9, 33, seed=2, shots=[2, 3, 5])
    assert f.shape == (6, 9, 33) and starts.tolist() == [0, 2, 3, 5] and starts.dtype == np.int32


# ---- dataflow.qp_law ---------------------------------------------------------------------------------------------------------------
def test_qp_law_end_points_and_monotonicity():
    from sap3d_tensorflow_amd import dataflow
    for lo, hi, gate, gamma in [(-12, 6, 0, 1.0), (-127, 127, 0, 1.0), (-20, 0, 40, 0.5), (-6, 6, 254, 2.0), (3, 3, 10, 1.0), (-9, 4, 100, 3.0)]:
        law = dataflow.qp_law(lo, hi, gate, gamma)
        assert law.dtype == np.int32 and law.shape == (256,)
        assert (law[:gate] == hi).all() and law[gate] == hi and law[255] == lo
        assert (np.diff(law) <= 0).all() and law.min() == lo and law.max() == hi
    # gamma = 1 is the straight line, rounded half up: lo = -1, hi = 0 turns at x = 1 / 2, v = 127.5
    law = dataflow.qp_law(-1, 0)
    assert (law[:128] == 0).all() and (law[128:] == -1).all()
    assert np.array_equal(dataflow.qp_law(-20, 6), qr.linear_law(-20, 6))
    # gamma bends it: below 1 the offset falls early
    assert dataflow.qp_law(-20, 0, 0, 0.5)[64] < dataflow.qp_law(-20, 0, 0, 1.0)[64] < dataflow.qp_law(-20, 0, 0, 2.0)[64]


@pytest.mark.parametrize("args", [(1, 0), (-128, 0), (0, 128), (-5, 5, -1), (-5, 5, 255), (-5, 5, 0, 0.0), (-5, 5, 0, -1.0),
                                  (-5, 5, 0, float("nan")), (-5, 5, 0, float("inf"))])
def test_qp_law_refusals(args):
    from sap3d_tensorflow_amd import dataflow
    with pytest.raises(ValueError):
        dataflow.qp_law(*args)
