"""The shot-aware launches of csrc/temporal.hip through p3d_temporal_filter_shots (every device buffer, the run table included,
between guards) against tests/shots_ref.py, bit for bit: F = 40 frames cut into shots of 1, 2, r, r + 1 frames and the rest, radii
either side of the switch between four pixels a lane and one (7 | 8) and the largest, pixel counts of one lane, a few, a ragged
strip and whole strips, NEWEST and MEAN, reads that start and end inside a shot, every offset off the 16-byte boundary."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import shots_ref as S          # noqa: E402
import temporal_ref as T       # noqa: E402

F = 40
RADII = [1, 7, 8, 24]
HWS = [1, 5, 1027, 4096]


def table(r):
    """Shots of 1, 2, r, r + 1 frames and the rest (for r = 24 the rest is nothing: the last shot is cut short)."""
    starts, at = [0], 0
    for length in (1, 2, r, r + 1):
        at += length
        if at < F and at not in starts:
            starts.append(at)
    return starts


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def maps_of(hw, seed):
    return np.random.default_rng([seed, hw]).random((F, hw), dtype=np.float32)


def run(v, cfg_args, starts, first=0, n=None, **kw):
    from sap3d_tensorflow_amd import dataflow
    return dataflow.temporal_filter(v, *cfg_args, first=first, n=n, shots=starts, **kw)


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("hw", HWS)
def test_gauss_inside_the_shots(r, hw):
    v = maps_of(hw, r)
    starts = table(r)
    cfg = T.parse(T.GAUSS, sigma=0.6 * r + 0.5, radius=r)
    want = S.temporal_shots(cfg, v, starts)
    got = run(v, ("gauss", 0.6 * r + 0.5, r), starts, offset=(r + hw) % 4)
    assert np.array_equal(bits(got), bits(want)), (r, hw, starts, np.argwhere(bits(got) != bits(want))[:4].tolist())
    # reads that start and end inside a shot are the slice
    for first, n in ((2, 1), (starts[-1] - 1, 3), (1, F - 2)):
        part = run(v, ("gauss", 0.6 * r + 0.5, r), starts, first=first, n=n, offset=(first + hw) % 4)
        assert np.array_equal(bits(part), bits(want[first:first + n])), (r, hw, first, n)


@pytest.mark.parametrize("r", [1, 8])
@pytest.mark.parametrize("offset", range(4))
def test_mean_divides_on_load_at_every_offset(r, offset):
    hw = 1027
    rng = np.random.default_rng([r, offset])
    counts = rng.integers(1, 4, F).astype(np.int32)
    sums = maps_of(hw, 9) * counts[:, None].astype(np.float32)
    starts = table(r)
    v = T.inputs(1, sums, counts, 0, F - 1)
    for kind, args, cfg in (("gauss", ("gauss", 1.7, r), T.parse(T.GAUSS, sigma=1.7, radius=r)), ("ema", ("ema", 0., 0, 0.6), T.parse(T.EMA, alpha=0.6))):
        want = S.temporal_shots(cfg, v, starts, 3, 30)
        got = run(sums, args, starts, first=3, n=30, counts=counts, mode="mean", offset=offset)
        assert np.array_equal(bits(got), bits(want)), (kind, r, offset)


@pytest.mark.parametrize("r", [7, 8])
def test_one_shot_is_the_filter_without_a_table(r):
    from sap3d_tensorflow_amd import dataflow
    v = maps_of(1027, 3)
    for args in (("gauss", 2.0, r), ("ema", 0., 0, 0.35)):
        for first, n in ((0, F), (5, 17)):
            want = dataflow.temporal_filter(v, *args, first=first, n=n)
            assert np.array_equal(bits(run(v, args, [0], first=first, n=n)), bits(want)), (args, first, n)


@pytest.mark.parametrize("hw", HWS + [2 ** 18])
def test_the_moving_average_restarts_at_every_shot(hw):
    """2^18 pixels is where a lane takes four."""
    v = maps_of(hw, 1)
    starts = [0, 1, 3, 10, 11, 30]
    cfg = T.parse(T.EMA, alpha=0.8)
    want = S.temporal_shots(cfg, v, starts)
    got = run(v, ("ema", 0., 0, 0.8), starts)
    assert np.array_equal(bits(got), bits(want))
    for s in starts:
        assert np.array_equal(bits(got[s]), bits(v[s]))     # a copy of the bits
    part = run(v, ("ema", 0., 0, 0.8), starts, first=12, n=25, offset=hw % 4)
    assert np.array_equal(bits(part), bits(want[12:37]))


def test_radius_beyond_the_video_is_legal_under_a_table():
    from sap3d_tensorflow_amd import dataflow, P3dError
    v = np.random.default_rng(0).random((5, 33), dtype=np.float32)
    cfg = T.parse(T.GAUSS, sigma=3.0, radius=24)
    with pytest.raises(P3dError):
        dataflow.temporal_filter(v, "gauss", 3.0, 24)
    for starts in ([0], [0, 2], [0, 1, 2, 3, 4]):
        got = dataflow.temporal_filter(v, "gauss", 3.0, 24, shots=starts)
        assert np.array_equal(bits(got), bits(S.temporal_shots(cfg, v, starts))), starts


def test_refusals_launch_nothing():
    from sap3d_tensorflow_amd import dataflow, P3dError
    v = maps_of(5, 0)
    for kw, word in ((dict(shots=[1, 5]), "frame 0"), (dict(shots=[0, 5, 5]), "ascend"), (dict(shots=[0, F]), "outside"), (dict(shots=[0], first=30, n=11), "outside"),
                     (dict(shots=[0], offset=4), "offset"), (dict(shots=[0, 7], counts=np.r_[np.ones(7, np.int32), 0, np.ones(F - 8, np.int32)], first=8, n=3), "frame 7")):
        with pytest.raises(P3dError) as e:
            dataflow.temporal_filter(v, "gauss", 1.0, 2, **kw)
        assert word in str(e.value), (kw, str(e.value))
    # frame 7 has no prediction, and a read inside the shot before it does not need it
    counts = np.r_[np.ones(7, np.int32), 0, np.ones(F - 8, np.int32)]
    got = dataflow.temporal_filter(v, "gauss", 1.0, 2, shots=[0, 7], counts=counts, first=4, n=3)
    assert np.array_equal(bits(got), bits(S.temporal_shots(T.parse(T.GAUSS, sigma=1.0, radius=2), v, [0, 7], 4, 3)))
