"""p3d_reframe_shots_u8 (csrc/reframe.hip's reframe_track_shots) against tests/shots_ref.py, tolerance 0: 17 frames in shots that
start at 0, 1, 2 and 9, every radius class, through the hook (buffers between guards) and through the stage on the stream's scratch."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import reframe_ref as F        # noqa: E402
import shots_ref as S          # noqa: E402

N, SHAPE, CROP, STARTS = 17, (9, 33), (4, 17), [0, 1, 2, 9]


def same(got, want):
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w), (g[:6].tolist(), w[:6].tolist())
    assert (got[3] is None and want[3] is None) or np.array_equal(got[3], want[3])


@pytest.mark.parametrize("R", [0, 1, 5, 255])
def test_the_track_is_smoothed_inside_the_shots(R):
    from sap3d_tensorflow_amd import dataflow
    sal = F.blobs(N, *SHAPE, seed=R)
    frames = F.frames_for(sal)
    want = S.reframe_shots(sal, frames, *CROP, 40, R, STARTS)
    for offset in (None, R % 16):
        same(dataflow.reframe(sal, frames, CROP, gate=40, smooth=R, offset=offset, shots=STARTS), want)
    same(dataflow.reframe(sal, None, CROP, gate=40, smooth=R, offset=3, shots=STARTS), want[:3] + (None,))
    if R:
        plain = dataflow.reframe(sal, None, CROP, gate=40, smooth=R)
        assert not np.array_equal(plain[0], want[0])        # the table matters
        assert np.array_equal(want[0][:2], want[1][:2])     # shots of one frame keep their raw window


@pytest.mark.parametrize("R", [0, 1, 5, 255])
def test_one_shot_is_reframe_u8(R):
    from sap3d_tensorflow_amd import dataflow
    sal = F.blobs(N, *SHAPE, seed=R + 7)
    frames = F.frames_for(sal)
    want = dataflow.reframe(sal, frames, CROP, gate=10, smooth=R)
    same(want, F.reframe(sal, frames, *CROP, 10, R))
    same(dataflow.reframe(sal, frames, CROP, gate=10, smooth=R, shots=[0]), want)
    same(dataflow.reframe(sal, frames, CROP, gate=10, smooth=R, shots=[0], offset=9), want)


def test_every_frame_its_own_shot_is_the_raw_track():
    from sap3d_tensorflow_amd import dataflow
    sal = F.blobs(N, *SHAPE, seed=1)
    t, raw, mass, _ = dataflow.reframe(sal, None, CROP, smooth=5, shots=list(range(N)), offset=0)
    assert np.array_equal(t, raw) and np.array_equal(mass[:, 0], mass[:, 1])


def test_refusals_launch_nothing():
    from sap3d_tensorflow_amd import dataflow, P3dError
    sal = F.blobs(3, 5, 7)
    for shots, word in (([1], "frame 0"), ([0, 2, 2], "ascend"), ([0, 3], "outside"), ([0, 1, 2, 3], "shots"), ([], "shots")):
        with pytest.raises(P3dError) as e:
            dataflow.reframe(sal, None, (2, 3), shots=shots)
        assert word in str(e.value), (shots, str(e.value))
    with pytest.raises(P3dError) as e:
        dataflow.reframe(sal, None, (2, 3), shots=[0], offset=16)
    assert "offset" in str(e.value)
