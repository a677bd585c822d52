"""The shot table of a resident video (P3DSession.video_detect_shots / video_set_shots / video_shots): the planted cut of a two-shot
source is found on the device; under the installed table the maps, the 8-bit maps and the reframe track are what the op-level
functions return on the unfiltered maps; removing the table, or opening another video, restores what was returned before; score and
render do not read it; refusals change nothing."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import reframe_ref as F        # noqa: E402
import shots_ref as S          # noqa: E402

CFG = dict(base=16, blocks=(2, 2, 3))
F20, T, SRC, CUT = 20, 16, (24, 40), 8
CROP = (24, 14)
RULE = dict(threshold=250, window=2, ratio=512, min_length=3)


def _session():
    from sap3d_tensorflow_amd import P3DSession
    return P3DSession("unet", seed=2, batch=3, frames=T, height=32, width=32, **CFG)


def _video():
    """Two shots of 24 x 40 frames, 8 and 12 long."""
    return S.fixture((CUT, F20 - CUT), *SRC)


def _resident(sess, bgr, mode="newest", keep=True):
    sess.open_video(len(bgr), mode)
    if keep:
        sess.video_keep_source(True)
    sess.video_put_u8(0, bgr[:7])
    sess.video_put_u8(7, bgr[7:])
    sess.video_predict([0, 2, 4])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("mode", ["newest", "mean"])
def test_detect_install_read_remove(mode):
    from sap3d_tensorflow_amd import dataflow
    bgr = _video()
    sess = _session()
    _resident(sess, bgr, mode)
    assert sess.video_shots() is None
    plain = sess.video_maps(0, F20)
    sess.set_video_temporal("gauss", 1.5, 3, 0.0)
    no_table = sess.video_maps(0, F20)
    no_table_u8 = sess.video_maps_u8(0, F20, size=SRC)
    no_table_track = sess.video_reframe(0, F20, CROP, gate=10, smooth=3, with_raw=True, with_mass=True)
    # the cut is found, on the device, and nothing is installed unless asked for
    for grid in ((1, 1), (2, 3), (4, 4)):
        starts, D = sess.video_detect_shots(grid, install=False, with_signal=True, **RULE)
        assert starts.tolist() == [0, CUT] and np.array_equal(D, S.distances(bgr, *grid))
        assert sess.video_shots() is None
    ms = sess.video_shots_last_ms()
    assert ms["signal"] > 0.0 and ms["decision"] > 0.0
    assert sess.video_detect_shots((2, 2), **RULE).tolist() == [0, CUT]
    assert sess.video_shots().tolist() == [0, CUT]
    # the temporal stage inside the shots: the op-level filter on the unfiltered maps
    want = dataflow.temporal_filter(plain, "gauss", 1.5, 3, shots=[0, CUT])
    assert np.array_equal(bits(sess.video_maps(0, F20)), bits(want))
    assert not np.array_equal(bits(want), bits(no_table))
    assert np.array_equal(bits(sess.video_maps(5, 9)), bits(want[5:14]))
    u8 = sess.video_maps_u8(0, F20, size=SRC)
    assert not np.array_equal(u8, no_table_u8)
    # the reframe track inside the shots, on those bytes; a part of the video sees the part of the table that falls into it
    res = sess.video_reframe(0, F20, CROP, gate=10, smooth=3, with_raw=True, with_mass=True, with_maps=True)
    assert np.array_equal(res["maps"], u8)
    wt = S.reframe_shots(u8, bgr, *CROP, 10, 3, [0, CUT])
    assert np.array_equal(res["track"], wt[0]) and np.array_equal(res["raw"], wt[1]) and np.array_equal(res["mass"], wt[2])
    assert np.array_equal(res["crop"], wt[3])
    part = sess.video_reframe(5, 9, CROP, frames=False, size=SRC, smooth=2, with_raw=True, with_mass=True)
    wp = S.reframe_shots(u8[5:14], None, *CROP, 0, 2, [0, CUT - 5])
    assert np.array_equal(part["track"], wp[0]) and np.array_equal(part["mass"], wp[2])
    late = sess.video_reframe(CUT, 5, CROP, frames=False, size=SRC, smooth=2, with_raw=True)      # one shot only
    assert np.array_equal(late["track"], F.reframe(u8[CUT:CUT + 5], None, *CROP, 0, 2)[0])
    # the moving average restarts
    sess.set_video_temporal("ema", 0., 0, 0.7)
    assert np.array_equal(bits(sess.video_maps(0, F20)), bits(dataflow.temporal_filter(plain, "ema", alpha=0.7, shots=[0, CUT])))
    assert np.array_equal(bits(sess.video_maps(CUT, 1)), bits(plain[CUT:CUT + 1]))
    # a radius beyond F - 1 is legal under a table, and refused without one
    sess.set_video_temporal("gauss", 3.0, 24, 0.0)
    assert np.array_equal(bits(sess.video_maps(0, F20)), bits(dataflow.temporal_filter(plain, "gauss", 3.0, 24, shots=[0, CUT])))
    sess.set_video_temporal("gauss", 1.5, 3, 0.0)
    # another table by hand; then none: what was returned before
    sess.video_set_shots([0, 1, 3, 12])
    assert sess.video_shots().tolist() == [0, 1, 3, 12]
    assert np.array_equal(bits(sess.video_maps(0, F20)), bits(dataflow.temporal_filter(plain, "gauss", 1.5, 3, shots=[0, 1, 3, 12])))
    sess.video_set_shots(None)
    assert sess.video_shots() is None
    assert np.array_equal(bits(sess.video_maps(0, F20)), bits(no_table))
    assert np.array_equal(sess.video_maps_u8(0, F20, size=SRC), no_table_u8)
    again = sess.video_reframe(0, F20, CROP, gate=10, smooth=3, with_raw=True, with_mass=True)
    for k in ("track", "raw", "mass", "crop"):
        assert np.array_equal(again[k], no_table_track[k])
    # open_video clears it
    sess.video_set_shots([0, CUT])
    _resident(sess, bgr, mode)
    assert sess.video_shots() is None
    assert np.array_equal(bits(sess.video_maps(0, F20)), bits(no_table))
    sess.close_video()
    sess.close()


def test_score_and_render_do_not_read_the_table():
    from sap3d_tensorflow_amd import dataflow
    bgr = _video()
    sess = _session()
    _resident(sess, bgr)
    den = F.blobs(F20, *SRC, seed=4)
    fix = np.where(np.random.default_rng(1).random(den.shape) < 0.02, 255, 0).astype(np.uint8)
    table = dataflow.render_table("jet", 0.6, "ramp", gate=20)
    sc = sess.video_score(0, F20, den, fix, size=SRC, columns=("cc", "sim", "judd", "kl", "nss"))
    rn = sess.video_render(0, F20, table=table)
    sess.video_set_shots([0, CUT])
    assert np.array_equal(sess.video_score(0, F20, den, fix, size=SRC, columns=("cc", "sim", "judd", "kl", "nss")), sc, equal_nan=True)
    assert np.array_equal(sess.video_render(0, F20, table=table), rn)
    sess.close_video()
    sess.close()


def test_refusals_change_nothing():
    from sap3d_tensorflow_amd import P3dError
    bgr = _video()
    sess = _session()
    with pytest.raises(P3dError):
        sess.video_set_shots([0])                           # no open video
    _resident(sess, bgr, keep=False)
    with pytest.raises(P3dError) as e:
        sess.video_detect_shots((2, 2), **RULE)
    assert "keeps no source" in str(e.value) and sess.video_shots() is None
    for starts, word in (([1, 5], "frame 0"), ([0, 5, 5], "ascend"), ([0, F20], "outside"), ([], "shots")):
        with pytest.raises(P3dError) as e:
            sess.video_set_shots(starts)
        assert word in str(e.value) and sess.video_shots() is None
    sess.video_set_shots([0, CUT])
    with pytest.raises(P3dError):
        sess.video_set_shots([0, 3, 2])
    assert sess.video_shots().tolist() == [0, CUT]
    # a source with a frame that was put as floats: the error names it
    sess.open_video(F20, "newest")
    sess.video_keep_source(True)
    sess.video_put_u8(0, bgr[:7])
    sess.video_put_u8(8, bgr[8:])
    with pytest.raises(P3dError) as e:
        sess.video_detect_shots((2, 2), **RULE)
    assert "frame 7" in str(e.value)
    sess.video_put_u8(7, bgr[7:8])
    for kw, word in ((dict(grid=(5, 1)), "grid"), (dict(threshold=0), "threshold"), (dict(window=33), "window"), (dict(ratio=255), "ratio"), (dict(min_length=0), "minimum length")):
        rule = dict(RULE)
        grid = kw.pop("grid", (2, 2))
        rule.update(kw)
        with pytest.raises(P3dError) as e:
            sess.video_detect_shots(grid, **rule)
        assert word in str(e.value) and sess.video_shots() is None
    assert sess.video_detect_shots((2, 2), **RULE).tolist() == [0, CUT]
    sess.close_video()
    sess.close()
