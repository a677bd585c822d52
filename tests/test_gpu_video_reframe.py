"""p3d_video_reframe on a resident video (P3DSession.video_reframe): tracks, masses and crop are tests/reframe_ref.py's on
video_maps_u8's bytes and the frames as they were put, exactly, with the kept source and with host frames, under every read-out
setting the maps follow; the other read-outs return what they returned before it; refusals change nothing."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import reframe_ref as F        # noqa: E402

CFG = dict(base=16, blocks=(2, 2, 3))
F20, T, SRC = 20, 16, (24, 40)
CROP = (24, 14)                # 9:16 of the frame's height, even


def _session():
    from sap3d_tensorflow_amd import P3DSession
    return P3DSession("unet", seed=2, batch=3, frames=T, height=32, width=32, **CFG)


def _video(seed=0):
    """20 frames of 24 x 40 in B, G, R order: a bright blob that moves, on noise."""
    rng = np.random.default_rng(seed)
    sal = F.blobs(F20, *SRC, seed=seed + 11)
    return np.clip(rng.integers(0, 120, (F20,) + SRC + (3,)) + sal[..., None] // 2, 0, 255).astype(np.uint8)


def _resident(sess, bgr, mode="newest", keep=True):
    sess.open_video(len(bgr), mode)
    if keep:
        sess.video_keep_source(True)
    sess.video_put_u8(0, bgr[:7])
    sess.video_put_u8(7, bgr[7:])
    sess.video_predict([0, 2, 4])


def _same(res, want, crop=True):
    assert np.array_equal(res["track"], want[0]) and np.array_equal(res["raw"], want[1]) and np.array_equal(res["mass"], want[2])
    if crop:
        assert res["crop"].dtype == np.uint8 and np.array_equal(res["crop"], want[3])
    else:
        assert res["crop"] is None


@pytest.mark.parametrize("setting", ["newest", "mean", "newest, temporal", "mean, blur, range"])
def test_reframing_is_the_replay_on_the_bytes_of_video_maps_u8(setting):
    sess = _session()
    if "temporal" in setting:
        sess.set_video_temporal("gauss", 1.0, 0, 0.0)
    if "blur" in setting:
        sess.set_postprocess(1.5, 0, "range")
    bgr = _video()
    _resident(sess, bgr, setting.split(",")[0])
    info = sess.video_source_info()
    assert info == dict(on=True, size=SRC, bytes=F20 * SRC[0] * SRC[1] * 3)
    before = sess.video_maps_u8(0, F20, size=SRC)
    assert before.max() > before.min()
    # the kept source, every frame, smoothed; the maps come back too
    res = sess.video_reframe(0, F20, CROP, gate=10, smooth=3, with_raw=True, with_mass=True, with_maps=True, timed=True)
    assert np.array_equal(res["maps"], before)
    _same(res, F.reframe(before, bgr, *CROP, 10, 3))
    assert res["crop"].shape == (F20,) + CROP + (3,)
    assert set(sess.last_reframe_ms) == {"upload", "device", "reframe"} and sess.last_reframe_ms["upload"] == 0.0
    assert sess.last_reframe_ms["reframe"] > 0.0 and sess.last_reframe_ms["device"] > 0.0
    print(setting, "raw track", res["raw"][::4].tolist(), "smoothed", res["track"][::4].tolist())
    # a part of the video is a world of its own for the filter; the defaults: no gate, the raw track
    part = sess.video_reframe(5, 9, (10, 16), smooth=2, with_raw=True, with_mass=True)
    _same(part, F.reframe(before[5:14], bgr[5:14], 10, 16, 0, 2))
    plain = sess.video_reframe(5, 9, (10, 16))
    assert set(plain) == {"track", "crop"} and np.array_equal(plain["track"], part["raw"])
    # the tracks alone, at the source's size and at another
    only = sess.video_reframe(0, F20, CROP, frames=False, size=SRC, gate=10, smooth=3, with_raw=True, with_mass=True)
    _same(only, F.reframe(before, None, *CROP, 10, 3), crop=False)
    size = (45, 23)
    maps2 = sess.video_maps_u8(2, 6, size=size)
    only = sess.video_reframe(2, 6, (20, 9), frames=False, size=size, smooth=1, with_raw=True, with_mass=True, with_maps=True)
    assert np.array_equal(only["maps"], maps2)
    _same(only, F.reframe(maps2, None, 20, 9, 0, 1), crop=False)
    # host frames, at the source's size and at another one
    other = F.frames_for(before[3:8], seed=5)
    res = sess.video_reframe(3, 5, CROP, frames=other, smooth=1, with_raw=True, with_mass=True, timed=True)
    _same(res, F.reframe(before[3:8], other, *CROP, 0, 1))
    assert sess.last_reframe_ms["upload"] > 0.0
    fr2 = F.frames_for(maps2, seed=6)
    res = sess.video_reframe(2, 6, (20, 9), frames=fr2, size=size, gate=128, smooth=255, with_raw=True, with_mass=True)
    _same(res, F.reframe(maps2, fr2, 20, 9, 128, 255))
    # the read-outs are what they were
    assert np.array_equal(sess.video_maps_u8(0, F20, size=SRC), before)
    assert sess.video_source_info() == info
    sess.close_video()
    sess.close()


def test_the_other_readouts_return_what_they_returned_before():
    from sap3d_tensorflow_amd import dataflow
    bgr = _video(seed=3)
    sess = _session()
    _resident(sess, bgr, "mean")
    rng = np.random.default_rng(1)
    den = F.blobs(F20, *SRC, seed=4)
    fix = np.where(rng.random(den.shape) < 0.02, 255, 0).astype(np.uint8)
    table = dataflow.render_table("jet", 0.6, "ramp", gate=20)
    cols = ("cc", "sim", "judd", "kl", "nss")
    u8 = sess.video_maps_u8(0, F20, size=SRC)
    sc = sess.video_score(0, F20, den, fix, size=SRC, columns=cols)
    img = sess.video_render(0, F20, table=table, contour=120, thickness=2)
    sess.video_reframe(0, F20, CROP, smooth=2)
    sess.video_reframe(4, 3, (5, 40), frames=bgr[4:7], gate=200)
    sess.video_reframe(4, 3, (5, 40), frames=False, size=(30, 50))
    assert np.array_equal(sess.video_maps_u8(0, F20, size=SRC), u8)
    assert np.array_equal(sess.video_score(0, F20, den, fix, size=SRC, columns=cols).view(np.uint64), sc.view(np.uint64))
    assert np.array_equal(sess.video_render(0, F20, table=table, contour=120, thickness=2), img)
    sess.close_video()
    sess.close()


def test_refusals_change_nothing():
    from sap3d_tensorflow_amd import P3dError, dataflow
    sess = _session()
    bgr = _video(seed=5)
    with pytest.raises(P3dError, match="no video is open"):
        sess.video_reframe(0, 1, (2, 2), frames=bgr[:1])
    # frames 16 .. 19 stay unpredicted; frame 9 is put again as floats and loses its source
    sess.open_video(F20, "newest")
    sess.video_keep_source(True)
    sess.video_put_u8(0, bgr)
    sess.video_predict([0])
    info = sess.video_source_info()
    before = sess.video_maps_u8(0, 16, size=SRC)
    want = F.reframe(before[:9], bgr[:9], *CROP, 0, 2)

    def valid():
        assert sess.video_source_info() == info
        _same(sess.video_reframe(0, 9, CROP, smooth=2, with_raw=True, with_mass=True), want)

    valid()
    with pytest.raises(P3dError, match="kept source is 24 x 40"):
        sess.video_reframe(0, 4, (8, 8), size=(48, 40))               # a size other than the kept source's
    valid()
    for bad, word in ((dict(crop=(25, 8)), "window"), (dict(crop=(8, 41)), "window"), (dict(crop=(0, 8)), "window"),
                      (dict(crop=(8, 8), gate=256), "gate"), (dict(crop=(8, 8), gate=-1), "gate"), (dict(crop=(8, 8), smooth=256), "radius"),
                      (dict(crop=(8, 8), smooth=-1), "radius")):
        with pytest.raises(P3dError, match=word):
            sess.video_reframe(0, 4, **bad)
        valid()
    with pytest.raises(P3dError, match="frame 16"):
        sess.video_reframe(10, 8, CROP)                               # an unpredicted frame
    valid()
    with pytest.raises(P3dError, match="outside"):
        sess.video_reframe(19, 2, CROP)
    with pytest.raises(P3dError, match="2\\^23"):
        sess.video_reframe(0, 1, (2, 2), frames=False, size=(2 ** 12, 2 ** 11 + 1))
    valid()
    sess.video_put(9, dataflow.mapf_frames(bgr[9:10], 32))            # floats have no source
    with pytest.raises(P3dError, match="frame 9 has no source"):
        sess.video_reframe(8, 4, CROP)
    valid()
    res = sess.video_reframe(9, 1, CROP, frames=bgr[9:10], with_raw=True, with_mass=True)     # host frames, and the tracks alone, still work
    _same(res, F.reframe(before[9:10], bgr[9:10], *CROP))
    only = sess.video_reframe(8, 4, CROP, frames=False, size=SRC, with_raw=True, with_mass=True)
    _same(only, F.reframe(before[8:12], None, *CROP), crop=False)
    # a video without the store: host frames and the tracks alone work, the kept source is refused
    sess.open_video(F20, "newest")
    sess.video_put_u8(0, bgr)
    sess.video_predict([0])
    with pytest.raises(P3dError, match="keeps no source"):
        sess.video_reframe(0, 4, CROP, size=SRC)
    with pytest.raises(P3dError, match="keeps no source"):
        sess.video_reframe(0, 4, CROP)                                # the size left to a source that is not there
    _same(sess.video_reframe(0, 9, CROP, frames=bgr[:9], smooth=2, with_raw=True, with_mass=True), want)
    sess.close_video()
    sess.close()
