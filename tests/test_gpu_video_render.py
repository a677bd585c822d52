"""p3d_video_render on a resident video (P3DSession.video_render): the overlay is tests/render_ref.py's on video_maps_u8's bytes and
the frames as they were put, exactly, with the kept source and with host frames, under every read-out setting the maps follow; the
source store changes nothing it does not own; refusals change nothing."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import render_ref as R        # noqa: E402

CFG = dict(base=16, blocks=(2, 2, 3))
F18, T, SRC = 18, 16, (36, 52)
LINE = dict(contour=120, thickness=2, contour_color=(10, 200, 30))      # (R, G, B)
LINE_REF = (120, 2, (30, 200, 10))


def _session():
    from sap3d_tensorflow_amd import P3DSession
    return P3DSession("unet", seed=2, batch=3, frames=T, height=32, width=32, **CFG)


def _video(seed=0):
    """18 frames of 36 x 52 in B, G, R order: a bright blob that moves, on noise."""
    rng = np.random.default_rng(seed)
    sal = R.blob(F18, *SRC, seed=seed + 11)
    return np.clip(rng.integers(0, 120, (F18,) + SRC + (3,)) + sal[..., None] // 2, 0, 255).astype(np.uint8)


def _resident(sess, bgr, mode="newest", keep=True):
    sess.open_video(len(bgr), mode)
    if keep:
        sess.video_keep_source(True)
    sess.video_put_u8(0, bgr[:7])
    sess.video_put_u8(7, bgr[7:])
    sess.video_predict([0, 1, 2])


def _table():
    from sap3d_tensorflow_amd import dataflow
    return dataflow.render_table("jet", 0.6, "ramp", gate=20)


@pytest.mark.parametrize("setting", ["newest", "mean", "newest, temporal", "mean, blur, range"])
def test_overlay_is_the_replay_on_the_bytes_of_video_maps_u8(setting):
    sess = _session()
    if "temporal" in setting:
        sess.set_video_temporal("gauss", 1.0, 0, 0.0)
    if "blur" in setting:
        sess.set_postprocess(1.5, 0, "range")
    bgr = _video()
    _resident(sess, bgr, setting.split(",")[0])
    info = sess.video_source_info()
    assert info == dict(on=True, size=SRC, bytes=F18 * SRC[0] * SRC[1] * 3)
    table = _table()
    before = sess.video_maps_u8(0, F18, size=SRC)
    assert before.max() > before.min()
    # the kept source, every frame, with a contour; the maps come back too
    got, maps = sess.video_render(0, F18, table=table, with_maps=True, timed=True, **LINE)
    assert np.array_equal(maps, before)
    want = R.render(before, bgr, table, *LINE_REF)
    assert got.dtype == np.uint8 and got.shape == (F18,) + SRC + (3,) and np.array_equal(got, want), setting
    assert set(sess.last_render_ms) == {"upload", "device", "render"} and sess.last_render_ms["upload"] == 0.0
    assert sess.last_render_ms["render"] > 0.0 and sess.last_render_ms["device"] > 0.0
    m = R.contour_mask(before, LINE_REF[0], LINE_REF[1])
    print(setting, "contour pixels", int(m.sum()), "of", int((before >= LINE_REF[0]).sum()), "at or above the level")
    # a part of the video, no contour, the defaults' table
    from sap3d_tensorflow_amd import dataflow
    part = sess.video_render(5, 9)
    assert np.array_equal(part, R.render(before[5:14], bgr[5:14], dataflow.render_table("jet", 0.6, "ramp")))
    # host frames, at the source's size and at another one
    other = R.frames_for(before[3:8], seed=5)
    got = sess.video_render(3, 5, frames=other, table=table, timed=True, **LINE)
    assert np.array_equal(got, R.render(before[3:8], other, table, *LINE_REF))
    assert sess.last_render_ms["upload"] > 0.0
    size = (45, 23)
    maps2 = sess.video_maps_u8(2, 4, size=size)
    fr2 = R.frames_for(maps2, seed=6)
    got, back = sess.video_render(2, 4, frames=fr2, size=size, table=table, with_maps=True, **LINE)
    assert np.array_equal(back, maps2) and np.array_equal(got, R.render(maps2, fr2, table, *LINE_REF))
    # the read-outs are what they were
    assert np.array_equal(sess.video_maps_u8(0, F18, size=SRC), before)
    assert sess.video_source_info() == info
    sess.close_video()
    sess.close()


def test_a_kept_source_off_the_16_byte_boundary():
    """35 x 51 source frames are 5355 bytes each: from frame 1 on the kept source starts 11, 6, 1, ... bytes past a 16-byte boundary
    while the maps and the images of a call start on one, so the frame is aligned unlike the other two and every pixel goes
    single.  Frame 16 of that video is aligned again (whole words), and a call of several frames has both."""
    odd = (35, 51)
    rng = np.random.default_rng(8)
    bgr = rng.integers(0, 256, (F18,) + odd + (3,), dtype=np.uint8)
    sess = _session()
    _resident(sess, bgr)
    assert sess.video_source_info()["size"] == odd
    table = _table()
    maps = sess.video_maps_u8(0, F18, size=odd)
    for first, n in ((1, 1), (3, 5), (16, 2), (0, F18)):
        assert (first * odd[0] * odd[1] * 3 % 16 != 0) == (first not in (0, 16))
        for line, ref in ((dict(), ()), (LINE, LINE_REF)):
            got = sess.video_render(first, n, table=table, **line)
            assert np.array_equal(got, R.render(maps[first:first + n], bgr[first:first + n], table, *ref)), (first, n, line)
    sess.close_video()
    sess.close()


def test_the_source_store_leaves_frames_maps_and_scores_alone():
    """The stored floats have no getter; every map is a function of them, so the float maps of a video put with the store on, with
    it off and as floats of dataflow.mapf_frames must agree bit for bit.  video_maps_u8 and video_score return the same bytes
    before and after a render."""
    from sap3d_tensorflow_amd import dataflow
    bgr = _video(seed=3)
    sess = _session()
    maps = {}
    for keep in (True, False):
        _resident(sess, bgr, "mean", keep)
        assert sess.video_source_info()["on"] == keep and (sess.video_source_info()["bytes"] > 0) == keep
        maps[keep] = sess.video_maps(0, F18)
    sess.open_video(F18, "mean")
    assert sess.video_source_info() == dict(on=False, size=(0, 0), bytes=0)      # every open starts with it off
    sess.video_put(0, dataflow.mapf_frames(bgr, 32))
    sess.video_predict([0, 1, 2])
    floats = sess.video_maps(0, F18)
    assert np.array_equal(maps[True].view(np.uint32), maps[False].view(np.uint32))
    assert np.array_equal(maps[True].view(np.uint32), floats.view(np.uint32))
    # scores and bytes around a render
    _resident(sess, bgr, "mean", True)
    rng = np.random.default_rng(1)
    den = R.blob(F18, *SRC, seed=4)
    fix = np.where(rng.random(den.shape) < 0.02, 255, 0).astype(np.uint8)
    u8 = sess.video_maps_u8(0, F18, size=SRC)
    sc, scored = sess.video_score(0, F18, den, fix, size=SRC, columns=("cc", "sim", "judd", "kl", "nss"), with_maps=True)
    sess.video_render(0, F18, table=_table(), **LINE)
    sess.video_render(4, 3, frames=bgr[4:7], table=_table())
    assert np.array_equal(sess.video_maps_u8(0, F18, size=SRC), u8) and np.array_equal(scored, u8)
    sc2, scored2 = sess.video_score(0, F18, den, fix, size=SRC, columns=("cc", "sim", "judd", "kl", "nss"), with_maps=True)
    assert np.array_equal(sc.view(np.uint64), sc2.view(np.uint64)) and np.array_equal(scored2, u8)
    sess.close_video()
    sess.close()


def test_refusals_change_nothing():
    from sap3d_tensorflow_amd import P3dError, dataflow
    sess = _session()
    bgr = _video(seed=5)
    table = _table()
    with pytest.raises(P3dError, match="no video is open"):
        sess.video_render(0, 1, frames=bgr[:1], table=table)
    with pytest.raises(P3dError, match="no video is open"):
        sess.video_keep_source(True)
    with pytest.raises(P3dError, match="no video is open"):
        sess.video_source_info()
    # frames 16 and 17 stay unpredicted; frame 9 is put again as floats and loses its source
    sess.open_video(F18, "newest")
    sess.video_keep_source(True)
    sess.video_keep_source(False)
    sess.video_keep_source(True)                      # legal until the first put
    sess.video_put_u8(0, bgr)
    sess.video_predict([0])
    info = sess.video_source_info()
    before = sess.video_maps_u8(0, 16, size=SRC)
    want = R.render(before[:9], bgr[:9], table, *LINE_REF)

    def valid():
        assert sess.video_source_info() == info
        assert np.array_equal(sess.video_render(0, 9, table=table, **LINE), want)

    valid()
    with pytest.raises(P3dError, match="already put"):
        sess.video_keep_source(False)                 # toggled after a put
    valid()
    with pytest.raises(P3dError, match="36 x 52"):
        sess.video_put_u8(3, np.zeros((2, 40, 52, 3), np.uint8))      # a second source size
    valid()
    with pytest.raises(P3dError, match="kept source is 36 x 52"):
        sess.video_render(0, 4, size=(48, 40), table=table)           # a size mismatch with the kept source
    valid()
    for bad in (dict(contour=100, thickness=0), dict(contour=100, thickness=5), dict(contour=256)):
        with pytest.raises(P3dError, match="thickness|level"):
            sess.video_render(0, 4, table=table, **bad)
        valid()
    with pytest.raises(P3dError, match="frame 16"):
        sess.video_render(10, 8, table=table)                         # an unpredicted frame
    valid()
    with pytest.raises(P3dError, match="outside"):
        sess.video_render(17, 2, table=table)
    with pytest.raises(P3dError, match="2\\^28"):
        sess.video_render(0, 1, frames=np.zeros((1, 2 ** 14, 2 ** 14 + 1, 3), np.uint8), table=table)
    valid()
    sess.video_put(9, dataflow.mapf_frames(bgr[9:10], 32))            # floats have no source
    with pytest.raises(P3dError, match="frame 9 has no source"):
        sess.video_render(8, 4, table=table)
    valid()
    assert np.array_equal(sess.video_render(9, 1, frames=bgr[9:10], table=table), R.render(before[9:10], bgr[9:10], table))
    # a video without the store: host frames still render, the kept source is refused
    sess.open_video(F18, "newest")
    sess.video_put_u8(0, bgr)
    sess.video_predict([0])
    with pytest.raises(P3dError, match="keeps no source"):
        sess.video_render(0, 4, size=SRC, table=table)
    with pytest.raises(P3dError, match="keeps no source"):
        sess.video_render(0, 4, table=table)                          # the size left to a source that is not there
    assert np.array_equal(sess.video_render(0, 9, frames=bgr[:9], table=table, **LINE), want)
    sess.close_video()
    sess.close()
