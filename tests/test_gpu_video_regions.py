"""p3d_video_regions on a resident video (P3DSession.video_regions): records, counts and label maps are tests/regions_ref.py's on
video_maps_u8's bytes, exactly, with and without a shot table; the other read-outs return what they returned before it; refusals
change nothing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import reframe_ref as F        # noqa: E402
import regions_ref as rr       # noqa: E402

CFG = dict(base=16, blocks=(2, 2, 3))
F20, T, SRC = 20, 16, (24, 40)


def _session():
    from sap3d_tensorflow_amd import P3DSession
    return P3DSession("unet", seed=2, batch=3, frames=T, height=32, width=32, **CFG)


def _video(seed=0):
    rng = np.random.default_rng(seed)
    sal = F.blobs(F20, *SRC, seed=seed + 11)
    return np.clip(rng.integers(0, 120, (F20,) + SRC + (3,)) + sal[..., None] // 2, 0, 255).astype(np.uint8)


def _resident(sess, bgr, mode="newest"):
    sess.open_video(len(bgr), mode)
    sess.video_keep_source(True)
    sess.video_put_u8(0, bgr)
    sess.video_predict([0, 2, 4])


def _gate(maps):
    """A level that leaves about a fifth of the pixels in the foreground: several regions a frame on a random net's maps."""
    return max(1, int(np.percentile(maps, 80)))


def _same(res, want):
    assert res["regions"].dtype == np.int32 and res["counts"].dtype == np.int32
    assert np.array_equal(res["counts"], want[1]), (res["counts"][:4].tolist(), want[1][:4].tolist())
    assert np.array_equal(res["regions"], want[0])
    if "labels" in res:
        assert np.array_equal(res["labels"], want[2])


@pytest.mark.parametrize("setting", ["newest", "mean, blur, range"])
def test_regions_are_the_replay_on_the_bytes_of_video_maps_u8(setting):
    sess = _session()
    if "blur" in setting:
        sess.set_postprocess(1.5, 0, "range")
    _resident(sess, _video(), setting.split(",")[0])
    before = sess.video_maps_u8(0, F20, size=SRC)
    assert before.max() > before.min()
    g = _gate(before)
    res = sess.video_regions(0, F20, SRC, g, max_regions=6, link=True, with_labels=True, with_maps=True, timed=True)
    assert np.array_equal(res["maps"], before)
    want = rr.regions(before, g, 8, 1, 6, True)
    assert want[1][:, 0].max() >= 2
    _same(res, want)
    assert set(sess.last_regions_ms) == {"device", "regions"} and sess.last_regions_ms["regions"] > 0.0 and sess.last_regions_ms["device"] > 0.0
    print(setting, "gate", g, "counts", res["counts"][::5].tolist())
    # a part of the video is a world of its own for the link; other settings; no labels
    part = sess.video_regions(5, 9, SRC, g, connectivity=4, min_area=3, max_regions=3, link=True)
    assert set(part) == {"regions", "counts"}
    _same(part, rr.regions(before[5:14], g, 4, 3, 3, True))
    # another size, link off
    size = (45, 23)
    maps2 = sess.video_maps_u8(2, 6, size=size)
    res2 = sess.video_regions(2, 6, size, _gate(maps2), with_labels=True, with_maps=True)
    assert np.array_equal(res2["maps"], maps2) and res2["regions"].shape == (6, 64, rr.FIELDS)
    _same(res2, rr.regions(maps2, _gate(maps2)))
    # under a shot table: the link starts anew at every start inside the range, cut as video_reframe cuts it
    sess.video_set_shots([0, 4, 8, 15])
    shots = sess.video_regions(0, F20, SRC, g, max_regions=6, link=True, with_labels=True)
    _same(shots, rr.regions(before, g, 8, 1, 6, True, shots=[0, 4, 8, 15]))
    assert not np.array_equal(shots["regions"], res["regions"])
    part = sess.video_regions(5, 9, SRC, g, max_regions=6, link=True)
    _same(part, rr.regions(before[5:14], g, 8, 1, 6, True, shots=[0, 3]))
    assert np.array_equal(sess.video_maps_u8(0, F20, size=SRC), before)
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
    ref = sess.video_reframe(0, F20, (24, 14), smooth=2, with_raw=True, with_mass=True)
    sess.video_regions(0, F20, SRC, _gate(u8), link=True, with_labels=True)
    sess.video_regions(4, 3, (30, 50), 1, connectivity=4, max_regions=1)
    assert np.array_equal(sess.video_maps_u8(0, F20, size=SRC), u8)
    assert np.array_equal(sess.video_score(0, F20, den, fix, size=SRC, columns=cols).view(np.uint64), sc.view(np.uint64))
    assert np.array_equal(sess.video_render(0, F20, table=table, contour=120, thickness=2), img)
    again = sess.video_reframe(0, F20, (24, 14), smooth=2, with_raw=True, with_mass=True)
    assert all(np.array_equal(again[k], ref[k]) for k in ("track", "raw", "mass", "crop"))
    sess.close_video()
    sess.close()


def test_refusals_change_nothing():
    from sap3d_tensorflow_amd import P3dError, dataflow
    from sap3d_tensorflow_amd._lib import lib
    sess = _session()
    bgr = _video(seed=5)
    with pytest.raises(P3dError, match="no video is open"):
        sess.video_regions(0, 1, SRC, 1)
    sess.open_video(F20, "newest")                                    # frames 16 .. 19 stay unpredicted
    sess.video_put_u8(0, bgr)
    sess.video_predict([0])
    before = sess.video_maps_u8(0, 16, size=SRC)
    g = _gate(before)
    want = rr.regions(before[:9], g, 8, 1, 5, True)

    def valid():
        _same(sess.video_regions(0, 9, SRC, g, max_regions=5, link=True, with_labels=True), want)
        assert np.array_equal(sess.video_maps_u8(0, 16, size=SRC), before)

    valid()
    for bad, word in ((dict(gate=0), "gate"), (dict(gate=256), "gate"), (dict(gate=g, connectivity=6), "connectivity"),
                      (dict(gate=g, max_regions=0), "max_regions"), (dict(gate=g, max_regions=65), "max_regions"), (dict(gate=g, min_area=0), "area")):
        with pytest.raises(P3dError, match=word):
            sess.video_regions(0, 4, SRC, **bad)
        valid()
    with pytest.raises(P3dError, match="2\\^23"):
        sess.video_regions(0, 1, (2 ** 12, 2 ** 11 + 1), g)
    valid()
    cfg = dataflow.regions_cfg(g)
    counts = np.zeros((4, 3), np.int32)
    assert lib().p3d_video_regions(sess._h, 0, 4, 255.0, SRC[0], SRC[1], cfg, None, counts.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None) != 0
    assert not counts.any()
    valid()
    with pytest.raises(P3dError, match="frame 16"):
        sess.video_regions(10, 8, SRC, g)                             # an unpredicted frame
    valid()
    with pytest.raises(P3dError, match="outside"):
        sess.video_regions(19, 2, SRC, g)
    valid()
    sess.close_video()
    sess.close()
