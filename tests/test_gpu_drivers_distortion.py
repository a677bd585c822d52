"""p3d_video_distortion on a resident video (P3DSession.video_distortion): the table and the block map are p3d_distortion_u8's, and
tests/distortion_ref.py's, on video_maps_u8's bytes and the put frames -- from the kept source and from an explicit reference, over a
part of the video -- and the maps, the render and the pre-filter read the same before and after; the pre-filter's own output changes
no salient pixel where its strength is 0 around it; refusals change nothing; and drivers/gen_pred.py --resident --distortion DIR end
to end on a small synthetic video, in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import distortion_ref as dr    # noqa: E402
import prefilter_ref as pr     # noqa: E402
import reframe_ref as F        # noqa: E402

SRC = (24, 40)
F20, T = 20, 16


def _video(n, seed):
    rng = np.random.default_rng(seed)
    return np.clip(rng.integers(0, 120, (n,) + SRC + (3,)) + F.blobs(n, *SRC, seed=3 + seed)[..., None] // 2, 0, 255).astype(np.uint8)


def _session():
    from sap3d_tensorflow_amd import P3DSession
    sess = P3DSession("unet", seed=2, batch=3, frames=T, height=32, width=32, base=16, blocks=(1, 1, 1))
    sess.set_postprocess(0., 0, "range")
    return sess


def test_distortion_is_the_op_on_the_bytes_of_video_maps_u8():
    from sap3d_tensorflow_amd import dataflow
    sess = _session()
    sess.open_video(F20, "mean")
    sess.video_keep_source(True)
    video = _video(F20, 0)
    sess.video_put_u8(0, video)
    sess.video_predict([0, 2, 4])
    before = sess.video_maps_u8(0, F20, size=SRC)
    seen = sess.video_render(0, F20)
    assert before.max() > before.min()
    gate = int(np.percentile(before, 60)) + 1
    law = dataflow.distortion_law(gate=gate, gamma=0.8, floor=1)
    test = dr.near(video, 9)
    # the whole video against the kept source
    table, bs, maps, ms = sess.video_distortion(0, F20, test, law, block=8, gate=gate)
    assert np.array_equal(maps, before)
    op_table, op_bs = dataflow.distortion(before, video, test, (8, gate), law)
    want_table, want_bs = dr.distortion(before, video, test, law, block=8, gate=gate)
    assert table.dtype == np.int64 and np.array_equal(table, op_table) and np.array_equal(table, want_table)
    assert bs.dtype == np.int64 and np.array_equal(bs, op_bs) and np.array_equal(bs, want_bs)
    assert (table[:, dr.SALIENT] > 0).any() and (table[:, dr.NW] == 5 * 9).all() and (table[:, dr.SSE:dr.SSE + 4] > 0).all()
    assert set(ms) == {"upload", "device", "distortion"} and ms["upload"] > 0.0 and ms["distortion"] > 0.0 and ms["device"] > 0.0
    # an explicit reference gives what the kept source gives; a part of the video is that part of the table
    again = sess.video_distortion(0, F20, test, law, block=8, gate=gate, ref=video)
    assert np.array_equal(again[0], table) and np.array_equal(again[1], bs) and np.array_equal(again[2], before)
    part = sess.video_distortion(5, 9, test[5:14], law, gate=gate)
    assert np.array_equal(part[0], table[5:14]) and part[1] is None and np.array_equal(part[2], before[5:14])
    other = _video(9, 7)
    assert np.array_equal(sess.video_distortion(5, 9, test[5:14], law, gate=gate, ref=other)[0],
                          dr.distortion(before[5:14], other, test[5:14], law, gate=gate)[0])
    rep = dataflow.distortion_report(table, SRC[0] * SRC[1])
    assert np.isfinite(rep["psnr"]).all() and (rep["ssim"] > 0).all() and (rep["ssim"] < 1).all()
    # every other entry point returns the same bits
    assert np.array_equal(sess.video_maps_u8(0, F20, size=SRC), before) and np.array_equal(sess.video_render(0, F20), seen)
    sess.close_video()
    sess.close()


def test_the_prefilter_changes_no_salient_pixel_where_its_strength_is_0():
    """video_prefilter's output fed back as `test`, the same gate, a weight law that is 0 from the gate on: against the replay's
    numbers.  Where the strength grid is 0 at the (up to) four blocks a pixel's weight interpolates between, the pixel is unchanged."""
    from sap3d_tensorflow_amd import dataflow
    sess = _session()
    sess.open_video(F20, "mean")
    sess.video_keep_source(True)
    video = _video(F20, 1)
    sess.video_put_u8(0, video)
    sess.video_predict([0, 2, 4])
    before = sess.video_maps_u8(0, F20, size=SRC)
    lo, gate = int(np.percentile(before, 20)), int(np.percentile(before, 70)) + 1
    pf_law = dataflow.prefilter_law(gate=gate, full=lo)
    filtered, grid, maps, _ = sess.video_prefilter(0, F20, SRC[0], SRC[1], pf_law, block=8, radius=3, passes=2)
    assert np.array_equal(maps, before) and (filtered != video).any() and (grid == 0).any() and (grid > 0).any()
    wlaw = np.where(np.arange(256) >= gate, 0, 255).astype(np.int32)
    table, bs, maps, _ = sess.video_distortion(0, F20, filtered, wlaw, block=8, gate=gate)
    want_table, want_bs = dr.distortion(before, video, filtered, wlaw, block=8, gate=gate)
    assert np.array_equal(maps, before) and np.array_equal(table, want_table) and np.array_equal(bs, want_bs)
    # the replay's own account of the promise: Wn = 0 exactly where the four grid entries round a pixel are 0
    changed = (filtered != video).any(axis=3)
    salient = before >= gate
    clear = np.stack([pr.weight(g, SRC[0], SRC[1], 8) == 0 for g in grid])
    assert (clear & salient).any() and not (changed & clear).any()
    inside = (changed & salient & clear).reshape(F20, -1).sum(axis=1)
    assert (inside == 0).all()
    outside = (changed & salient & ~clear).reshape(F20, -1).sum(axis=1)
    assert np.array_equal(table[:, dr.CHANGED_SALIENT], outside) and np.array_equal(want_table[:, dr.CHANGED_SALIENT], inside + outside)
    # a salient pixel weighs 0 under this law, so the weighted error is the error where nobody looks
    assert (table[:, dr.WSSE:dr.WSSE + 4] <= 255 * table[:, dr.SSE:dr.SSE + 4]).all()
    sess.close_video()
    sess.close()


def test_refusals_change_nothing():
    from sap3d_tensorflow_amd import P3dError, dataflow
    sess = _session()
    law = dataflow.distortion_law()
    video = _video(F20, 5)
    test = dr.near(video, 6)
    with pytest.raises(P3dError, match="no video is open"):
        sess.video_distortion(0, 1, test[:1], law, ref=video[:1])
    sess.open_video(F20, "newest")
    sess.video_put_u8(0, video)
    sess.video_predict([0])
    maps = sess.video_maps_u8(0, 16, size=SRC)
    with pytest.raises(P3dError, match="keeps no source"):
        sess.video_distortion(0, 4, test[:4], law, size=SRC)
    assert np.array_equal(sess.video_maps_u8(0, 16, size=SRC), maps)
    assert np.array_equal(sess.video_distortion(0, 4, test[:4], law, ref=video[:4])[0], dr.distortion(maps[:4], video[:4], test[:4], law)[0])
    sess.close_video()
    sess.open_video(F20, "newest")                                    # frames 16 .. 19 stay unpredicted
    sess.video_keep_source(True)
    sess.video_put_u8(0, video)
    sess.video_predict([0])
    before = sess.video_maps_u8(0, 16, size=SRC)
    seen = sess.video_render(0, 16)
    want = dr.distortion(before[:9], video[:9], test[:9], law, block=16, gate=99)

    def valid():
        got = sess.video_distortion(0, 9, test[:9], law, block=16, gate=99)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(sess.video_maps_u8(0, 16, size=SRC), before) and np.array_equal(sess.video_render(0, 16), seen)

    valid()
    bad_law = law.copy()
    bad_law[3] = 256
    for kw, word in ((dict(block=24), "block"), (dict(gate=256), "gate"), (dict(block=0, block_map=True), "block map")):
        with pytest.raises(P3dError, match=word):
            sess.video_distortion(0, 4, test[:4], law, **kw)
    with pytest.raises(P3dError, match="wlaw\\[3\\]"):
        sess.video_distortion(0, 4, test[:4], bad_law)
    valid()
    with pytest.raises(P3dError, match="frame 16"):
        sess.video_distortion(10, 8, test[10:18], law)                # an unpredicted frame
    with pytest.raises(P3dError, match="outside"):
        sess.video_distortion(19, 2, test[:2], law)
    with pytest.raises(ValueError):
        sess.video_distortion(0, 4, None, law)
    valid()
    sess.close_video()
    sess.close()


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def _run(args, ok=True):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "drivers", "gen_pred.py")] + args
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert (done.returncode == 0) == ok, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    return done.stdout if ok else done.stderr


def test_driver_writes_the_three_files(tmp_path):
    from sap3d_tensorflow_amd import dataflow
    videos, decoded = tmp_path / "videos", tmp_path / "decoded"
    videos.mkdir()
    decoded.mkdir()
    n = 18
    rgb = _video(n, 0)
    test = dr.near(rgb, 4)
    test[3] = rgb[3]                                           # a frame that came through unchanged
    np.save(videos / "a.npy", rgb)
    np.save(decoded / "a.npy", test)
    text = _run(["--structure", "unet", "--videos", str(videos), "--batch", "3", "--base", "16", "--blocks", "1,1,1", "--resident",
                 "--write", "png", "--size", str(SRC[0]), str(SRC[1]), "--normalize", "range", "--out", str(tmp_path / "out"), "--distortion", str(decoded),
                 "--dist-gate", "100", "--dist-block", "8", "--dist-gamma", "0.5", "--dist-floor", "2", "--time"])
    assert "distortion launches" in text
    out = tmp_path / "out"
    table, bs = np.load(out / "a_distortion.npy"), np.load(out / "a_block_sse.npy")
    assert table.dtype == np.int64 and table.shape == (n, dr.RECORD) and bs.dtype == np.int64 and bs.shape == (n, 3, 5)
    # what does not depend on the maps is the replay's on the frames alone
    want, want_bs = dr.distortion(np.zeros((n,) + SRC, np.uint8), rgb[..., ::-1], test[..., ::-1], dr.identity_law(), block=8)
    for k in (dr.SSE, dr.MAXABS):
        assert np.array_equal(table[:, k:k + 4], want[:, k:k + 4])
    assert np.array_equal(table[:, [dr.CHANGED, dr.NW, dr.SQ]], want[:, [dr.CHANGED, dr.NW, dr.SQ]]) and np.array_equal(bs, want_bs)
    assert (table[3, :dr.SW] == 0).all() and table[3, dr.SQ] == 65536 * table[3, dr.NW]
    law = dataflow.distortion_law(100, 0.5, 2)
    assert (table[:, dr.SW] >= 2 * SRC[0] * SRC[1]).all() and (table[:, dr.SW] <= int(law.max()) * SRC[0] * SRC[1]).all()
    rep = dataflow.distortion_report(table, SRC[0] * SRC[1])
    lines = open(out / "a_distortion.csv").read().splitlines()
    assert lines[0] == "frame,psnr_b,psnr_g,psnr_r,psnr_y,wpsnr_b,wpsnr_g,wpsnr_r,wpsnr_y,ssim,wssim,changed_salient_share" and len(lines) == n + 1
    for k in (0, 3, n - 1):
        cells = lines[k + 1].split(",")
        assert int(cells[0]) == k + 1 and float(cells[4]) == rep["psnr"][k, 3] and float(cells[9]) == rep["ssim"][k]
    assert float(lines[4].split(",")[4]) == float("inf")
    assert "a distortion over %d frames: psnr_y" % n in text and "a_distortion.npy, a_distortion.csv, a_block_sse.npy" in text
    # an explicit reference: the same frames again give the same table
    text = _run(["--structure", "unet", "--videos", str(videos), "--batch", "3", "--base", "16", "--blocks", "1,1,1", "--resident",
                 "--write", "png", "--size", str(SRC[0]), str(SRC[1]), "--normalize", "range", "--out", str(tmp_path / "out2"), "--distortion", str(decoded),
                 "--dist-gate", "100", "--dist-gamma", "0.5", "--dist-floor", "2", "--dist-ref", str(videos)])
    assert np.array_equal(np.load(tmp_path / "out2" / "a_distortion.npy"), table) and not os.path.exists(tmp_path / "out2" / "a_block_sse.npy")


def test_the_flag_is_refused_without_resident(tmp_path):
    err = _run(["--structure", "unet", "--videos", str(tmp_path), "--out", str(tmp_path / "out"), "--distortion", str(tmp_path / "d")], ok=False)
    assert "--distortion needs --resident" in err
    err = _run(["--structure", "unet", "--videos", str(tmp_path), "--out", str(tmp_path / "out"), "--resident", "--dist-gate", "2"], ok=False)
    assert "need --distortion DIR" in err
    err = _run(["--structure", "unet", "--videos", str(tmp_path), "--out", str(tmp_path / "out"), "--resident", "--distortion", str(tmp_path / "d"),
                "--dist-block", "24"], ok=False)
    assert "--dist-block is 0, 8, 16, 32, 64 or 128" in err
    assert not os.path.exists(tmp_path / "out")
