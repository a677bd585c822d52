"""p3d_video_qpmap on a resident video (P3DSession.video_qpmap): offsets, levels and statistics are tests/qpmap_ref.py's on
video_maps_u8's bytes, exactly -- over a part of the video, under a shot table, under temporal smoothing -- and the maps read the same
before and after; and drivers/gen_pred.py --resident --qpmap DIR end to end on two small synthetic videos, in a child process:
qp.npy, stats.npy and levels.npy are the replay's tables of the 8-bit maps the same run writes (the bytes the session call reads),
and qp.txt parses back to qp.npy."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import qpmap_ref as qr         # noqa: E402
import reframe_ref as F        # noqa: E402

SRC = (24, 40)
F20, T = 20, 16
LENGTHS = dict(a=18, b=16)


def _video(n, seed):
    rng = np.random.default_rng(seed)
    return np.clip(rng.integers(0, 120, (n,) + SRC + (3,)) + F.blobs(n, *SRC, seed=3 + seed)[..., None] // 2, 0, 255).astype(np.uint8)


def _same(res, want):
    assert res["qp"].dtype == np.int32 and np.array_equal(res["qp"], want[0]), (res["qp"][:2].tolist(), want[0][:2].tolist())
    if "levels" in res:
        assert res["levels"].dtype == np.uint8 and np.array_equal(res["levels"], want[1])
    if "stats" in res:
        assert res["stats"].dtype == np.int32 and np.array_equal(res["stats"], want[2])


@pytest.mark.parametrize("temporal", [False, True])
def test_qpmap_is_the_replay_on_the_bytes_of_video_maps_u8(temporal):
    from sap3d_tensorflow_amd import P3DSession, dataflow
    sess = P3DSession("unet", seed=2, batch=3, frames=T, height=32, width=32, base=16, blocks=(1, 1, 1))
    sess.set_postprocess(0., 0, "range")
    sess.open_video(F20, "mean")
    sess.video_put_u8(0, _video(F20, 0))
    sess.video_predict([0, 2, 4])
    if temporal:
        sess.set_video_temporal("gauss", sigma=1.0)
    law = dataflow.qp_law(-30, 10, gate=20, gamma=0.8)
    before = sess.video_maps_u8(0, F20, size=SRC)
    assert before.max() > before.min()
    # the whole video, no shot table
    res = sess.video_qpmap(0, F20, SRC, law, block=8, dilate=1, fall=1, rise=2, lo=-30, hi=10, with_levels=True, with_stats=True,
                           with_maps=True, timed=True)
    assert np.array_equal(res["maps"], before)
    want = qr.qpmap(before, law, 8, 128, 1, 1, 2, 1, 0, -30, 10)
    assert want[0].shape == (F20, 3, 5) and want[0].max() > want[0].min()
    _same(res, want)
    assert set(sess.last_qpmap_ms) == {"device", "qpmap"} and sess.last_qpmap_ms["qpmap"] > 0.0 and sess.last_qpmap_ms["device"] > 0.0
    assert np.array_equal(sess.video_maps_u8(0, F20, size=SRC), before)          # off until called, and nothing left behind
    # a part that does not start at 0 is a world of its own for the limiter
    part = sess.video_qpmap(5, 9, SRC, law, block=16, fall=1, rise=2, balance=False, lo=-30, hi=10, with_stats=True)
    assert set(part) == {"qp", "stats"}
    _same(part, qr.qpmap(before[5:14], law, 16, 128, 0, 1, 2, 0, 0, -30, 10))
    # under a shot table, cut to the range as video_reframe cuts it: starts 8 and 13 of the video are 3 and 8 of the call
    sess.video_set_shots([0, 4, 8, 13, 15])
    under = sess.video_maps_u8(0, F20, size=SRC)                                 # (the temporal filter follows the table too)
    assert temporal or np.array_equal(under, before)
    full = sess.video_qpmap(0, F20, SRC, law, block=8, dilate=1, fall=1, rise=2, lo=-30, hi=10, with_levels=True, with_stats=True)
    _same(full, qr.qpmap(under, law, 8, 128, 1, 1, 2, 1, 0, -30, 10, shots=[0, 4, 8, 13, 15]))
    part = sess.video_qpmap(5, 9, SRC, law, block=8, fall=1, rise=2, lo=-30, hi=10, with_maps=True)
    assert np.array_equal(part["maps"], under[5:14])
    _same(part, qr.qpmap(under[5:14], law, 8, 128, 0, 1, 2, 1, 0, -30, 10, shots=[0, 3, 8]))
    # another size
    size = (45, 23)
    maps2 = sess.video_maps_u8(2, 6, size=size)
    res2 = sess.video_qpmap(2, 6, size, law, block=32, peak_weight=256, with_maps=True, with_levels=True)
    assert np.array_equal(res2["maps"], maps2) and res2["qp"].shape == (6, 2, 1)
    _same(res2, qr.qpmap(maps2, law, 32, 256, shots=[0, 2]))
    assert np.array_equal(sess.video_maps_u8(0, F20, size=SRC), under)
    sess.close_video()
    sess.close()


def test_refusals_change_nothing():
    from sap3d_tensorflow_amd import P3DSession, P3dError, dataflow
    sess = P3DSession("unet", seed=2, batch=3, frames=T, height=32, width=32, base=16, blocks=(1, 1, 1))
    law = dataflow.qp_law(-12, 6)
    with pytest.raises(P3dError, match="no video is open"):
        sess.video_qpmap(0, 1, SRC, law)
    sess.open_video(F20, "newest")                                    # frames 16 .. 19 stay unpredicted
    sess.video_put_u8(0, _video(F20, 5))
    sess.video_predict([0])
    before = sess.video_maps_u8(0, 16, size=SRC)
    want = qr.qpmap(before[:9], law, 8, 128, 0, 2, 2)

    def valid():
        _same(sess.video_qpmap(0, 9, SRC, law, block=8, fall=2, rise=2, with_levels=True, with_stats=True), want)
        assert np.array_equal(sess.video_maps_u8(0, 16, size=SRC), before)

    valid()
    bad_law = law.copy()
    bad_law[3] = 128
    for bad, word in ((dict(block=12), "block"), (dict(lo=3, hi=2, target=2), "lo"), (dict(target=100, hi=50), "target"),
                      (dict(peak_weight=-1), "peak_weight"), (dict(dilate=9), "dilate"), (dict(fall=255), "fall")):
        with pytest.raises(P3dError, match=word):
            sess.video_qpmap(0, 4, SRC, law, **bad)
        valid()
    with pytest.raises(P3dError, match="law\\[3\\]"):
        sess.video_qpmap(0, 4, SRC, bad_law)
    with pytest.raises(P3dError, match="2\\^23"):
        sess.video_qpmap(0, 1, (2 ** 12, 2 ** 11 + 1), law)
    valid()
    with pytest.raises(P3dError, match="frame 16"):
        sess.video_qpmap(10, 8, SRC, law)                             # an unpredicted frame
    with pytest.raises(P3dError, match="outside"):
        sess.video_qpmap(19, 2, SRC, law)
    valid()
    sess.close_video()
    sess.close()


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _run(args, ok=True):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "drivers", "gen_pred.py")] + args
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert (done.returncode == 0) == ok, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    return done.stdout if ok else done.stderr


def test_driver_writes_the_replays_tables(tmp_path):
    from sap3d_tensorflow_amd import dataflow
    videos = tmp_path / "videos"
    videos.mkdir()
    for k, (name, n) in enumerate(sorted(LENGTHS.items())):
        np.save(videos / (name + ".npy"), _video(n, k))
    shots = tmp_path / "shots.npy"
    np.save(shots, np.array([0, 6, 11], np.int32))
    text = _run(["--structure", "unet", "--videos", str(videos), "--batch", "3", "--base", "16", "--blocks", "1,1,1", "--resident",
                 "--write", "png", "--size", str(SRC[0]), str(SRC[1]), "--normalize", "range", "--out", str(tmp_path / "out"),
                 "--qpmap", str(tmp_path / "qp"), "--qp-block", "8", "--qp-peak-weight", "200", "--qp-dilate", "1", "--qp-fall", "1",
                 "--qp-rise", "2", "--qp-min", "-20", "--qp-max", "8", "--qp-gate", "30", "--qp-gamma", "0.7", "--qp-levels",
                 "--shots", str(shots), "--time"])
    assert "qpmap launches" in text
    law = dataflow.qp_law(-20, 8, 30, 0.7)
    for name, n in LENGTHS.items():
        maps = np.stack([_png(tmp_path / "out" / name / ("frame_%d.png" % k)) for k in range(1, n + 1)])
        assert maps.dtype == np.uint8 and maps.shape == (n,) + SRC and maps.max() == 255
        want = qr.qpmap(maps, law, 8, 200, 1, 1, 2, 1, 0, -20, 8, shots=[0, 6, 11])
        assert sorted(os.listdir(tmp_path / "qp" / name)) == ["levels.npy", "qp.npy", "qp.txt", "stats.npy"]
        qp, st, lev = (np.load(tmp_path / "qp" / name / (k + ".npy")) for k in ("qp", "stats", "levels"))
        assert qp.dtype == np.int32 and qp.shape == (n, 3, 5) and st.dtype == np.int32 and st.shape == (n, 4) and lev.dtype == np.uint8
        assert qp.max() > qp.min()
        assert np.array_equal(qp, want[0]) and np.array_equal(lev, want[1]) and np.array_equal(st, want[2])
        rows = [[int(v) for v in line.split(" ")] for line in open(tmp_path / "qp" / name / "qp.txt").read().splitlines()]
        assert [r[0] for r in rows] == list(range(1, n + 1)) and all(len(r) == 1 + 15 for r in rows)
        assert np.array_equal(np.array([r[1:] for r in rows], np.int32).reshape(n, 3, 5), qp)
        assert "%s 3 x 5 offsets in [%d, %d] over %d frames" % (name, qp.min(), qp.max(), n) in text


def test_the_flag_is_refused_without_resident(tmp_path):
    err = _run(["--structure", "unet", "--videos", str(tmp_path), "--out", str(tmp_path / "out"), "--qpmap", str(tmp_path / "qp")], ok=False)
    assert "--qpmap needs --resident" in err
    err = _run(["--structure", "unet", "--videos", str(tmp_path), "--out", str(tmp_path / "out"), "--resident", "--qp-fall", "2"], ok=False)
    assert "need --qpmap DIR" in err
    err = _run(["--structure", "unet", "--videos", str(tmp_path), "--out", str(tmp_path / "out"), "--resident", "--qpmap", str(tmp_path / "qp"),
                "--qp-block", "12"], ok=False)
    assert "--qp-block is 8, 16, 32, 64 or 128" in err
