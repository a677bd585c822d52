"""p3d_video_score on a resident video (P3DSession.video_score): the scored bytes are video_maps_u8's, the scores are
metrics.score_bytes' on those bytes, bit for bit; the read-out before and after is unchanged; refusals change nothing; and
drivers/gen_pred.py --truth writes what it promises."""
import importlib.util
import os
import re
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import score_u8_ref as R        # noqa: E402

CFG = dict(base=16, blocks=(2, 2, 3))
F20, T, SIZE = 20, 16, (48, 40)


def _session():
    from sap3d_tensorflow_amd import P3DSession
    return P3DSession("unet", seed=2, batch=3, frames=T, height=32, width=32, **CFG)


def _frames(F, seed=0):
    return np.random.default_rng(seed).normal(0.0, 0.5, (F, 32, 32, 3)).astype(np.float32)


def _truth(F, seed=3):
    rng = np.random.default_rng(seed)
    den = R.blobs(rng, F, *SIZE)
    fix = np.stack([R.fixations(rng, d, 40) for d in den])
    return den, fix


def _resident(sess, frames, mode, starts):
    sess.open_video(len(frames), mode)
    sess.video_put(0, frames)
    for i in range(0, len(starts), 3):
        sess.video_predict(starts[i:i + 3])


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("setting", ["plain newest", "mean, temporal, blur, range"])
def test_scores_are_score_bytes_on_the_bytes_of_video_maps_u8(setting):
    from sap3d_tensorflow_amd import metrics
    sess = _session()
    plain = setting == "plain newest"
    if not plain:
        sess.set_postprocess(1.5, 0, "range")
        sess.set_video_temporal("gauss", 1.0, 0, 0.0)
    _resident(sess, _frames(F20, seed=4), "newest" if plain else "mean", [0, 1, 2, 3, 4])
    den, fix = _truth(F20)
    before = sess.video_maps_u8(0, F20, size=SIZE)
    for columns, ties in ((("cc", "sim", "judd"), "expected"), (("cc", "sim", "judd", "kl", "nss"), "reference")):
        got, maps = sess.video_score(0, F20, den, fix, size=SIZE, columns=columns, ties=ties, with_maps=True)
        assert maps.dtype == np.uint8 and np.array_equal(maps, before)
        want = metrics.score_bytes(maps, den, fix, flags=columns, ties=ties)
        assert got.shape == (F20, 5) and np.array_equal(_bits(got), _bits(want)), setting
        assert np.isfinite(got[:, :3]).all() and np.isnan(got[:, 3]).all() == ("kl" not in columns)
        assert set(sess.last_score_ms) == {"upload", "device", "score"} and sess.last_score_ms["score"] > 0.0
    # a part of the video, no maps back, and the replay's view of the same bytes
    part = sess.video_score(17, 3, den[17:], fix[17:], size=SIZE, columns="matlab")
    assert np.array_equal(_bits(part), _bits(metrics.score_bytes(before[17:], den[17:], fix[17:], flags="matlab")))
    ref = R.score_maps(before[17:], den[17:], fix[17:], R.MATLAB, R.EXPECTED)
    assert np.allclose(part[:, :3], ref[:, :3], rtol=R.GPU_GATE, atol=0.0)
    # the read-out is what it was
    assert np.array_equal(sess.video_maps_u8(0, F20, size=SIZE), before)
    sess.close_video()
    sess.close()


def test_refusals_change_nothing_and_launch_nothing():
    from sap3d_tensorflow_amd import P3dError
    sess = _session()
    den, fix = _truth(F20)
    with pytest.raises(P3dError, match="no video is open"):
        sess.video_score(0, 1, den[:1], fix[:1], size=SIZE)
    frames = _frames(F20, seed=6)
    sess.open_video(F20, "mean")
    sess.video_put(0, frames)
    sess.video_predict([0, 2])                        # frames 18 and 19 have no prediction
    before = sess.video_maps_u8(0, 18, size=SIZE)
    info = sess.video_info()
    with pytest.raises(P3dError, match="frame 18"):
        sess.video_score(10, 10, den[10:], fix[10:], size=SIZE)
    with pytest.raises(P3dError, match="flags"):
        sess.video_score(0, 4, den[:4], fix[:4], size=SIZE, columns=0)
    with pytest.raises(P3dError, match="flags"):
        sess.video_score(0, 4, den[:4], fix[:4], size=SIZE, columns=32)
    with pytest.raises(P3dError, match="fixation"):
        sess.video_score(0, 4, den[:4], None, size=SIZE, columns=("cc", "nss"))
    with pytest.raises(P3dError, match="outside"):
        sess.video_score(18, 4, den[:4], fix[:4], size=SIZE)
    big = np.zeros((1, 2 ** 12, 2 ** 11 + 1), np.uint8)
    with pytest.raises(P3dError, match="2\\^23"):
        sess.video_score(0, 1, big, big, size=big.shape[1:])
    with pytest.raises(ValueError):
        sess.video_score(0, 4, den[:4], fix[:4], size=SIZE, ties="random")
    with pytest.raises(ValueError):
        sess.video_score(0, 4, den[:3], fix[:4], size=SIZE)
    assert sess.video_info() == info and np.array_equal(sess.video_maps_u8(0, 18, size=SIZE), before)
    ok = sess.video_score(0, 4, den[:4], None, size=SIZE, columns=("cc", "sim", "kl"))       # no fixation maps needed
    assert np.isfinite(ok[:, [0, 1, 3]]).all() and np.isnan(ok[:, [2, 4]]).all()
    sess.close_video()
    sess.close()


def test_driver_truth_writes_scores_and_prints_their_means(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    videos, truth = tmp_path / "videos", tmp_path / "truth"
    videos.mkdir()
    truth.mkdir()
    rng = np.random.default_rng(0)
    frames = {"a": 20, "b": 17}
    for name, F in frames.items():
        np.save(videos / (name + ".npy"), rng.integers(0, 256, (F, 60, 80, 3)).astype(np.uint8))
        den, fix = _truth(F, seed=F)
        if name == "b":
            fix[3] = 0                                 # a frame without fixation: NaN in AUC_Judd, dropped from the mean
        np.save(truth / (name + "_density.npy"), den)
        np.save(truth / (name + "_fixation.npy"), fix)
    out = tmp_path / "out"
    gp.main(["--structure", "unet", "--videos", str(videos), "--batch", "3", "--base", "16", "--blocks", "1,1,1", "--out", str(out),
             "--resident", "--truth", str(truth), "--size", str(SIZE[0]), str(SIZE[1]), "--score-columns", "cc", "sim", "judd", "nss"])
    text = capsys.readouterr().out
    means = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for name, F in frames.items():
            scores = np.load(out / (name + "_scores.npy"))
            assert scores.shape == (F, 5) and scores.dtype == np.float64
            assert np.isnan(scores[:, 3]).all() and np.isfinite(scores[:, [0, 1]]).all()
            assert np.isnan(scores[3, 2]) == (name == "b")
            assert not os.path.isdir(out / name)       # --write npy: no image left the device
            m = re.search(r"^%s scores over %d frames: (.*)$" % (name, F), text, re.M)
            printed = [float(v.split("=")[1]) for v in m.group(1).split(", ")]
            want = np.nanmean(scores, axis=0)
            assert np.array_equal(np.array(printed), want, equal_nan=True), (name, printed, want)
            means.append(want)
        m = re.search(r"^mean over 2 videos: (.*)$", text, re.M)
        printed = [float(v.split("=")[1]) for v in m.group(1).split(", ")]
        assert np.array_equal(np.array(printed), np.nanmean(np.stack(means), axis=0), equal_nan=True)
    # --write png with --truth: the images are the scored bytes, encoded as the run without --truth encodes them
    common = ["--structure", "unet", "--videos", str(videos), "--batch", "3", "--base", "16", "--blocks", "1,1,1", "--resident", "--write", "png",
              "--size", str(SIZE[0]), str(SIZE[1])]
    gp.main(common + ["--out", str(tmp_path / "png_scored"), "--truth", str(truth), "--score-columns", "cc", "sim", "judd", "nss"])
    gp.main(common + ["--out", str(tmp_path / "png_plain")])
    for name, F in frames.items():
        assert np.array_equal(np.load(tmp_path / "png_scored" / (name + "_scores.npy")), np.load(out / (name + "_scores.npy")), equal_nan=True)
        for k in range(1, F + 1):
            a, b = (tmp_path / d / name / ("frame_%d.png" % k) for d in ("png_scored", "png_plain"))
            assert a.read_bytes() == b.read_bytes(), (name, k)

