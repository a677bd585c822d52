"""drivers/gen_pred.py --resident --shots detect --temporal gauss --reframe DIR end to end on a small two-shot video, in a child
process: the shot table and the cut signal it writes are tests/shots_ref.py's, and the reframe track on either side of the cut is
the track of that side alone -- nothing of the other shot enters it, so the window may jump at the cut."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import reframe_ref as F        # noqa: E402
import shots_ref as S          # noqa: E402

SRC, N, CUT = (24, 40), 18, 8


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _run(args, ok=True):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "drivers", "gen_pred.py")] + args
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert (done.returncode == 0) == ok, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    return done.stdout + done.stderr


def test_driver_detects_the_cut_and_reframes_inside_the_shots(tmp_path):
    videos = tmp_path / "videos"
    videos.mkdir()
    rgb = S.fixture((CUT, N - CUT), *SRC)
    np.save(videos / "v.npy", rgb)
    common = ["--structure", "unet", "--videos", str(videos), "--batch", "3", "--base", "16", "--blocks", "1,1,1", "--resident",
              "--write", "png", "--size", str(SRC[0]), str(SRC[1]), "--normalize", "range", "--temporal", "gauss", "--temporal-sigma", "1.5",
              "--reframe-aspect", "9:16", "--reframe-smooth", "3"]
    text = _run(common + ["--out", str(tmp_path / "out"), "--reframe", str(tmp_path / "cut"), "--shots", "detect", "--shots-grid", "2", "3"])
    assert "v 2 shots, starting at frames 0 %d" % CUT in text
    starts = np.load(tmp_path / "out" / "v_shots.npy")
    assert starts.dtype == np.int32 and starts.tolist() == [0, CUT]
    assert np.array_equal(np.load(tmp_path / "out" / "v_cutsignal.npy"), S.distances(rgb, 2, 3))
    hc, wc = F.aspect_window(*SRC, 9, 16)
    maps = np.stack([_png(tmp_path / "out" / "v" / ("frame_%d.png" % k)) for k in range(1, N + 1)])
    rows = np.load(tmp_path / "cut" / "v" / "track.npy")
    track, raw, mass, crop = S.reframe_shots(maps, rgb, hc, wc, 0, 3, [0, CUT])
    assert np.array_equal(rows[:, 0:2], track) and np.array_equal(rows[:, 2:4], raw) and np.array_equal(rows[:, 4:7], mass)
    assert np.array_equal(track[:CUT], F.reframe(maps[:CUT], None, hc, wc, 0, 3)[0])
    assert np.array_equal(track[CUT:], F.reframe(maps[CUT:], None, hc, wc, 0, 3)[0])
    for k in (1, CUT, CUT + 1, N):
        assert np.array_equal(_png(tmp_path / "cut" / "v" / ("frame_%d.png" % k)), crop[k - 1]), k
    print("track either side of the cut", track[CUT - 1].tolist(), track[CUT].tolist())
    # the same table from a file: the same maps and the same track; no cut signal is written
    text = _run(common + ["--out", str(tmp_path / "out2"), "--reframe", str(tmp_path / "cut2"), "--shots", str(tmp_path / "out" / "v_shots.npy")])
    assert np.array_equal(np.load(tmp_path / "cut2" / "v" / "track.npy"), rows)
    assert np.array_equal(_png(tmp_path / "out2" / "v" / ("frame_%d.png" % CUT)), maps[CUT - 1])
    assert not os.path.exists(tmp_path / "out2" / "v_cutsignal.npy") and np.array_equal(np.load(tmp_path / "out2" / "v_shots.npy"), starts)
    # without a table the maps round the cut are other maps: the filter ran across it
    _run(common + ["--out", str(tmp_path / "out3"), "--reframe", str(tmp_path / "cut3")])
    other = np.stack([_png(tmp_path / "out3" / "v" / ("frame_%d.png" % k)) for k in range(1, N + 1)])
    assert not np.array_equal(other[CUT - 1:CUT + 1], maps[CUT - 1:CUT + 1])


@pytest.mark.parametrize("extra,word", [
    (["--shots", "detect"], "needs --resident"),
    (["--resident", "--shots-grid", "2", "2"], "need --shots detect"),
    (["--resident", "--shots", "detect", "--shots-grid", "5", "1"], "--shots-grid"),
    (["--resident", "--shots", "detect", "--shots-threshold", "0"], "--shots-threshold"),
    (["--resident", "--shots", "detect", "--shots-window", "33"], "--shots-window"),
    (["--resident", "--shots", "detect", "--shots-ratio", "255"], "--shots-ratio"),
    (["--resident", "--shots", "detect", "--shots-min-length", "0"], "--shots-min-length"),
])
def test_driver_checks_its_values_before_anything_runs(extra, word, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    with pytest.raises(SystemExit):
        gp.parse_args(["--structure", "unet", "--videos", "nowhere", "--out", "nowhere"] + extra)
    assert word in capsys.readouterr().err
