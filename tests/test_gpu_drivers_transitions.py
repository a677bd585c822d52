"""drivers/gen_pred.py --resident --shots detect on tests/transitions_ref.py's planted video, in a child process: without
--shots-gradual the driver writes the files it wrote before the gradual detector existed -- the cut table and the cut signal of
tests/shots_ref.py, and nothing else; with it, the replay's table, kinds and signals."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import shots_ref as S          # noqa: E402
import transitions_ref as T    # noqa: E402

SRC = (24, 40)


def _run(args):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "drivers", "gen_pred.py")] + args
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    return done.stdout + done.stderr


def test_driver_writes_the_cut_table_as_before_and_the_gradual_table_when_asked(tmp_path):
    videos = tmp_path / "videos"
    videos.mkdir()
    rgb = T.fixture(*SRC)
    np.save(videos / "v.npy", rgb)
    rule = T.FIXTURE_RULE
    common = ["--structure", "unet", "--videos", str(videos), "--batch", "4", "--base", "16", "--blocks", "1,1,1", "--resident", "--stride", "16",
              "--shots", "detect", "--shots-grid", "4", "4", "--shots-threshold", str(rule["threshold"]), "--shots-window", str(rule["window"]),
              "--shots-ratio", str(rule["ratio"]), "--shots-min-length", str(rule["min_length"])]
    D, E, v = T.signals(rgb, *T.FIXTURE_GRID, 12)
    # without the flag: the parent's files, byte for byte -- np.save of the replay's arrays
    text = _run(common + ["--out", str(tmp_path / "cuts")])
    assert "v 3 shots, starting at frames 0 48 188" in text
    want = tmp_path / "want"
    want.mkdir()
    np.save(want / "v_shots.npy", np.asarray(S.cuts(D, SRC[0] * SRC[1], **rule), np.int32))
    np.save(want / "v_cutsignal.npy", S.distances(rgb, *T.FIXTURE_GRID))
    for name in ("v_shots.npy", "v_cutsignal.npy"):
        assert (tmp_path / "cuts" / name).read_bytes() == (want / name).read_bytes(), name
    assert sorted(n for n in os.listdir(tmp_path / "cuts") if n.startswith("v_")) == ["v_cutsignal.npy", "v_shots.npy"]
    # with it: the replay's table, kinds and signals
    text = _run(common + ["--out", str(tmp_path / "gradual"), "--shots-gradual"])
    assert "v 6 shots, starting at frames 0 24 48 77 126 188" in text
    got = dict((n, np.load(tmp_path / "gradual" / ("v_%s.npy" % n))) for n in ("shots", "shotkinds", "cutsignal", "lagsignal", "spread"))
    assert got["shots"].dtype == np.int32 and got["shots"].tolist() == T.FIXTURE_STARTS
    assert got["shotkinds"].dtype == np.int32 and got["shotkinds"].tolist() == T.FIXTURE_KINDS
    assert np.array_equal(got["cutsignal"], D) and np.array_equal(got["lagsignal"], E) and np.array_equal(got["spread"], v)
    assert got["spread"].dtype == np.int64
