"""drivers/gen_pred.py --resident --reframe DIR end to end on two small synthetic videos, in a child process: the colour PNGs it
writes, decoded, are tests/reframe_ref.py's windows of the video's own frames on the track of the 8-bit maps the same run writes,
track.npy is the replay's track, raw track and masses, and --render beside it writes what it writes alone."""
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
import render_ref as R         # noqa: E402

SRC = (24, 40)
LENGTHS = dict(a=18, b=16)


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _run(args):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "drivers", "gen_pred.py")] + args
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    return done.stdout


def test_driver_writes_the_replays_windows_and_tracks(tmp_path):
    from sap3d_tensorflow_amd import dataflow
    videos = tmp_path / "videos"
    videos.mkdir()
    rgb = {}
    for k, (name, n) in enumerate(sorted(LENGTHS.items())):
        rng = np.random.default_rng(k)
        rgb[name] = np.clip(rng.integers(0, 120, (n,) + SRC + (3,)) + F.blobs(n, *SRC, seed=3 + k)[..., None] // 2, 0, 255).astype(np.uint8)
        np.save(videos / (name + ".npy"), rgb[name])
    common = ["--structure", "unet", "--videos", str(videos), "--batch", "3", "--base", "16", "--blocks", "1,1,1", "--resident",
              "--write", "png", "--size", str(SRC[0]), str(SRC[1]), "--normalize", "range"]
    text = _run(common + ["--out", str(tmp_path / "out"), "--reframe", str(tmp_path / "cut"), "--reframe-aspect", "9:16", "--reframe-gate", "20",
                          "--reframe-smooth", "2", "--render", str(tmp_path / "seen"), "--time"])
    assert "reframe launches" in text and "render launches" in text
    hc, wc = F.aspect_window(*SRC, 9, 16)
    assert (hc, wc) == (24, 12)
    table = dataflow.render_table("jet", 0.6, "ramp")
    for name, n in LENGTHS.items():
        assert "%s %d reframed %d x %d png files and track.npy in" % (name, n, hc, wc) in text
        maps = np.stack([_png(tmp_path / "out" / name / ("frame_%d.png" % k)) for k in range(1, n + 1)])
        assert maps.dtype == np.uint8 and maps.shape == (n,) + SRC and maps.max() == 255
        track, raw, mass, crop = F.reframe(maps, rgb[name], hc, wc, 20, 2)
        rows = np.load(tmp_path / "cut" / name / "track.npy")
        assert rows.dtype == np.int64 and rows.shape == (n, 7)
        assert np.array_equal(rows[:, 0:2], track) and np.array_equal(rows[:, 2:4], raw) and np.array_equal(rows[:, 4:7], mass)
        assert sorted(os.listdir(tmp_path / "cut" / name)) == sorted(["frame_%d.png" % k for k in range(1, n + 1)] + ["track.npy"])
        for k in range(1, n + 1):
            got = _png(tmp_path / "cut" / name / ("frame_%d.png" % k))
            assert got.shape == (hc, wc, 3) and np.array_equal(got, crop[k - 1]), (name, k)
        # --render beside it: the overlays of the same maps on the whole frames
        assert len(os.listdir(tmp_path / "seen" / name)) == n
        want = R.render(maps, rgb[name][..., ::-1], table)[..., ::-1]
        for k in (1, n):
            assert np.array_equal(_png(tmp_path / "seen" / name / ("frame_%d.png" % k)), want[k - 1]), (name, k)
        print(name, "track", rows[::5, :2].tolist())


def test_driver_reframes_to_a_given_size_alone(tmp_path):
    """--reframe-size, no --render, the raw track (no smoothing, no gate)."""
    videos = tmp_path / "videos"
    videos.mkdir()
    rng = np.random.default_rng(7)
    n = 16
    rgb = np.clip(rng.integers(0, 120, (n,) + SRC + (3,)) + F.blobs(n, *SRC, seed=9)[..., None] // 2, 0, 255).astype(np.uint8)
    np.save(videos / "c.npy", rgb)
    text = _run(["--structure", "unet", "--videos", str(videos), "--batch", "3", "--base", "16", "--blocks", "1,1,1", "--resident",
                 "--write", "png", "--size", str(SRC[0]), str(SRC[1]), "--out", str(tmp_path / "out"), "--reframe", str(tmp_path / "cut"),
                 "--reframe-size", "9", "21"])
    assert "c 16 reframed 9 x 21 png files" in text and "rendered" not in text
    maps = np.stack([_png(tmp_path / "out" / "c" / ("frame_%d.png" % k)) for k in range(1, n + 1)])
    track, raw, mass, crop = F.reframe(maps, rgb, 9, 21, 0, 0)
    rows = np.load(tmp_path / "cut" / "c" / "track.npy")
    assert np.array_equal(rows[:, 0:2], raw) and np.array_equal(rows[:, 2:4], raw) and np.array_equal(rows[:, 4:7], mass)
    for k in range(1, n + 1):
        assert np.array_equal(_png(tmp_path / "cut" / "c" / ("frame_%d.png" % k)), crop[k - 1]), k
