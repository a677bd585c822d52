"""drivers/gen_pred.py --resident --regions DIR end to end on two small synthetic videos, in a child process: regions.npy, counts.npy
and labels.npy have the documented shapes and dtypes and are tests/regions_ref.py's tables of the 8-bit maps the same run writes
(the bytes P3DSession.video_regions labels), inside the shots of --shots; without --resident the flag is refused."""
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
import regions_ref as rr       # noqa: E402

SRC = (24, 40)
LENGTHS = dict(a=18, b=16)


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _run(args, ok=True):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "drivers", "gen_pred.py")] + args
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert (done.returncode == 0) == ok, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    return done.stdout if ok else done.stderr


def test_driver_writes_the_replays_tables(tmp_path):
    videos = tmp_path / "videos"
    videos.mkdir()
    for k, (name, n) in enumerate(sorted(LENGTHS.items())):
        rng = np.random.default_rng(k)
        rgb = np.clip(rng.integers(0, 120, (n,) + SRC + (3,)) + F.blobs(n, *SRC, seed=3 + k)[..., None] // 2, 0, 255).astype(np.uint8)
        np.save(videos / (name + ".npy"), rgb)
    shots = tmp_path / "shots.npy"
    np.save(shots, np.array([0, 6, 11], np.int32))
    text = _run(["--structure", "unet", "--videos", str(videos), "--batch", "3", "--base", "16", "--blocks", "1,1,1", "--resident",
                 "--write", "png", "--size", str(SRC[0]), str(SRC[1]), "--normalize", "range", "--out", str(tmp_path / "out"),
                 "--regions", str(tmp_path / "reg"), "--regions-gate", "150", "--regions-connectivity", "4", "--regions-min-area", "2",
                 "--regions-max", "5", "--regions-link", "--regions-labels", "--shots", str(shots), "--time"])
    assert "regions launches" in text
    for name, n in LENGTHS.items():
        maps = np.stack([_png(tmp_path / "out" / name / ("frame_%d.png" % k)) for k in range(1, n + 1)])
        assert maps.dtype == np.uint8 and maps.shape == (n,) + SRC and maps.max() == 255
        want = rr.regions(maps, 150, 4, 2, 5, True, shots=[0, 6, 11])
        assert sorted(os.listdir(tmp_path / "reg" / name)) == ["counts.npy", "labels.npy", "regions.npy"]
        rec, counts, lab = (np.load(tmp_path / "reg" / name / (k + ".npy")) for k in ("regions", "counts", "labels"))
        assert rec.dtype == np.int32 and rec.shape == (n, 5, rr.FIELDS) and counts.dtype == np.int32 and counts.shape == (n, 3)
        assert lab.dtype == np.uint8 and lab.shape == (n,) + SRC
        assert counts[:, 2].max() >= 1
        assert np.array_equal(counts, want[1]) and np.array_equal(rec, want[0]) and np.array_equal(lab, want[2])
        assert "%s %d regions over %d frames" % (name, counts[:, 2].sum(), n) in text
        print(name, "kept", counts[:, 2].tolist())


def test_the_flag_is_refused_without_resident(tmp_path):
    err = _run(["--structure", "unet", "--videos", str(tmp_path), "--out", str(tmp_path / "out"), "--regions", str(tmp_path / "reg")], ok=False)
    assert "--regions needs --resident" in err
    err = _run(["--structure", "unet", "--videos", str(tmp_path), "--out", str(tmp_path / "out"), "--resident", "--regions-link"], ok=False)
    assert "need --regions DIR" in err
