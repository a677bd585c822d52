"""drivers/gen_pred.py --resident --render DIR end to end on a small synthetic video: the colour PNGs it writes, decoded, are
tests/render_ref.py's overlay of the 8-bit maps the same run writes on the video's own frames."""
import importlib.util
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import render_ref as R        # noqa: E402

F18, SRC = 18, (36, 52)


def _driver():
    spec = importlib.util.spec_from_file_location("gen_pred_render_gpu", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_driver_writes_the_replays_overlays(tmp_path, capsys):
    from sap3d_tensorflow_amd import dataflow
    gp = _driver()
    videos = tmp_path / "videos"
    videos.mkdir()
    rng = np.random.default_rng(0)
    rgb = np.clip(rng.integers(0, 120, (F18,) + SRC + (3,)) + R.blob(F18, *SRC, seed=3)[..., None] // 2, 0, 255).astype(np.uint8)
    np.save(videos / "a.npy", rgb)
    common = ["--structure", "unet", "--videos", str(videos), "--batch", "3", "--base", "16", "--blocks", "1,1,1", "--resident",
              "--write", "png", "--size", str(SRC[0]), str(SRC[1]), "--normalize", "range"]
    flags = ["--render-colormap", "hot", "--render-alpha", "0.8", "--render-opacity", "constant", "--render-gate", "30",
             "--render-contour", "128", "--render-thickness", "2", "--render-contour-color", "0,255,64"]
    gp.main(common + ["--out", str(tmp_path / "out"), "--render", str(tmp_path / "seen"), "--time"] + flags)
    text = capsys.readouterr().out
    assert "a 18 rendered png files in" in text and "render launches" in text
    gp.main(common + ["--out", str(tmp_path / "plain")])
    table = dataflow.render_table("hot", 0.8, "constant", gate=30)
    maps = np.stack([_png(tmp_path / "out" / "a" / ("frame_%d.png" % k)) for k in range(1, F18 + 1)])
    assert maps.dtype == np.uint8 and maps.shape == (F18,) + SRC and maps.max() == 255
    want = R.render(maps, rgb[..., ::-1], table, 128, 2, (64, 255, 0))[..., ::-1]
    for k in range(1, F18 + 1):
        got = _png(tmp_path / "seen" / "a" / ("frame_%d.png" % k))
        assert got.shape == SRC + (3,) and np.array_equal(got, want[k - 1]), k
        # the map write-out is what it is without --render
        a, b = (tmp_path / d / "a" / ("frame_%d.png" % k) for d in ("out", "plain"))
        assert a.read_bytes() == b.read_bytes(), k
    assert R.contour_mask(maps, 128, 2).any()
    assert len(os.listdir(tmp_path / "seen" / "a")) == F18

