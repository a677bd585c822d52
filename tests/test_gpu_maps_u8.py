"""gen_pred.py's 8-bit write-out on the GPU (csrc/metrics_full.hip's resize_u8_kernel through the C ABI): the op bit-exact to the
float64 restatement (tests/maps_u8_ref.py), P3DSession.pred_maps_u8 on the network's own prediction buffer, the refusals, and
drivers/gen_pred.py --write png end to end."""
import ctypes as C
import importlib.util
import os
import zlib

import numpy as np
import pytest

import maps_u8_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(base=16, blocks=(2, 2, 3))
GN_CFG = dict(base=16, blocks=(1, 2, 2))


def _values(kind, shape, rng):
    if kind == "unit":
        return rng.random(shape).astype(np.float32)
    if kind == "normal":
        return rng.normal(0.0, 3.0, shape).astype(np.float32)
    if kind == "special":
        m = rng.normal(0.5, 0.5, shape).astype(np.float32)
        flat = m.reshape(-1)
        k = rng.choice(flat.size, size=max(3, flat.size // 50), replace=flat.size < 3)
        flat[k[0::3]] = np.nan
        flat[k[1::3]] = np.inf
        flat[k[2::3]] = -np.inf
        return m
    if kind == "halves":                          # k + 0.5 at scale 1: every exact half of [0, 255] and beyond
        return (rng.integers(-4, 260, shape) + 0.5).astype(np.float32)
    raise ValueError(kind)


SIZES = [((112, 112), (1080, 960)), ((112, 112), (112, 112)), ((112, 112), (37, 53)), ((7, 5), (1, 1)), ((1, 1), (9, 4))]


@pytest.mark.parametrize("src,dst", SIZES, ids=["112-1080x960", "112-112", "112-37x53", "7x5-1x1", "1x1-9x4"])
@pytest.mark.parametrize("n", [1, 37])
@pytest.mark.parametrize("kind", ["unit", "normal", "special", "halves"])
def test_resize_linear_u8_is_bit_exact_to_the_restatement(src, dst, n, kind):
    from sap3d_tensorflow_amd import dataflow as gdf
    rng = np.random.default_rng(zlib.crc32(repr((src, dst, n, kind)).encode()))
    m = _values(kind, (n,) + src, rng)
    scale = 1.0 if kind == "halves" else 255.0
    got = gdf.resize_linear_u8(m, dst, scale=scale)
    again = gdf.resize_linear_u8(m, dst, scale=scale)
    want = ref.maps_u8(m, dst[0], dst[1], scale)
    assert got.dtype == np.uint8 and got.shape == (n,) + dst
    assert np.array_equal(got, again)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    if n == 1:
        assert np.array_equal(gdf.resize_linear_u8(m[0], dst, scale=scale), want[0])        # [h, w] in, [H, W] out


def _session(structure, batch, **cfg):
    from sap3d_tensorflow_amd import P3DSession
    return P3DSession(structure, batch=batch, seed=0, **cfg)


@pytest.mark.parametrize("structure,cfg", [("unet", CFG), ("gn_p3d", GN_CFG)])
def test_pred_maps_u8_matches_the_restatement_of_the_prediction(structure, cfg):
    B, T = 4, 16
    s = _session(structure, B, **cfg)
    x = np.random.default_rng(3).normal(0.0, 0.5, s.x_shape).astype(np.float32)
    pred = s.predict_windows(x)[..., 0]
    first = [0, 15, 7, T]
    for scale, size in ((255.0, (1080, 960)), (255.0, (37, 53)), (1e10, (40, 30))):    # 1e10: products past int32 (-> 0)
        got = s.pred_maps_u8(first, size=size, scale=scale)
        again = s.pred_maps_u8(first, size=size, scale=scale)
        want = np.concatenate([ref.maps_u8(pred[b, f:], size[0], size[1], scale) for b, f in enumerate(first) if f < T])
        assert got.shape == (16 + 1 + 9, ) + size
        assert np.array_equal(got, again)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (structure, scale, size, len(bad), bad[:5])
        assert set(s.last_maps_ms) == {"device", "d2h"} and s.last_maps_ms["device"] > 0.0
    assert s.pred_maps_u8([T] * B).shape == (0, 1080, 960)
    s.close()


def test_refusals():
    from sap3d_tensorflow_amd import P3dError, lib
    from sap3d_tensorflow_amd import dataflow as gdf
    s = _session("unet", 2, **CFG)
    with pytest.raises(P3dError, match="no prediction"):
        s.pred_maps_u8([0, 0])                              # nothing has run yet
    s.predict_windows(np.zeros(s.x_shape, np.float32))
    for ff in ([-1, 0], [0, 17]):
        with pytest.raises(P3dError, match="first_frame"):
            s.pred_maps_u8(ff)
    for size in ((0, 960), (1080, 0)):
        with pytest.raises(P3dError, match="empty"):
            s.pred_maps_u8([15, 15], size=size)
    with pytest.raises(P3dError, match="int32"):
        s.pred_maps_u8([15, 16], size=(65536, 32768))
    with pytest.raises(ValueError):
        s.pred_maps_u8([0])                                 # one entry per clip
    assert s.pred_maps_u8([15, 15], size=(3, 2)).shape == (2, 3, 2)      # and the handle still works
    s.close()
    m = np.zeros((1, 4, 4), np.float32)
    one = np.zeros(1, np.uint8)
    f, u = m.ctypes.data_as(C.POINTER(C.c_float)), one.ctypes.data_as(C.POINTER(C.c_ubyte))
    assert lib().p3d_resize_linear_u8(0, f, 1, 4, 4, 255.0, 65536, 32768, u) != 0
    assert lib().p3d_resize_linear_u8(0, f, 1, 4, 4, 255.0, 0, 4, u) != 0
    assert lib().p3d_resize_linear_u8(0, f, 0, 4, 4, 255.0, 4, 4, u) != 0
    with pytest.raises(P3dError):
        gdf.resize_linear_u8(m, (4, 0))


def test_gen_pred_driver_png_equals_the_restatement_of_npy(tmp_path):
    from PIL import Image
    from sap3d_tensorflow_amd import P3DSession
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    videos = tmp_path / "videos"
    videos.mkdir()
    np.save(videos / "synth.npy", np.random.default_rng(0).integers(0, 256, (20, 120, 160, 3)).astype(np.uint8))
    sess = P3DSession("unet", batch=3, seed=4, base=16, blocks=(1, 1, 2))
    gp.run(sess, gp.parse_args(["--videos", str(videos), "--out", str(tmp_path / "npy"), "--batch", "3"]))
    gp.run(sess, gp.parse_args(["--videos", str(videos), "--out", str(tmp_path / "png"), "--batch", "3", "--write", "png",
                                "--time"]))
    sess.close()
    sal = np.load(tmp_path / "npy" / "synth.npy")
    assert sal.shape == (20, 112, 112)
    files = os.listdir(tmp_path / "png" / "synth")
    assert sorted(files) == sorted("frame_%d.png" % k for k in range(1, 21))
    want = ref.maps_u8(sal, 1080, 960)
    for f in range(20):
        got = np.asarray(Image.open(tmp_path / "png" / "synth" / ("frame_%d.png" % (f + 1))))
        assert got.dtype == np.uint8 and np.array_equal(got, want[f]), f
