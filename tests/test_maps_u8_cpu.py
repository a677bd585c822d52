"""gen_pred.py's 8-bit write-out without a GPU: the float64 restatement (tests/maps_u8_ref.py) against closed forms, its tables
against the float32 oracle's, and drivers/gen_pred.py's image mode with a stand-in session."""
import importlib.util
import os

import numpy as np
import pytest

import maps_u8_ref as ref
from oracle import dataflow as odf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _driver():
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


# ---- the restatement: closed forms ----------------------------------------------------------------------------------
def test_same_size_is_the_quantised_float32_product():
    m = np.random.default_rng(0).normal(0.5, 0.4, (3, 17, 23)).astype(np.float32)
    want = np.clip(np.rint((m * np.float32(255)).astype(np.float64)), 0, 255).astype(np.uint8)
    assert np.array_equal(ref.maps_u8(m, 17, 23), want)


def test_constant_map_stays_constant():
    """c (1 - w) + c w is c up to one rounding (1.f - w is not always exact): constants whose product is an exact half, such
    as 0.5 * 255 = 127.5 or float32(0.7) * 255 = 178.5, may land on either side of it, so none is used here."""
    for c in (0.0, 0.2, 0.6, 1.0):
        m = np.full((2, 112, 112), c, np.float32)
        q = int(np.rint(np.float64(np.float32(c) * np.float32(255))))
        for H, W in ((1080, 960), (37, 53), (1, 1), (112, 112)):
            assert np.all(ref.maps_u8(m, H, W) == q), (c, H, W)


def test_exact_halves_round_to_even():
    m = np.array([[0.5, 1.5, 2.5, 3.5, 4.5, 253.5, 254.5, 255.5]], np.float32)
    assert ref.maps_u8(m, 1, 8, scale=1.0).tolist() == [[0, 2, 2, 4, 4, 254, 254, 255]]
    # through a resize whose weights are multiples of 1/4 (x 2 upscale: 1 - w exact), a constant half stays a half
    assert np.all(ref.maps_u8(np.full((7, 5), 2.5, np.float32), 14, 10, scale=1.0) == 2)
    assert np.all(ref.maps_u8(np.full((7, 5), 3.5, np.float32), 14, 10, scale=1.0) == 4)


def test_out_of_range_values_give_the_defined_bytes():
    v = np.array([[-1.0, -0.5, -0.49, 255.49, 255.5, 256.0, 1e6, 2.0 ** 31 - 1, 2.0 ** 31, -2.0 ** 31, -2.0 ** 31 - 512,
                   3e38, np.inf, -np.inf, np.nan]], np.float64)
    got = ref.quantise(v).tolist()[0]
    assert got == [0, 0, 0, 255, 255, 255, 255, 255, 0, 0, 0, 0, 0, 0, 0]
    # 2^31 - 0.5 rounds (half to even) to 2^31: outside int32
    assert ref.quantise(np.array([2.0 ** 31 - 0.5, 2.0 ** 31 - 1.5])).tolist() == [0, 255]
    # the same through the map path (same size: a copy); float32 2^31 is exactly 2^31
    m = np.array([[-3.0, 300.0, 2.0 ** 31, np.inf, -np.inf, np.nan, 1e10, 100.4]], np.float32)
    assert ref.maps_u8(m, 1, 8, scale=1.0).tolist() == [[0, 255, 0, 0, 0, 0, 0, 100]]


def test_resize_of_an_inf_is_nan_where_a_weight_is_zero():
    """The tables' clamped border multiplies its second tap by 0: an inf there gives inf * 0 = NaN -> 0, as the float32 path."""
    m = np.zeros((2, 2), np.float32)
    m[:, 1] = np.inf
    out = ref.maps_u8(m, 2, 4, scale=1.0)        # x centres -0.25, 0.25, 0.75, 1.25: clamped, inside, inside, clamped
    assert out.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0]]


def test_weight_tables_are_the_float32_oracles():
    for dst, src in ((1080, 112), (960, 112), (37, 112), (1, 7), (9, 1), (112, 112)):
        x0, x1, wx = odf._coef(dst, src)
        scale = float(src) / float(dst)
        f = ((np.arange(dst) + 0.5) * scale - 0.5).astype(np.float32)
        s = np.floor(f).astype(np.int64)
        w = (f - s.astype(np.float32)).astype(np.float32)
        w[(s < 0) | (s >= src - 1)] = 0
        s = np.clip(s, 0, src - 1)
        assert np.array_equal(x0, s) and np.array_equal(x1, np.minimum(s + 1, src - 1)) and np.array_equal(wx, w)
    # and the restatement's interior equals a hand-written double bilinear of the float32 product
    m = np.random.default_rng(1).random((5, 6)).astype(np.float32)
    x0, x1, wx = odf._coef(13, 6)
    y0, y1, wy = odf._coef(11, 5)
    s = (m * np.float32(255)).astype(np.float64)
    y, x = 4, 7
    ax, ay = np.float64(np.float32(1) - wx[x]), np.float64(np.float32(1) - wy[y])
    r0 = s[y0[y], x0[x]] * ax + s[y0[y], x1[x]] * np.float64(wx[x])
    r1 = s[y1[y], x0[x]] * ax + s[y1[y], x1[x]] * np.float64(wx[x])
    assert ref.resize_f64(s, 11, 13)[y, x] == r0 * ay + r1 * np.float64(wy[y])


# ---- drivers/gen_pred.py --write png / jpg with a stand-in session ---------------------------------------------------
class FakeSession:
    """predict_windows: frame t of clip k is the constant (its frame tag) / 40; pred_maps_u8: the restatement of it."""
    def __init__(self, batch):
        self.x_shape = (batch, 16, 112, 112, 3)
        self.calls = []

    def predict_windows(self, clips):
        self.pred = np.broadcast_to(clips[:, :, :1, :1, :1] / np.float32(40), clips.shape[:4] + (1,)).astype(np.float32)
        return self.pred

    def pred_maps_u8(self, first_frame, size=(1080, 960), scale=255.):
        self.calls.append(list(first_frame))
        out = [ref.maps_u8(self.pred[b, t, :, :, 0], size[0], size[1], scale) for b, f in enumerate(first_frame) for t in range(f, 16)]
        self.last_maps_ms = dict(device=0.5, d2h=0.25)
        return np.stack(out) if out else np.zeros((0,) + tuple(size), np.uint8)


def _tagged_video(F):
    return np.arange(F, dtype=np.float32)[:, None, None, None] * np.ones((1, 112, 112, 3), np.float32)


def test_image_mode_writes_every_frame_once(tmp_path):
    gp = _driver()
    F, batch = 20, 3
    sess = FakeSession(batch)
    seen = []
    for idx, maps in gp.predict_video_images(sess, _tagged_video(F), batch, size=(9, 7)):
        assert len(idx) == len(maps)
        for f, m in zip(idx, maps):
            seen.append(f)
            assert np.all(m == ref.maps_u8(np.full((1, 1), f / np.float32(40), np.float32), 9, 7)[0]), f   # frame f's map
    assert sorted(seen) == list(range(F))
    # windows 0..4 in batches of 3: the second batch pads one clip, which writes nothing
    assert sess.calls == [[0, 15, 15], [15, 15, 16]]

    out = tmp_path / "v"
    out.mkdir()
    t = gp.write_video_images(sess, _tagged_video(F), batch, str(out), "png", size=(9, 7), writers=2)
    assert t["files"] == F and t["device"] == 1.0 and t["d2h"] == 0.5
    assert sorted(os.listdir(out)) == sorted("frame_%d.png" % (f + 1) for f in range(F))


def test_driver_image_mode_files_and_skip(tmp_path, monkeypatch):
    from PIL import Image
    gp = _driver()
    videos = tmp_path / "videos"
    videos.mkdir()
    np.save(videos / "clipA.npy", np.zeros((17, 8, 8, 3), np.uint8))
    np.save(videos / "clipB.npy", np.zeros((18, 8, 8, 3), np.uint8))
    out = tmp_path / "pred"
    (out / "clipB").mkdir(parents=True)                 # already written: skipped, as gen_pred.py:83-86 does
    # smooth per-frame maps of different levels, so that a PNG read back checks the pixels and a JPEG its error
    yy, xx = np.mgrid[0:112, 0:112]
    base = (0.5 + 0.45 * np.sin(yy / 17.0) * np.cos(xx / 23.0)).astype(np.float32)

    def preprocess(video):
        return np.stack([np.repeat((base * (0.6 + 0.02 * f))[:, :, None], 3, axis=2) for f in range(len(video))])
    monkeypatch.setattr(gp, "preprocess", preprocess)

    class MapSession(FakeSession):
        def predict_windows(self, clips):
            self.pred = clips[..., :1].astype(np.float32)
            return self.pred

    args = gp.parse_args(["--videos", str(videos), "--out", str(out), "--write", "png", "--batch", "2", "--size", "60", "44",
                          "--time"])
    sess = MapSession(2)
    gp.run(sess, args)
    assert os.listdir(out / "clipB") == []
    files = sorted(os.listdir(out / "clipA"), key=lambda n: int(n[6:-4]))
    assert files == ["frame_%d.png" % k for k in range(1, 18)]
    for f in (0, 9, 16):
        got = np.asarray(Image.open(out / "clipA" / ("frame_%d.png" % (f + 1))))
        assert got.dtype == np.uint8 and np.array_equal(got, ref.maps_u8(base * np.float32(0.6 + 0.02 * f), 60, 44))

    args = gp.parse_args(["--videos", str(videos), "--out", str(tmp_path / "jpg"), "--write", "jpg", "--batch", "3"])
    gp.run(MapSession(3), args)
    assert len(os.listdir(tmp_path / "jpg" / "clipA")) == 17 and len(os.listdir(tmp_path / "jpg" / "clipB")) == 18
    got = np.asarray(Image.open(tmp_path / "jpg" / "clipB" / "frame_18.jpg"))
    want = ref.maps_u8(base * np.float32(0.6 + 0.02 * 17), 1080, 960)
    assert got.shape == (1080, 960)
    assert np.abs(got.astype(np.float64) - want).mean() <= 1.0


def test_driver_default_is_npy_and_writers_are_capped():
    gp = _driver()
    args = gp.parse_args(["--videos", "x"])
    assert args.write == "npy" and tuple(args.size) == (1080, 960) and args.writers == 4
    with pytest.raises(SystemExit):
        gp.parse_args(["--videos", "x", "--writers", "17"])
