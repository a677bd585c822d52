"""The smoothing / normalisation stage of P3DSession.set_postprocess on the GPU (csrc/postprocess.hip through the C ABI), held
bit for bit to the numpy replay of include/p3d_hip.h (tests/postprocess_ref.py) with the library's own taps: the blur alone,
the whole chain on supplied maps, the two users of a session's prediction (pred_maps_u8, evaluate), the refusals, and
drivers/gen_pred.py --write png end to end."""
import importlib.util
import os
import zlib

import numpy as np
import pytest

import postprocess_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(base=16, blocks=(2, 2, 3))
NORMS = ("none", "max", "range")


def _values(kind, shape, rng):
    if kind == "unit":
        return rng.random(shape).astype(np.float32)
    if kind == "normal":
        return rng.normal(0.0, 3.0, shape).astype(np.float32)
    if kind == "const":
        return np.full(shape, 0.37, np.float32)
    raise ValueError(kind)


def _exact(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


# (H, W, r): r = min - 1; a small, a middling and a near-full radius off every tile multiple; r just under a 64-row map;
# width and height off every tile multiple with r above a tile
BLUR_SHAPES = [(5, 7, 4), (37, 53, 1), (37, 53, 9), (37, 53, 36), (64, 64, 63), (130, 257, 128)]


@pytest.mark.parametrize("H,W,r", BLUR_SHAPES, ids=["%dx%d-r%d" % s for s in BLUR_SHAPES])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("kind", ["unit", "normal", "const"])
def test_gaussian_blur_is_bit_exact_to_the_replay(H, W, r, n, kind):
    from sap3d_tensorflow_amd import dataflow as gdf
    rng = np.random.default_rng(zlib.crc32(repr((H, W, r, n, kind)).encode()))
    m = _values(kind, (n, H, W), rng)
    sigma = max(0.5, r / 3.0)
    w = gdf.blur_taps(sigma, r)
    assert len(w) == 2 * r + 1
    got = gdf.gaussian_blur(m, sigma, r)
    _exact(got, ref.blur(m, w), (H, W, r, n, kind))
    assert np.array_equal(got, gdf.gaussian_blur(m, sigma, r))
    if n == 1:
        assert np.array_equal(gdf.gaussian_blur(m[0], sigma, r), got[0])           # [H, W] in, [H, W] out


def test_gaussian_blur_at_output_resolution():
    from sap3d_tensorflow_amd import dataflow as gdf
    m = np.random.default_rng(5).random((1, 1080, 960)).astype(np.float32)
    w = gdf.blur_taps(32.0)
    assert len(w) == 257                                                            # sigma 32 -> r 128
    got = gdf.gaussian_blur(m, 32.0)
    _exact(got, ref.blur(m, w), "1080x960 sigma 32")
    assert np.array_equal(got, gdf.gaussian_blur(m, 32.0))


def test_blur_commutes_with_flips_bit_for_bit():
    from sap3d_tensorflow_amd import dataflow as gdf
    m = np.random.default_rng(6).normal(0.0, 3.0, (2, 37, 53)).astype(np.float32)
    out = gdf.gaussian_blur(m, 3.0, 9)
    assert np.array_equal(gdf.gaussian_blur(m[:, :, ::-1], 3.0, 9), out[:, :, ::-1])
    assert np.array_equal(gdf.gaussian_blur(m[:, ::-1, :], 3.0, 9), out[:, ::-1, :])


@pytest.fixture(scope="module")
def source_maps():
    """float32 [3, 112, 112, 3]: channel 0 is the map (elem_stride 3), with negatives so that MAX and RANGE differ."""
    return np.random.default_rng(7).normal(0.3, 0.4, (3, 112, 112, 3)).astype(np.float32)


@pytest.fixture(scope="module")
def resized(source_maps):
    from oracle.dataflow import resize_linear
    m = np.ascontiguousarray(source_maps[..., 0])
    return dict((size, np.stack([resize_linear(k, size[0], size[1]) for k in m]).astype(np.float32))
                for size in ((37, 53), (112, 112), (1080, 960)))


@pytest.mark.parametrize("size,sigma,radius", [((37, 53), 2.0, 0), ((112, 112), 4.0, 7), ((1080, 960), 8.0, 0)],
                         ids=["37x53", "112x112", "1080x960"])
@pytest.mark.parametrize("stride", [1, 3])
def test_postprocess_maps_is_bit_exact_to_the_replay(source_maps, resized, size, sigma, radius, stride):
    from sap3d_tensorflow_amd import dataflow as gdf
    src = source_maps if stride == 3 else np.ascontiguousarray(source_maps[..., 0])
    n = 3 if size != (1080, 960) else 2
    src, base = src[:n], resized[size][:n]
    w = gdf.blur_taps(sigma, radius)
    assert np.array_equal(gdf.resize_linear(np.ascontiguousarray(source_maps[:n, :, :, 0]), size), base)
    _exact(gdf.postprocess_maps(src, size), base, "neutral")                      # neutral: the float32 resize alone
    blurred = ref.blur(base, w)                                                   # once: the replay of a 1080x960 blur takes seconds
    for norm in NORMS:
        f, b = gdf.postprocess_maps_both(src, size, sigma, radius, norm, scale=255.0)
        want = ref.normalise(blurred, norm)
        _exact(f, want, (size, norm, "f32"))
        _exact(b, ref.quantise(want, 255.0), (size, norm, "u8"))
        if size != (1080, 960):
            _exact(gdf.postprocess_maps(src, size, sigma, radius, norm), want, (size, norm, "f32 alone"))
            _exact(gdf.postprocess_maps(src, size, sigma, radius, norm, scale=255.0), b, (size, norm, "u8 alone"))
    _exact(gdf.postprocess_maps(src, size, norm="range", scale=200.0), ref.quantise(ref.normalise(base, "range"), 200.0), "no blur")


def test_postprocess_maps_beyond_one_chunk():
    """37 maps of 37 x 53: three chunks of 16, 16 and 5 maps, whose byte ranges meet inside a word (37 * 53 is odd)."""
    from oracle.dataflow import resize_linear
    from sap3d_tensorflow_amd import dataflow as gdf
    m = np.random.default_rng(8).random((37, 20, 24)).astype(np.float32)
    base = np.stack([resize_linear(k, 37, 53) for k in m]).astype(np.float32)
    w = gdf.blur_taps(1.5)
    f, b = gdf.postprocess_maps_both(m, (37, 53), 1.5, 0, "range", scale=255.0)
    want = ref.postprocess(base, w, "range")
    _exact(f, want, "f32")
    _exact(b, ref.quantise(want, 255.0), "u8")


def _session(batch):
    from sap3d_tensorflow_amd import P3DSession
    return P3DSession("unet", batch=batch, seed=0, **CFG)


def test_pred_maps_u8_runs_the_chain_on_the_prediction_and_is_untouched_when_off():
    from sap3d_tensorflow_amd import dataflow as gdf
    B, T = 4, 16
    s = _session(B)
    x = np.random.default_rng(3).normal(0.0, 0.5, s.x_shape).astype(np.float32)
    pred = s.predict_windows(x)[..., 0]
    first = [0, 15, T, 7]
    maps = np.concatenate([pred[b, f:] for b, f in enumerate(first)])
    assert len(maps) == 16 + 1 + 0 + 9
    size = (90, 80)
    off = gdf.resize_linear_u8(maps, size)
    assert s.postprocess is None
    _exact(s.pred_maps_u8(first, size=size), off, "off")
    base = gdf.resize_linear(maps, size)
    for sigma, radius, norm in ((2.0, 0, "range"), (3.0, 5, "max"), (0.0, 0, "max"), (1.0, 0, "none")):
        s.set_postprocess(sigma, radius, norm)
        assert s.postprocess == dict(sigma=sigma, radius=radius, norm=norm)
        got = s.pred_maps_u8(first, size=size)
        _exact(got, ref.postprocess(base, gdf.blur_taps(sigma, radius), norm, scale=255.0), (sigma, radius, norm))
        assert np.array_equal(got, s.pred_maps_u8(first, size=size))
    s.set_postprocess(None)
    assert s.postprocess is None
    _exact(s.pred_maps_u8(first, size=size), off, "off again")
    s.set_postprocess(2.0, 0, "range")
    s.set_postprocess()                                                               # the defaults switch it off as well
    _exact(s.pred_maps_u8(first, size=size), off, "off by the defaults")
    s.close()


def test_evaluate_scores_the_postprocessed_map():
    from sap3d_tensorflow_amd import dataflow as gdf
    from sap3d_tensorflow_amd import metrics as gm
    from sap3d_tensorflow_amd import synthetic
    size = (90, 80)
    x, dens, fix = synthetic.synthetic_test_set(2, 3, size=size, density_size=(45, 40), crop=48)      # clip 2 has no fixation
    from sap3d_tensorflow_amd import P3DSession
    s = P3DSession("unet", batch=3, seed=0, height=48, width=48, **CFG)
    pred = s.forward(x)[:, -1, :, :, 0]
    assert np.isfinite(pred).all()
    plain = s.evaluate(x, dens, fix, size=size, rng=np.random.RandomState(11))
    for post in (dict(sigma=2.0, radius=0, norm="range"), dict(sigma=0.0, radius=0, norm="max"), dict(sigma=1.5, radius=6, norm="none")):
        s.set_postprocess(**post)
        got = s.evaluate(x, dens, fix, size=size, rng=np.random.RandomState(11))
        full = gdf.postprocess_maps(pred, size, **post)
        assert np.isfinite(full).all()
        want = gm.evaluate_maps(full, dens, fix, size=size, rng=np.random.RandomState(11))
        assert np.array_equal(got, want, equal_nan=True), (post, got, want)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        hook = gm.evaluate_maps(pred, dens, fix, size=size, rng=np.random.RandomState(11), postprocess=post)
        assert np.array_equal(got, hook, equal_nan=True), post
    assert not np.array_equal(got, plain, equal_nan=True)
    s.set_postprocess(None)
    assert np.array_equal(s.evaluate(x, dens, fix, size=size, rng=np.random.RandomState(11)), plain, equal_nan=True)
    s.close()


def test_refusals_leave_the_setting_alone():
    from sap3d_tensorflow_amd import P3dError
    from sap3d_tensorflow_amd import dataflow as gdf
    s = _session(2)
    s.predict_windows(np.zeros(s.x_shape, np.float32))
    s.set_postprocess(2.0, 0, "range")
    keep = s.postprocess
    for sigma, radius in ((-1.0, 0), (float("nan"), 0), (float("inf"), 0), (1.0, -1), (1.0, 256), (0.0, 3), (64.0, 0)):
        with pytest.raises(P3dError, match="postprocess"):
            s.set_postprocess(sigma, radius, "none")
        assert s.postprocess == keep
    with pytest.raises(ValueError):
        s.set_postprocess(1.0, 0, "sum")
    from sap3d_tensorflow_amd import _lib, lib
    import ctypes as C
    bad = _lib.P3dPostprocess(1.0, 0, 7)
    assert lib().p3d_set_postprocess(s._h, C.byref(bad)) != 0 and s.postprocess == keep
    with pytest.raises(P3dError, match="radius 8 exceeds"):
        s.pred_maps_u8([15, 15], size=(8, 40))                                        # r = 8 > min(H, W) - 1 = 7, at call time
    assert s.postprocess == keep
    assert s.pred_maps_u8([15, 15], size=(9, 40)).shape == (2, 9, 40)                 # r = min - 1 runs, and the handle still works
    s.close()
    m = np.zeros((1, 6, 6), np.float32)
    with pytest.raises(P3dError, match="exceeds"):
        gdf.gaussian_blur(m, 1.0, 6)
    with pytest.raises(P3dError, match="exceeds"):
        gdf.postprocess_maps(m, (5, 9), 1.0, 5)
    with pytest.raises(ValueError):
        gdf.postprocess_maps(m, (5, 9), norm="sum")


def test_gen_pred_driver_png_with_blur_equals_the_session_path(tmp_path):
    from PIL import Image
    from sap3d_tensorflow_amd import P3DSession
    from sap3d_tensorflow_amd import dataflow as gdf
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    videos = tmp_path / "videos"
    videos.mkdir()
    np.save(videos / "synth.npy", np.random.default_rng(0).integers(0, 256, (20, 120, 160, 3)).astype(np.uint8))
    with pytest.raises(SystemExit) as e:
        gp.parse_args(["--videos", str(videos), "--write", "npy", "--blur-sigma", "2"])
    assert e.value.code != 0
    args = gp.parse_args(["--videos", str(videos), "--out", str(tmp_path / "png"), "--batch", "3", "--write", "png", "--size", "60", "50",
                          "--blur-sigma", "2", "--normalize", "range"])
    sess = P3DSession("unet", batch=3, seed=4, base=16, blocks=(1, 1, 2))
    sal = gp.predict_video(sess, gp.preprocess(np.load(videos / "synth.npy")), 3)
    sess.set_postprocess(args.blur_sigma, args.blur_radius, args.normalize)
    gp.run(sess, args)
    sess.close()
    assert sorted(os.listdir(tmp_path / "png" / "synth")) == sorted("frame_%d.png" % k for k in range(1, 21))
    want = gdf.postprocess_maps(sal, (60, 50), 2.0, 0, "range", scale=255.0)
    _exact(want, ref.postprocess(gdf.resize_linear(sal, (60, 50)), gdf.blur_taps(2.0), "range", scale=255.0), "session path")
    for f in range(20):
        got = np.asarray(Image.open(tmp_path / "png" / "synth" / ("frame_%d.png" % (f + 1))))
        assert got.dtype == np.uint8 and np.array_equal(got, want[f]), f
