"""Histogram matching on the GPU (csrc/hist_match.hip through the C ABI), held bit for bit to the numpy replay of
include/p3d_hip.h (tests/hist_match_ref.py, itself held to np.histogram / np.interp by tests/test_hist_match_cpu.py): the tables,
the remap on supplied maps, the stage inside the postprocess chain, the three users of a session's prediction, the refusals, and
that training never sees the option.  Tolerance 0 everywhere the law is the reference: it is fully specified in IEEE double."""
import zlib

import numpy as np
import pytest

import hist_match_ref as ref
import postprocess_ref as pref

pytestmark = pytest.mark.gpu

CFG = dict(base=16, blocks=(2, 2, 3))
SHAPES = [(5, 7), (37, 53), (130, 257)]


def _exact(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bits = np.uint64 if got.dtype == np.float64 else np.uint32 if got.dtype == np.float32 else got.dtype
    bad = np.argwhere(got.view(bits) != want.view(bits))
    assert bad.size == 0, (what, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


def _tables(maps, nb):
    t = [ref.cumulative_distribution(m, nb) for m in maps]
    return tuple(np.stack([k[i] for k in t]) for i in range(3))


@pytest.mark.parametrize("H,W", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("nb", [256, 7])
def test_tables_and_matched_maps_are_bit_exact_to_the_replay(H, W, n, nb):
    from sap3d_tensorflow_amd import dataflow as gdf
    for kind in ref.KINDS:
        rng = np.random.default_rng(zlib.crc32(repr((H, W, n, nb, kind)).encode()))
        m = ref.values(kind, (n, H, W), rng)
        cdf, centre, count = _tables(m, nb)
        got = gdf.cumulative_distribution(m, nb, with_counts=True)
        assert np.array_equal(got[2], count), (kind, "counts")
        _exact(got[0], cdf, (kind, "cdf"))
        _exact(got[1], centre, (kind, "centres"))
        again = gdf.cumulative_distribution(m, nb)
        _exact(again[0], cdf, (kind, "cdf again"))
        # per-map target images (the reference's recipe), one of them 3-valued: long runs of equal cdf entries
        targets = np.stack([ref.values(("three", "normal", "skewed")[k % 3], (H, W), rng) for k in range(n)])
        out = gdf.match_hist_maps(m, targets, nb)
        _exact(out, ref.match_hist_maps(m, targets, nb), (kind, "per-map targets"))
        assert np.array_equal(out, gdf.match_hist_maps(m, targets, nb))
        tc, tx, _ = _tables(targets, nb)
        _exact(gdf.match_hist(m, tc, tx, nb), out, (kind, "the same through supplied per-map tables"))
        # one shared table, of another length than nb
        sc, sx, _ = ref.cumulative_distribution(ref.values("three", (H, W), rng), 64)
        shared = gdf.match_hist(m, sc, sx, nb)
        _exact(shared, ref.match_table(m, sc, sx, nb), (kind, "shared table"))
        if n == 1:
            _exact(gdf.match_hist(m[0], sc, sx, nb), shared[0], (kind, "[H, W] in, [H, W] out"))
            one = gdf.cumulative_distribution(m[0], nb)
            assert one[0].shape == (nb,) and np.array_equal(one[0], cdf[0]) and np.array_equal(one[1], centre[0])


@pytest.mark.parametrize("seed,nb", ref.EDGE_CASES)
def test_values_a_rounding_away_from_an_edge_take_the_fix_ups(seed, nb):
    from sap3d_tensorflow_amd import dataflow as gdf
    m = ref.edge_values(seed, nb)[None]                                              # [1, 1, L]
    cdf, centre, count = ref.cumulative_distribution(m, nb)
    got = gdf.cumulative_distribution(m, nb, with_counts=True)
    assert np.array_equal(got[2][0], count)
    _exact(got[0][0], cdf, "cdf")
    _exact(got[1][0], centre, "centres")
    _exact(gdf.match_hist_maps(m, m[:, :, ::-1] * np.float32(0.5), nb), ref.match_hist_maps(m, m[:, :, ::-1] * np.float32(0.5), nb), "match")


def test_at_output_resolution():
    from sap3d_tensorflow_amd import dataflow as gdf
    rng = np.random.default_rng(5)
    m = ref.values("skewed", (1, 1080, 960), rng)
    t = ref.values("normal", (1, 1080, 960), rng)
    cdf, centre, count = _tables(m, 256)
    got = gdf.cumulative_distribution(m, 256, with_counts=True)
    assert np.array_equal(got[2], count)
    _exact(got[0], cdf, "cdf")
    _exact(got[1], centre, "centres")
    out = gdf.match_hist_maps(m, t, 256)
    _exact(out, ref.match_hist_maps(m, t, 256), "1080x960")
    assert np.array_equal(out, gdf.match_hist_maps(m, t, 256))


@pytest.fixture(scope="module")
def source_maps():
    """float32 [3, 112, 112, 3]: channel 0 is the map (elem_stride 3)."""
    return np.random.default_rng(7).normal(0.3, 0.4, (3, 112, 112, 3)).astype(np.float32)


@pytest.fixture(scope="module")
def table():
    """A target table of 64 entries: a peaked density-like histogram."""
    cdf, centre, _ = ref.cumulative_distribution(ref.values("skewed", (64, 64), np.random.default_rng(9)), 64)
    return cdf, centre


@pytest.mark.parametrize("size", [(37, 53), (224, 200)], ids=["37x53", "224x200"])
def test_stage_in_the_postprocess_chain(source_maps, table, size):
    from oracle.dataflow import resize_linear
    from sap3d_tensorflow_amd import dataflow as gdf
    base = np.stack([resize_linear(k, size[0], size[1]) for k in np.ascontiguousarray(source_maps[..., 0])]).astype(np.float32)
    for nb in (256, 7):
        want = ref.match_table(base, table[0], table[1], nb)
        _exact(gdf.postprocess_maps(source_maps, size, hist_match=table, nbins=nb), want, (size, nb, "MATCH alone"))
    sigma = 2.0
    blurred = pref.blur(base, gdf.blur_taps(sigma))
    want = pref.normalise(ref.match_table(blurred, table[0], table[1], 256), "range")
    _exact(gdf.postprocess_maps(source_maps, size, sigma, 0, "range", hist_match=table), want, (size, "blur + MATCH + range"))
    _exact(gdf.postprocess_maps(source_maps, size, sigma, 0, "range", scale=255.0, hist_match=table), pref.quantise(want, 255.0),
           (size, "blur + MATCH + range + bytes"))
    # without the option the entry point returns what it returned before
    _exact(gdf.postprocess_maps(source_maps, size, sigma, 0, "range"), pref.normalise(blurred, "range"), (size, "off"))
    _exact(gdf.postprocess_maps(source_maps, size, sigma, 0, "range", hist_match="off"), pref.normalise(blurred, "range"), (size, "off, named"))


def _session(batch, **kw):
    from sap3d_tensorflow_amd import P3DSession
    return P3DSession("unet", batch=batch, seed=0, **dict(CFG, **kw))


def test_evaluate_scores_the_matched_map(table):
    import eval_maps_ref as R
    from oracle import dataflow as odf
    from oracle import evaluation as oev
    from sap3d_tensorflow_amd import dataflow as gdf
    from sap3d_tensorflow_amd import metrics as gm
    from test_gpu_eval import _check
    size = (90, 80)
    s = _session(3, height=48, width=48)
    x = np.random.default_rng(3).normal(0.0, 0.5, s.x_shape).astype(np.float32)
    pred = s.forward(x)[:, -1, :, :, 0]
    full = np.stack([odf.resize_linear(p, *size) for p in pred]).astype(np.float32)
    rng = np.random.default_rng(4)
    spread = np.stack([(f - f.min()) / (f.max() - f.min()) for f in full])        # the ground truth follows the prediction
    dens = np.stack([R._density(rng, f) for f in spread])
    fix = np.stack([R._fixation(rng, f, k) for f, k in zip(spread, (300, 0, 50))])
    assert s.hist_match is None
    plain = s.evaluate(x, dens, fix, size=size, rng=np.random.RandomState(11))
    dens_f64 = np.stack([odf.resize_linear_u8(d, *size) for d in dens]) / 255.
    for target, nb, post in (("density", 256, None), ("density", 7, dict(sigma=1.5, radius=0, norm="range")), (table, 256, None)):
        s.set_postprocess(**post) if post else s.set_postprocess(None)
        s.set_hist_match(target, nb)
        hm = s.hist_match
        assert hm["nbins"] == nb and hm["mode"] == ("density" if target == "density" else "table")
        if target != "density":
            assert np.array_equal(hm["cdf"], table[0]) and np.array_equal(hm["bin_centers"], table[1])
        got = s.evaluate(x, dens, fix, size=size, rng=np.random.RandomState(11))
        hook = gm.evaluate_maps(pred, dens, fix, size=size, rng=np.random.RandomState(11), postprocess=post, hist_match=target, nbins=nb)
        assert np.array_equal(got, hook, equal_nan=True), (target if target == "density" else "table", nb, got, hook)
        assert not np.array_equal(got, plain, equal_nan=True)
        # the replay, then the float64 oracle of test.py's loop body on the matched map
        maps = pref.blur(full, gdf.blur_taps(post["sigma"])) if post else full
        if target == "density":
            maps = ref.match_hist_maps(maps, dens_f64, nb)
        else:
            maps = ref.match_table(maps, table[0], table[1], nb)
        if post:
            maps = pref.normalise(maps, post["norm"])
        r = np.random.RandomState(11)
        for b in range(3):
            with np.errstate(all="ignore"):
                want = oev.test_py_clip_metrics(maps[b], dens[b], fix[b], rng=r)
            print(b, got[b], want)
            _check(got[b], want)
    s.set_postprocess(None)
    s.set_hist_match("off")
    assert s.hist_match is None
    assert np.array_equal(s.evaluate(x, dens, fix, size=size, rng=np.random.RandomState(11)), plain, equal_nan=True)
    s.close()


def test_written_maps_under_a_table_and_untouched_when_off(table):
    from sap3d_tensorflow_amd import P3dError
    from sap3d_tensorflow_amd import dataflow as gdf
    B, T = 2, 16
    s = _session(B)
    x = np.random.default_rng(3).normal(0.0, 0.5, s.x_shape).astype(np.float32)
    pred = s.predict_windows(x)[..., 0]
    first = [0, 15]
    maps = np.concatenate([pred[b, f:] for b, f in enumerate(first)])
    size = (90, 80)
    off = s.pred_maps_u8(first, size=size)
    _exact(off, gdf.resize_linear_u8(maps, size), "off")
    base = gdf.resize_linear(maps, size)
    s.set_hist_match(table, 256)
    got = s.pred_maps_u8(first, size=size)
    _exact(got, pref.quantise(ref.match_table(base, table[0], table[1], 256), 255.0), "table, postprocess off")
    assert np.array_equal(got, s.pred_maps_u8(first, size=size))
    s.set_postprocess(2.0, 0, "range")
    s.set_hist_match(table, 7)
    want = pref.normalise(ref.match_table(pref.blur(base, gdf.blur_taps(2.0)), table[0], table[1], 7), "range")
    _exact(s.pred_maps_u8(first, size=size), pref.quantise(want, 255.0), "blur + table + range")
    s.set_postprocess(None)
    # the resident video's maps take the same chain
    frames = np.random.default_rng(5).normal(0.0, 0.5, (T + 1,) + s.x_shape[2:]).astype(np.float32)
    s.open_video(T + 1)
    s.video_put(0, frames)
    s.video_predict([0, 1])
    vmaps = s.video_maps(0, T + 1)
    s.set_hist_match("off")
    voff = s.video_maps_u8(0, T + 1, size=size)
    s.set_hist_match(table, 256)
    _exact(s.video_maps_u8(0, T + 1, size=size), pref.quantise(ref.match_table(gdf.resize_linear(vmaps, size), table[0], table[1], 256), 255.0),
           "video, table")
    # the density mode has no ground truth here: refused by both, and nothing changes
    s.set_hist_match("density")
    for call in (lambda: s.pred_maps_u8([15, 15], size=size), lambda: s.video_maps_u8(0, T + 1, size=size)):
        with pytest.raises(P3dError, match="P3D_MATCH_DENSITY"):
            call()
    assert s.hist_match == dict(mode="density", nbins=256)
    s.set_hist_match("off")
    _exact(s.video_maps_u8(0, T + 1, size=size), voff, "video, off again")
    s.close_video()
    s.predict_windows(x)
    _exact(s.pred_maps_u8(first, size=size), off, "off again")
    s.close()


def test_refusals_leave_the_setting_alone(table):
    import ctypes as C
    from sap3d_tensorflow_amd import P3dError, _lib, lib
    s = _session(2)
    s.set_hist_match(table, 64)
    keep = s.hist_match

    def same():
        now = s.hist_match
        return now["mode"] == keep["mode"] and now["nbins"] == 64 and np.array_equal(now["cdf"], keep["cdf"])

    bad = table[0].copy()
    bad[5] = np.nan
    down = table[0].copy()
    down[6] = down[5] - 1e-6
    for target, nb, word in ((table, 1, "nbins"), (table, 1025, "nbins"), ((bad, table[1]), 256, "finite"), ((table[0], bad), 256, "finite"),
                             ((down, table[1]), 256, "non-decreasing"), ((table[0][:1], table[1][:1]), 256, "nt"), ("density", 0, "nbins")):
        with pytest.raises(P3dError, match=word):
            s.set_hist_match(target, nb)
        assert same()
    for cfg in (_lib.P3dHistMatch(7, 256, 0, None, None), _lib.P3dHistMatch(1, 256, 8, None, None)):
        assert lib().p3d_set_hist_match(s._h, C.byref(cfg)) != 0 and same()
    s.close()


def test_training_never_sees_the_option(table):
    out = []
    for on in (False, True):
        s = _session(2, height=48, width=48)
        if on:
            s.set_hist_match(table, 256)
        x = np.random.default_rng(6).normal(0.0, 0.5, s.x_shape).astype(np.float32)
        y = np.random.default_rng(7).random(s.y_shape).astype(np.float32)
        loss = s.train_step(x, y, dropout=0.5, seed=3)
        name = s.variables()[0][0]
        out.append((np.float32(loss), s.get_param(name).copy()))
        s.close()
    assert out[0][0].view(np.uint32) == out[1][0].view(np.uint32)
    assert np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))
