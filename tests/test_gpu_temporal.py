"""Temporal smoothing of a resident video's maps on the GPU (csrc/temporal.hip through the C ABI): the launch at op level through
p3d_debug_video_temporal against tests/temporal_ref.py -- every device buffer `offset` elements past a 16-byte boundary between
guards -- then the session's two read-outs, the refusals, the isolation of the train step and the driver's --temporal path.
Every comparison is bit for bit (uint32 views)."""
import ctypes as C
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import temporal_ref as tr     # noqa: E402
import video_ref as vr        # noqa: E402

T = 16
_i32p = C.POINTER(C.c_int32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _gen_pred():
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


# ---- the hook ---------------------------------------------------------------------------------------------------------------
def hook(mode, setting, store, count, first, n, offset, out=None):
    """p3d_debug_video_temporal: setting = (kind, sigma, radius, alpha); store [F, hw], count [F] -> [n, hw].  The hook itself
    fails when the launch changed the store, the counts or a guard."""
    from sap3d_tensorflow_amd import _lib
    from sap3d_tensorflow_amd._lib import check, fptr
    F, hw = store.shape
    cnt = np.ascontiguousarray(count, np.int32)
    out = np.empty((max(n, 0), hw), np.float32) if out is None else out
    cfg = _lib.P3dVideoTemporal(*setting)
    check(_lib.lib().p3d_debug_video_temporal(0, mode, C.byref(cfg), fptr(store), cnt.ctypes.data_as(_i32p), F, hw, first, n, offset, fptr(out)))
    return out


@functools.lru_cache(maxsize=None)
def _case(F, hw, mode):
    """(store, count) of a video: NEWEST maps with every count 1; MEAN sums with counts 1 .. 5, a count-1 frame holding -0.0
    and a denormal.  Shared by the tests and never written."""
    rng = np.random.default_rng(F * 4096 + hw + mode)
    store = rng.standard_normal((F, hw)).astype(np.float32)
    if mode == vr.NEWEST:
        count = np.ones(F, np.int32)
    else:
        count = (1 + np.arange(F) * 3 % 5).astype(np.int32)          # 1, 4, 2, 5, 3, ...
        assert count[0] == 1 and count[5] == 1 and set(count.tolist()) == {1, 2, 3, 4, 5}
        store *= count[:, None].astype(np.float32)
        store[5, :2] = (-0.0, 1e-45)
        store[1, 2] = 1e-44                                              # a denormal that is divided
    store.setflags(write=False)
    count.setflags(write=False)
    return store, count


@functools.lru_cache(maxsize=None)
def _want(F, hw, mode, setting):
    store, count = _case(F, hw, mode)
    full = tr.filter_maps(tr.parse(*setting), mode, store, count)
    full.setflags(write=False)
    return full


def _plan(kind, r, hw, n):
    from sap3d_tensorflow_amd import dataflow
    return dataflow.temporal_plan(kind, r, hw, n)


def _reads(F):
    return [(0, F), (0, 1), (F - 1, 1), (5, 7)]


GAUSS_SHAPES = [(F, hw, r) for F in (16, 41) for hw in (35, 1024) for r in (1, 15, 24) if r <= F - 1]
SIGMA = {1: 0.8, 7: 2.5, 8: 2.5, 15: 5.0, 24: 8.0}


@pytest.mark.parametrize("mode", [vr.NEWEST, vr.MEAN], ids=["newest", "mean"])
@pytest.mark.parametrize("F,hw,r", GAUSS_SHAPES)
def test_gauss_matches_the_replay(F, hw, r, mode):
    setting = (tr.GAUSS, SIGMA[r], r, 0.0)
    store, count = _case(F, hw, mode)
    want = _want(F, hw, mode, setting)
    reads = _reads(F)
    # one read that starts in one block's run of frames and ends in the next
    seam = [n for n in range(F - 3, 1, -1) if _plan("gauss", r, hw, n)[1] < n]
    if seam:
        n = seam[0]
        fpb = _plan("gauss", r, hw, n)[1]
        assert 3 + fpb < 3 + n <= F
        reads.append((3, n))
    assert seam or (F, r) in ((16, 15), (41, 24)), "a seam along the frame axis is tested wherever the plan has one"
    for offset in range(4):
        for first, n in reads:
            got = hook(mode, setting, store, count, first, n, offset)
            assert np.array_equal(bits(got), bits(want[first:first + n])), (offset, first, n)
    if F == 16 and r == 15:
        assert all(tr.rho(0 - d, F) != 0 - d for d in range(1, r + 1))      # every tap of frame 0 reflects on one side


@pytest.mark.parametrize("hw", [35, 1024])
def test_gauss_either_side_of_the_radius_where_the_lane_layout_changes(hw):
    """Up to r = 7 a lane owns four pixels, from r = 8 on one (the ring must fit 64 KB): both sides of that threshold."""
    F = 41
    assert _plan("gauss", 7, hw, F)[0] == 4 * _plan("gauss", 8, hw, F)[0]
    for r in (7, 8):
        setting = (tr.GAUSS, SIGMA[r], r, 0.0)
        store, count = _case(F, hw, vr.MEAN)
        want = _want(F, hw, vr.MEAN, setting)
        for offset in range(4):
            for first, n in ((0, F), (5, 7)):
                got = hook(vr.MEAN, setting, store, count, first, n, offset)
                assert np.array_equal(bits(got), bits(want[first:first + n])), (r, offset, first, n)


def test_gauss_has_seams_along_the_frame_axis_at_the_tested_shapes():
    assert _plan("gauss", 1, 1024, 41)[1] < 41 and _plan("gauss", 15, 1024, 41)[1] < 41 and _plan("gauss", 1, 35, 16)[1] < 16


@pytest.mark.parametrize("r", [1, 15, 24])
@pytest.mark.parametrize("tail", [36, 37], ids=["vec", "scalar"])
def test_gauss_over_two_pixel_strips(r, tail):
    F = 41
    ppb = _plan("gauss", r, 4096, F)[0]
    hw = ppb + tail
    assert _plan("gauss", r, hw, F)[0] == ppb and ppb < hw < 2 * ppb
    setting = (tr.GAUSS, SIGMA[r], r, 0.0)
    store, count = _case(F, hw, vr.MEAN)
    want = _want(F, hw, vr.MEAN, setting)
    for offset in range(4):
        for first, n in ((0, F), (5, 7)):
            got = hook(vr.MEAN, setting, store, count, first, n, offset)
            assert np.array_equal(bits(got), bits(want[first:first + n])), (offset, first, n)


@pytest.mark.parametrize("mode", [vr.NEWEST, vr.MEAN], ids=["newest", "mean"])
@pytest.mark.parametrize("alpha", [0.0, 0.5, 0.9375])
@pytest.mark.parametrize("F,hw", [(F, hw) for F in (16, 41) for hw in (35, 1024)])
def test_ema_matches_the_replay(F, hw, alpha, mode):
    setting = (tr.EMA, 0.0, 0, alpha)
    store, count = _case(F, hw, mode)
    want = _want(F, hw, mode, setting)
    if alpha == 0.0 and mode == vr.NEWEST:
        assert np.array_equal(bits(want[0]), bits(store[0]))               # m_0 is a copy of the bits
    for offset in range(4):
        for first, n in _reads(F) + [(3, F - 3)]:
            got = hook(mode, setting, store, count, first, n, offset)
            assert np.array_equal(bits(got), bits(want[first:first + n])), (offset, first, n)


def test_ema_with_four_elements_per_lane_where_hw_is_large():
    """The kernel takes another path from hw = 2^18 on (float4 lanes, with 16-byte aligned bases): the smallest such hw whose last
    block is not full, aligned (offset 0) and not (offset 1: one element per lane again)."""
    F, hw = 16, (1 << 18) + 4
    assert _plan("ema", 0, hw, F)[0] == 4 * _plan("ema", 0, 1024, F)[0]
    setting = (tr.EMA, 0.0, 0, 0.5)
    store, count = _case(F, hw, vr.MEAN)
    want = _want(F, hw, vr.MEAN, setting)
    for offset, (first, n) in ((0, (0, F)), (0, (11, 3)), (1, (2, 14))):
        got = hook(vr.MEAN, setting, store, count, first, n, offset)
        assert np.array_equal(bits(got), bits(want[first:first + n])), (offset, first, n)


@pytest.mark.parametrize("F,hw,r", [(41, 1024, 24), (16, 35, 15), (41, 35, 1)])
def test_gauss_commutes_with_time_reversal_on_the_device(F, hw, r):
    setting = (tr.GAUSS, SIGMA[r], r, 0.0)
    store, count = _case(F, hw, vr.MEAN)
    rs, rc = np.ascontiguousarray(store[::-1]), np.ascontiguousarray(count[::-1])
    for offset in (0, 3):
        a = hook(vr.MEAN, setting, rs, rc, 0, F, offset)
        b = hook(vr.MEAN, setting, store, count, 0, F, offset)
        assert np.array_equal(bits(a), bits(b[::-1])), offset


def test_hook_refusals_leave_the_outputs_untouched():
    from sap3d_tensorflow_amd import P3dError
    F, hw = 16, 35
    store, _ = _case(F, hw, vr.NEWEST)
    ones = np.ones(F, np.int32)
    out = np.full((F, hw), 7.0, np.float32)

    def refused(setting, count, first, n, match):
        with pytest.raises(P3dError, match=match):
            hook(vr.MEAN, setting, store, count, first, n, 0, out)
        assert np.all(out == 7.0)

    refused((tr.GAUSS, 4.0, 16, 0.0), ones, 0, F, "F - 1")                 # r > F - 1
    count = ones.copy()
    count[9] = 0
    refused((tr.GAUSS, 1.0, 3, 0.0), count, 3, 4, r"frame 9\b")            # frames 3 .. 6 with r = 3 need 0 .. 9
    refused((tr.EMA, 0.0, 0, 0.5), count, 8, 4, r"frame 9\b")              # frames 8 .. 11 need 0 .. 11
    refused((tr.EMA, 0.0, 0, 1.0), ones, 0, F, "alpha")
    refused((tr.EMA, 0.0, 0, -0.5), ones, 0, F, "alpha")
    refused((tr.GAUSS, float("nan"), 2, 0.0), ones, 0, F, "sigma")
    # an unneeded frame of count 0 is accepted: GAUSS r = 3 on frames 2 .. 5 needs 0 .. 8, EMA on 2 .. 8 needs 0 .. 8
    cfg = tr.parse(tr.GAUSS, 1.0, 3)
    got = hook(vr.MEAN, (tr.GAUSS, 1.0, 3, 0.0), store, count, 2, 4, 1)
    assert np.array_equal(bits(got), bits(tr.filter_maps(cfg, vr.MEAN, store, count, 2, 4)))
    got = hook(vr.MEAN, (tr.EMA, 0.0, 0, 0.5), store, count, 2, 7, 1)
    assert np.array_equal(bits(got), bits(tr.filter_maps(tr.parse(tr.EMA, alpha=0.5), vr.MEAN, store, count, 2, 7)))


@pytest.mark.parametrize("kind", ["gauss", "ema"])
def test_temporal_filter_equals_the_hook_with_counts_of_one(kind):
    from sap3d_tensorflow_amd import dataflow
    F, H, W = 20, 5, 7
    store, count = _case(F, H * W, vr.NEWEST)
    setting = (tr.GAUSS, 1.5, 0, 0.0) if kind == "gauss" else (tr.EMA, 0.0, 0, 0.75)
    maps = store.reshape(F, H, W)
    for first, n in ((0, F), (3, 5)):
        got = dataflow.temporal_filter(maps, kind, sigma=setting[1], radius=setting[2], alpha=setting[3], first=first, n=n)
        assert got.shape == (n, H, W)
        assert np.array_equal(bits(got).reshape(n, -1), bits(hook(vr.NEWEST, setting, store, count, first, n, 0)))
    assert np.array_equal(bits(dataflow.temporal_filter(maps, kind, sigma=setting[1], alpha=setting[3])).reshape(F, -1),
                          bits(_want(F, H * W, vr.NEWEST, setting)))


# ---- the session ------------------------------------------------------------------------------------------------------------
SMALL = dict(batch=3, frames=16, height=32, width=32, base=16, blocks=(1, 1, 1))      # tests/test_gpu_video.py's
F20 = 20
SETTINGS = {"gauss": ("gauss", 1.5, 0, 0.0), "ema": ("ema", 0.0, 0, 0.75)}


def _session(structure="unet", **over):
    from sap3d_tensorflow_amd import P3DSession
    cfg = dict(SMALL)
    cfg.update(over)
    return P3DSession(structure, seed=2, **cfg)


def _frames(F, H, W, seed=0):
    return np.random.default_rng(seed).normal(0.0, 0.5, (F, H, W, 3)).astype(np.float32)


def _resident(sess, frames, mode, starts, batch=3):
    sess.open_video(len(frames), mode)
    sess.video_put(0, frames)
    for i in range(0, len(starts), batch):
        sess.video_predict(starts[i:i + batch])


def _ref(kind, maps, first=0, n=None):
    """temporal_ref on finalised maps [F, H, W] (what the read-out returns with the stage off), every count 1."""
    name, sigma, radius, alpha = SETTINGS[kind]
    cfg = tr.parse(tr.KINDS[name], sigma, radius, alpha)
    F = len(maps)
    return tr.filter_maps(cfg, vr.NEWEST, maps.reshape(F, -1), [1] * F, first, n).reshape((-1,) + maps.shape[1:])


@pytest.mark.parametrize("mode,stride", [("mean", 4), ("newest", 1)])
def test_video_maps_are_the_replay_of_the_unfiltered_maps(mode, stride):
    sess = _session()
    assert sess.get_video_temporal() is None
    _resident(sess, _frames(F20, 32, 32, seed=stride), mode, vr.window_starts(F20, T, stride))
    off, counts = sess.video_maps(0, F20, with_counts=True)
    if mode == "mean":
        assert max(counts) > 1
    for kind in ("gauss", "ema"):
        sess.set_video_temporal(*SETTINGS[kind])
        assert sess.get_video_temporal()["kind"] == kind
        on, counts_on = sess.video_maps(0, F20, with_counts=True)
        assert np.array_equal(counts_on, counts)
        assert np.array_equal(bits(on), bits(_ref(kind, off)))
        assert not np.array_equal(bits(on), bits(off))
        assert np.array_equal(bits(sess.video_maps(3, 5)), bits(on[3:8]))
        assert sess.video_temporal_last_ms() > 0.0
    sess.set_video_temporal("off")
    assert sess.get_video_temporal() is None
    assert np.array_equal(bits(sess.video_maps(0, F20)), bits(off))       # off again: the earlier bits
    sess.close_video()
    sess.close()


def test_more_windows_can_follow_a_filtered_read():
    sess = _session()
    frames = _frames(F20, 32, 32, seed=11)
    _resident(sess, frames, "mean", [0, 2, 4])
    want = sess.video_maps(0, F20)                                        # the stage off, no read in between
    sess.set_video_temporal(*SETTINGS["gauss"])
    _resident(sess, frames, "mean", [0])
    part = sess.video_maps(0, 5)                                          # r = 6: needs frames 0 .. 10 of the 16 predicted
    sess.video_predict([2, 4])
    on = sess.video_maps(0, F20)
    assert np.array_equal(bits(on), bits(_ref("gauss", want)))            # the sums were not rewritten by the filtered read
    assert not np.array_equal(bits(part), bits(on[:5]))                   # (frames 2 .. 10 have more contributions now)
    sess.set_video_temporal(None)
    assert np.array_equal(bits(sess.video_maps(0, F20)), bits(want))
    sess.close_video()
    sess.close()


@pytest.mark.parametrize("post", [False, True], ids=["plain", "postprocess"])
def test_maps_u8_runs_its_chain_on_the_filtered_maps(post):
    from sap3d_tensorflow_amd import dataflow
    sess = _session()
    size = (40, 36)
    if post:
        sess.set_postprocess(2.0, 0, "range")
    _resident(sess, _frames(F20, 32, 32, seed=4), "mean", vr.window_starts(F20, T, 4))
    plain = sess.video_maps_u8(0, F20, size=size)
    for kind in ("gauss", "ema"):
        sess.set_video_temporal(*SETTINGS[kind])
        filtered = sess.video_maps(0, F20)
        want = dataflow.postprocess_maps(filtered, size, 2.0, 0, "range", scale=255.) if post else dataflow.resize_linear_u8(filtered, size)
        got = sess.video_maps_u8(0, F20, size=size)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        assert np.array_equal(sess.video_maps_u8(17, 3, size=size), want[17:])
        assert not np.array_equal(got, plain)
    sess.set_video_temporal("off")
    assert np.array_equal(sess.video_maps_u8(0, F20, size=size), plain)
    sess.close_video()
    sess.close()


def test_a_filtered_read_out_in_between_does_not_change_the_train_step():
    from sap3d_tensorflow_amd import synthetic
    shape = (3, 16, 32, 32)
    x, y = synthetic.synthetic_clip(0, shape + (3,)), synthetic.synthetic_target(1, shape)
    runs = []
    for with_video in (False, True):
        sess = _session()
        l0 = sess.train_step(x, y, dropout=0.5, seed=7)
        if with_video:
            sess.set_video_temporal(*SETTINGS["gauss"])
            _resident(sess, _frames(F20, 32, 32), "mean", [0, 1, 4])
            sess.video_maps(0, F20)
            sess.video_maps_u8(0, F20, size=(8, 8))
            sess.close_video()
        losses = (l0, sess.train_step(x, y, dropout=0.5, seed=8), sess.train_step(x, y, dropout=0.5, seed=9))
        weights = np.concatenate([bits(sess.get_param(name)).reshape(-1) for name, _, _ in sess.variables()])
        runs.append((np.float32(losses).view(np.uint32), weights))
        sess.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def test_session_refusals_change_nothing():
    from sap3d_tensorflow_amd import P3dError
    sess = _session()
    for args in (("gauss", 0.0), ("gauss", -1.0), ("gauss", float("nan")), ("gauss", 1.0, 25), ("gauss", 7.0), ("gauss", 0.0, 3),
                 ("ema", 0.0, 0, 1.0), ("ema", 0.0, 0, float("inf"))):
        with pytest.raises(P3dError, match="video_temporal"):
            sess.set_video_temporal(*args)
        assert sess.get_video_temporal() is None
    with pytest.raises(ValueError):
        sess.set_video_temporal("median")
    with pytest.raises(P3dError, match="no read-out"):
        sess.video_temporal_last_ms()
    sess.set_video_temporal("gauss", 1.5)                                  # needs no open video
    assert sess.get_video_temporal() == dict(kind="gauss", sigma=1.5, radius=0, alpha=0.0)
    with pytest.raises(P3dError, match="video_temporal"):
        sess.set_video_temporal("ema", alpha=2.0)
    assert sess.get_video_temporal()["kind"] == "gauss"                    # a refused setting leaves the earlier one
    frames = _frames(F20, 32, 32, seed=6)
    sess.open_video(F20, "mean")
    sess.video_put(0, frames)
    sess.video_predict([0, 2])                                             # frames 0 .. 17
    info = sess.video_info()
    sess.set_video_temporal("off")
    maps, counts = sess.video_maps(0, 18, with_counts=True)
    sess.set_video_temporal("gauss", 1.5)                                  # r = 6
    for call in (lambda: sess.video_maps(10, 5), lambda: sess.video_maps_u8(12, 1, size=(4, 4)), lambda: sess.video_maps(0, F20)):
        with pytest.raises(P3dError, match=r"frame 18\b"):
            call()                                                         # a frame no window has predicted yet
    got = sess.video_maps(0, 12)                                           # needs 0 .. 17: a valid read still works
    assert np.array_equal(bits(got), bits(_ref("gauss", maps, 0, 12)))    # (no tap of frames 0 .. 11 reaches the last frame's reflection)
    sess.set_video_temporal("gauss", 9.0, 20)
    with pytest.raises(P3dError, match="F - 1"):
        sess.video_maps(0, 5)                                              # r = 20 > F - 1 = 19
    sess.set_video_temporal("off")
    m2, c2 = sess.video_maps(0, 18, with_counts=True)
    assert sess.video_info() == info and np.array_equal(bits(m2), bits(maps)) and np.array_equal(c2, counts)
    sess.video_predict([4])                                                # and the video still works
    assert sess.video_info()["last_start"] == 4
    sess.close_video()
    sess.close()


# ---- the driver -------------------------------------------------------------------------------------------------------------
def test_driver_temporal_writes_the_bytes_of_the_session_calls(tmp_path, capsys):
    from sap3d_tensorflow_amd import P3DSession
    gp = _gen_pred()
    videos = tmp_path / "videos"
    videos.mkdir()
    video = np.random.default_rng(0).integers(0, 256, (20, 60, 80, 3)).astype(np.uint8)
    np.save(videos / "synth.npy", video)
    common = ["--structure", "unet", "--videos", str(videos), "--batch", "3", "--base", "16", "--blocks", "1,1,1", "--size", "40", "36"]
    gp.main(common + ["--out", str(tmp_path / "png"), "--resident", "--temporal", "gauss", "--temporal-sigma", "1.5", "--write", "png", "--time"])
    out = capsys.readouterr().out
    assert "temporal gauss" in out and "ms on the device" in out
    gp.main(common + ["--out", str(tmp_path / "npy"), "--temporal", "ema", "--temporal-alpha", "0.75"])      # implies --resident
    sess = P3DSession("unet", batch=3, device=0, seed=0, base=16, blocks=(1, 1, 1))
    gp.predict_video_resident(sess, video, 3)
    sess.set_video_temporal("gauss", 1.5)
    by_hand = tmp_path / "by_hand"
    by_hand.mkdir()
    for first in (0, 16):
        for k, m in enumerate(sess.video_maps_u8(first, min(16, 20 - first), size=(40, 36))):
            gp.save_image(str(by_hand / ("frame_%d.png" % (first + k + 1))), m, "png")
    for k in range(1, 21):
        a, b = (tmp_path / "png" / "synth" / ("frame_%d.png" % k)).read_bytes(), (by_hand / ("frame_%d.png" % k)).read_bytes()
        assert len(a) > 0 and a == b, k
    sess.set_video_temporal("ema", alpha=0.75)
    assert np.array_equal(bits(np.load(tmp_path / "npy" / "synth.npy")), bits(sess.video_maps(0, 20)))
    sess.close_video()
    sess.close()
