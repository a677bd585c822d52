"""Resident video inference on the GPU (csrc/video.hip through the C ABI): the gather, scatter and mean launches at op level
against tests/video_ref.py, the session's video path against host-stacked predict_windows calls and against
drivers/gen_pred.py:predict_video, the refusals, the isolation of the train step, and the driver's --resident path.  Every
comparison is bit for bit (uint32 views).

predict_video writes into a [F, 112, 112] array, so the checks against it run sessions of 112 x 112 (base 16, one block per
stage); the MEAN and stride checks, whose reference is the replay, run at 32 x 32."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import video_ref as vr        # noqa: E402

T = 16
_i32p = C.POINTER(C.c_int32)
SPECIALS = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff], np.uint32)


def _gen_pred():
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the hooks ------------------------------------------------------------------------------------------------------------
def gather(store, starts, B, offset):
    from sap3d_tensorflow_amd import _lib
    from sap3d_tensorflow_amd._lib import check, fptr
    F, fe = store.shape
    st = np.ascontiguousarray(starts, np.int32)
    x = np.empty((B, T, fe), np.float32)
    check(_lib.lib().p3d_debug_video_gather(0, fptr(store), F, T, fe, st.ctypes.data_as(_lib._ip), len(st), B, offset, fptr(x)))
    return x


@pytest.mark.parametrize("frame_elems", [105, 3072])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_gather_copies_the_bits_and_pads_with_the_last_window(frame_elems, offset):
    F, B = 40, 4
    rng = np.random.default_rng(frame_elems + offset)
    store = rng.standard_normal((F, frame_elems)).astype(np.float32)
    su = store.view(np.uint32)
    su.reshape(-1)[rng.choice(su.size, 64, replace=False)] = np.resize(SPECIALS, 64)      # NaNs with payloads, +-inf, -0, denormals
    for starts in ([0, 1, 2, 3], [3, 8, 24], [F - T]):
        got = gather(store, starts, B, offset)
        padded = starts + [starts[-1]] * (B - len(starts))
        want = np.stack([su[s:s + T] for s in padded])
        assert np.array_equal(got.view(np.uint32), want), (starts, offset)


def test_gather_refuses_a_window_outside_the_store():
    from sap3d_tensorflow_amd import P3dError
    store = np.zeros((20, 8), np.float32)
    for starts in ([5], [-1]):
        with pytest.raises(P3dError):
            gather(store, starts, 2, 0)


def scatter(mode, pred, starts, F, last_start, store, count, offset):
    """pred [B, T, hw, ld]; store and count are updated in place."""
    from sap3d_tensorflow_amd import _lib
    from sap3d_tensorflow_amd._lib import check, fptr
    B, _, hw, ld = pred.shape
    st = np.ascontiguousarray(starts, np.int32)
    check(_lib.lib().p3d_debug_video_scatter(0, mode, fptr(pred), B, T, hw, ld, st.ctypes.data_as(_lib._ip), len(st), F, last_start,
                                             fptr(store), count.ctypes.data_as(_i32p), offset))


CALLS = {"contiguous": [[0, 1, 2], [3, 4, 5, 6]], "stride5": [[0, 5, 10, 15], [20, 25]], "stride20": [[0, 20], [40]]}


@pytest.mark.parametrize("mode", [vr.NEWEST, vr.MEAN], ids=["newest", "mean"])
@pytest.mark.parametrize("hw,ld", [(35, 1), (35, 4), (1024, 1), (1024, 4)])
@pytest.mark.parametrize("calls", sorted(CALLS))
def test_scatter_matches_the_replay_over_two_calls(mode, hw, ld, calls):
    F, B = 60, 4
    for offset in range(4):
        rng = np.random.default_rng(hw * 8 + ld + offset)
        store = rng.standard_normal((F, hw)).astype(np.float32)           # what an earlier video left: frames nothing reaches keep it
        count = np.zeros(F, np.int32)
        want_store, want_count, last = store.copy(), [0] * F, -1
        for starts in CALLS[calls]:
            pred = np.full((B, T, hw, ld), np.nan, np.float32)            # the other columns hold NaN and must not be read
            pred[..., 0] = rng.standard_normal((B, T, hw)).astype(np.float32)
            pred[0, :, :3, 0] = -0.0                                      # a first contribution of -0 stays -0
            pred[len(starts):, ..., 0] += 100.0                           # padding clips: contribute nothing
            scatter(mode, pred, starts, F, last, store, count, offset)
            vr.scatter(mode, want_store, want_count, np.ascontiguousarray(pred[..., 0]), starts)
            last = starts[-1]
            assert count.tolist() == want_count, (calls, offset)
            assert np.array_equal(bits(store), bits(want_store)), (calls, offset)
        assert not np.isnan(store).any()
        untouched = [f for f in range(F) if want_count[f] == 0]
        if calls == "stride20":
            assert 16 in untouched and 39 in untouched
        first_frame = CALLS[calls][0][0]
        assert np.signbit(store[first_frame, :3]).all() and (store[first_frame, :3] == 0).all()
        if mode == vr.MEAN and calls != "stride20":
            assert max(want_count) > 1


def test_scatter_validates_as_predict_does():
    from sap3d_tensorflow_amd import P3dError
    pred = np.zeros((2, T, 8, 1), np.float32)
    store, count = np.zeros((20, 8), np.float32), np.zeros(20, np.int32)
    for starts, last in (([1, 1], -1), ([0, 5], -1), ([2], 2), ([0, 1, 2], -1)):
        with pytest.raises(P3dError, match="video"):
            scatter(vr.MEAN, pred, starts, 20, last, store, count, 0)
    assert not store.any() and not count.any()


@pytest.mark.parametrize("hw", [35, 1024])
def test_mean_divides_once_and_copies_a_count_of_one(hw):
    from sap3d_tensorflow_amd import _lib
    from sap3d_tensorflow_amd._lib import check, fptr
    n = 16
    rng = np.random.default_rng(hw)
    s = (rng.standard_normal((n, hw)) * 3.0).astype(np.float32)
    s.view(np.uint32)[0, :8] = SPECIALS                                   # count 1: the sum's bits, whatever they are
    s[1, :2] = (-0.0, 1e-45)
    count = np.arange(1, n + 1, dtype=np.int32)
    with np.errstate(all="ignore"):
        want = np.stack([s[i] if count[i] == 1 else s[i] / np.float32(count[i]) for i in range(n)])
    for offset in range(4):
        out = np.empty_like(s)
        check(_lib.lib().p3d_debug_video_mean(0, fptr(s), count.ctypes.data_as(_i32p), n, hw, offset, fptr(out)))
        assert np.array_equal(bits(out), bits(want)), offset
    assert np.array_equal(bits(vr.read_out(vr.MEAN, s, count.tolist())), bits(want))


# ---- the session ----------------------------------------------------------------------------------------------------------
SMALL = dict(batch=3, frames=16, height=32, width=32, base=16, blocks=(1, 1, 1))
F20 = 20


def _session(structure="unet", **over):
    from sap3d_tensorflow_amd import P3DSession
    cfg = dict(SMALL)
    cfg.update(over)
    return P3DSession(structure, seed=2, **cfg)


def _frames(F, H, W, seed=0):
    return np.random.default_rng(seed).normal(0.0, 0.5, (F, H, W, 3)).astype(np.float32)


def _host_predict(sess, frames):
    def predict(starts):
        return sess.predict_windows(np.stack([frames[s:s + T] for s in starts]))[..., 0]
    return predict


def _resident(sess, frames, mode, starts, batch=3):
    sess.open_video(len(frames), mode)
    sess.video_put(0, frames)
    for i in range(0, len(starts), batch):
        sess.video_predict(starts[i:i + batch])


@pytest.mark.parametrize("structure", ["unet", "gn_p3d", "unet++ds"])
def test_newest_at_stride_1_equals_the_drivers_predict_video(structure):
    gp = _gen_pred()
    sess = _session(structure, height=112, width=112)
    frames = _frames(F20, 112, 112)
    want = gp.predict_video(sess, frames, 3)
    _resident(sess, frames, "newest", gp.window_starts(F20, 1))            # five windows: a full batch and a short one
    got, counts = sess.video_maps(0, F20, with_counts=True)
    assert counts.tolist() == [1] * F20
    assert np.array_equal(bits(got), bits(want))
    assert sess.video_info() == dict(frames=F20, mode="newest", last_start=4)
    sess.close_video()
    sess.close()


@pytest.mark.parametrize("mode,stride", [("mean", 1), ("mean", 4), ("newest", 4), ("mean", 3)])
def test_modes_and_strides_equal_the_replay_of_host_stacked_windows(mode, stride):
    sess = _session()
    frames = _frames(F20, 32, 32, seed=stride)
    starts = vr.window_starts(F20, T, stride)
    m = vr.MEAN if mode == "mean" else vr.NEWEST
    store, count = vr.run_video(m, F20, T, 3, starts, _host_predict(sess, frames))
    want = vr.read_out(m, store, count).reshape(F20, 32, 32)
    _resident(sess, frames, mode, starts)
    got, counts = sess.video_maps(0, F20, with_counts=True)
    assert counts.tolist() == count
    assert np.array_equal(bits(got), bits(want))
    again = sess.video_maps(3, 5)                                          # the read-out does not rewrite the sums
    assert np.array_equal(bits(again), bits(want[3:8]))
    if mode == "mean" and stride == 1:
        assert max(count) == 5 and count[0] == 1
    sess.close_video()
    sess.close()


def test_prediction_of_a_batch_is_predict_windows_bit_for_bit():
    sess = _session()
    frames = _frames(F20, 32, 32, seed=9)
    want = sess.predict_windows(np.stack([frames[0:16], frames[2:18], frames[2:18]]))
    sess.open_video(F20, "newest")
    sess.video_put(4, frames[4:])                                          # any order, several calls
    sess.video_put(0, frames[:4])
    sess.video_predict([0, 2])
    assert np.array_equal(bits(sess.video_maps(0, 16)), bits(want[0, ..., 0]))
    assert np.array_equal(bits(sess.video_maps(16, 2)), bits(want[1, 14:, :, :, 0]))
    u8 = sess.pred_maps_u8([15, 15, T], size=(8, 8))                       # pred_maps_u8 keeps working on the batch
    assert u8.shape == (2, 8, 8)
    sess.close_video()
    sess.close()


def test_put_u8_stores_what_mapf_frames_returns():
    from sap3d_tensorflow_amd import dataflow
    sess = _session()
    bgr = np.random.default_rng(1).integers(0, 256, (F20, 40, 56, 3)).astype(np.uint8)
    norm = dataflow.mapf_frames(bgr, (32, 32))
    _resident(sess, norm, "mean", [0, 2, 4])
    want = sess.video_maps(0, F20)
    sess.open_video(F20, "mean")                                           # opening again replaces the video
    sess.video_put_u8(0, bgr[:7])
    sess.video_put_u8(7, bgr[7:])
    sess.video_predict([0, 2, 4])
    assert np.array_equal(bits(sess.video_maps(0, F20)), bits(want))
    sess.close_video()
    sess.close()


@pytest.mark.parametrize("post", [False, True], ids=["plain", "postprocess"])
def test_maps_u8_equals_pred_maps_u8_on_the_same_frames(post):
    sess = _session()
    if post:
        sess.set_postprocess(2.0, 0, "range")
    frames = _frames(F20, 32, 32, seed=4)
    size = (40, 36)
    want = np.empty((F20,) + size, np.uint8)
    sess.predict_windows(np.stack([frames[0:16], frames[1:17], frames[2:18]]))
    want[:18] = sess.pred_maps_u8([0, 15, 15], size=size)
    sess.predict_windows(np.stack([frames[3:19], frames[4:20], frames[4:20]]))
    want[18:] = sess.pred_maps_u8([15, 15, T], size=size)
    _resident(sess, frames, "newest", [0, 1, 2, 3, 4])
    got = sess.video_maps_u8(0, F20, size=size)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(sess.video_maps_u8(17, 3, size=size), want[17:])
    assert set(sess.last_maps_ms) == {"device", "d2h"} and sess.last_maps_ms["device"] > 0.0
    sess.close_video()
    # MEAN is finalised first: with one window per frame the mean is the map
    _resident(sess, frames, "mean", [0])
    sess.predict_windows(np.stack([frames[0:16]] * 3))
    assert np.array_equal(sess.video_maps_u8(0, 16, size=size), sess.pred_maps_u8([0, T, T], size=size))
    sess.close_video()
    sess.close()


def test_refusals_change_nothing():
    from sap3d_tensorflow_amd import P3dError
    sess = _session()
    frames = _frames(F20, 32, 32, seed=6)
    for call in (lambda: sess.video_predict([0]), lambda: sess.video_info(), lambda: sess.video_maps(0, 1),
                 lambda: sess.video_put(0, frames[:1])):
        with pytest.raises(P3dError, match="no video is open"):
            call()
    for frames_, mode in ((15, "newest"), (-1, "mean")):
        with pytest.raises(P3dError, match="video_open"):
            sess.open_video(frames_, mode)
    with pytest.raises(ValueError):
        sess.open_video(F20, "median")
    sess.open_video(F20, "mean")
    sess.video_put(0, frames[:18])
    with pytest.raises(P3dError, match="frame 18"):
        sess.video_predict([0, 3])                                         # a window over a frame never put
    with pytest.raises(P3dError, match="outside"):
        sess.video_put(19, frames[:2])
    assert sess.video_info()["last_start"] == -1
    sess.video_predict([0, 2])
    info, (maps, counts) = sess.video_info(), sess.video_maps(0, 18, with_counts=True)

    def unchanged():
        m, c = sess.video_maps(0, 18, with_counts=True)
        return sess.video_info() == info and np.array_equal(bits(m), bits(maps)) and np.array_equal(c, counts)
    with pytest.raises(P3dError, match="frame 18"):
        sess.video_maps(10, 10)                                            # count 0
    with pytest.raises(P3dError, match="frame 18"):
        sess.video_maps_u8(18, 1, size=(4, 4))
    assert unchanged()
    sess.video_put(18, frames[18:])
    for starts in ([2], [1, 3], [3, 3], [4, 3], [5], [3, 4, 4, 4]):          # repeated / not ascending / past F - T / more than batch
        with pytest.raises(P3dError, match="video"):
            sess.video_predict(starts)
        assert unchanged(), starts
    sess.video_predict([3, 4])                                             # and the video still works
    assert sess.video_info()["last_start"] == 4
    sess.close_video()
    with pytest.raises(P3dError, match="no video is open"):
        sess.video_maps(0, 1)
    sess.close()


def test_a_video_in_between_does_not_change_the_train_step():
    from sap3d_tensorflow_amd import synthetic
    shape = (3, 16, 32, 32)
    x, y = synthetic.synthetic_clip(0, shape + (3,)), synthetic.synthetic_target(1, shape)
    losses = []
    for with_video in (False, True):
        sess = _session()
        l0 = sess.train_step(x, y, dropout=0.5, seed=7)
        if with_video:
            _resident(sess, _frames(F20, 32, 32), "mean", [0, 1, 4])
            sess.video_maps(0, F20)
            sess.close_video()
        losses.append((l0, sess.train_step(x, y, dropout=0.5, seed=8), sess.train_step(x, y, dropout=0.5, seed=9)))
        sess.close()
    assert np.array_equal(np.float32(losses[0]).view(np.uint32), np.float32(losses[1]).view(np.uint32)), losses


def test_under_ema_swap_the_video_scores_the_averages():
    from sap3d_tensorflow_amd import synthetic
    shape = (3, 16, 32, 32)
    sess = _session()
    sess.set_ema(0.5)
    sess.train_step(synthetic.synthetic_clip(0, shape + (3,)), synthetic.synthetic_target(1, shape), dropout=0.0, seed=1)
    frames = _frames(F20, 32, 32, seed=2)
    with sess.averaged():
        want = sess.predict_windows(np.stack([frames[0:16]] * 3))[0, ..., 0]
        _resident(sess, frames, "newest", [0])
        got = sess.video_maps(0, 16)
        sess.close_video()
    assert np.array_equal(bits(got), bits(want))
    sess.close()


# ---- the driver -----------------------------------------------------------------------------------------------------------
def test_driver_resident_writes_the_default_paths_bytes(tmp_path, capsys):
    gp = _gen_pred()
    videos = tmp_path / "videos"
    videos.mkdir()
    np.save(videos / "synth.npy", np.random.default_rng(0).integers(0, 256, (20, 60, 80, 3)).astype(np.uint8))
    common = ["--structure", "unet", "--videos", str(videos), "--batch", "3", "--base", "16", "--blocks", "1,1,1"]
    gp.main(common + ["--out", str(tmp_path / "host")])
    gp.main(common + ["--out", str(tmp_path / "resident"), "--resident"])
    a, b = (tmp_path / "host" / "synth.npy").read_bytes(), (tmp_path / "resident" / "synth.npy").read_bytes()
    assert len(a) > 20 * 112 * 112 * 4 and a == b
    capsys.readouterr()
    gp.main(common + ["--out", str(tmp_path / "mean"), "--stride", "4", "--overlap", "mean", "--time"])
    sal = np.load(tmp_path / "mean" / "synth.npy")
    assert sal.shape == (20, 112, 112) and sal.dtype == np.float32 and np.isfinite(sal).all()
    out = capsys.readouterr().out
    assert "wall" in out and "stride 4" in out and "overlap mean" in out and "1 forward passes" in out
