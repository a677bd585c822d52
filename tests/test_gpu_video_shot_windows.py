"""Shot-aware windows on the GPU (p3d_video_predict_shots; csrc/video.hip's video_gather_slots_kernel through the C ABI): the slot
gather and the live-slot scatter at op level against tests/shot_windows_ref.py, the session's path against host-gathered reflected
windows, a table of one shot against p3d_video_predict, the point of it all -- no frame of another shot reaches a map --, the
refusals, the isolation of the train step, and the driver's --shot-windows.  Every comparison is bit for bit (uint32 views)."""
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
import shot_windows_ref as sw        # noqa: E402
import shots_ref                     # noqa: E402
import video_ref as vr               # noqa: E402

T = 16
F41, TABLE = sw.EXAMPLE_F, sw.EXAMPLE_TABLE      # shots of 20, 5, 1, 2 and 13 frames
_i32p = C.POINTER(C.c_int32)
SPECIALS = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff], np.uint32)
MODES = {"newest": vr.NEWEST, "mean": vr.MEAN}


def _gen_pred():
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the hooks ------------------------------------------------------------------------------------------------------------
def gather_slots(store, table, starts, B, offset):
    from sap3d_tensorflow_amd import _lib
    from sap3d_tensorflow_amd._lib import check, fptr
    F, fe = store.shape
    tb, st = np.ascontiguousarray(table, np.int32), np.ascontiguousarray(starts, np.int32)
    x = np.empty((B, T, fe), np.float32)
    check(_lib.lib().p3d_debug_video_gather_slots(0, fptr(store), F, T, fe, tb.ctypes.data_as(_i32p), len(tb), st.ctypes.data_as(_lib._ip),
                                                  len(st), B, offset, fptr(x)))
    return x


@pytest.mark.parametrize("frame_elems", [105, 3072])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_gather_copies_the_bits_of_every_slots_frame_and_pads_with_the_last_row(frame_elems, offset):
    B = 4
    rng = np.random.default_rng(frame_elems + offset)
    store = rng.standard_normal((F41, frame_elems)).astype(np.float32)
    su = store.view(np.uint32)
    su.reshape(-1)[rng.choice(su.size, 64, replace=False)] = np.resize(SPECIALS, 64)      # NaNs with payloads, +-inf, -0, denormals
    for starts in ([0, 4, 20], [25, 26, 28], [20]):
        got = gather_slots(store, TABLE, starts, B, offset)
        g, _ = sw.slots(TABLE, F41, T, B, starts)
        assert g[len(starts):].tolist() == [g[len(starts) - 1].tolist()] * (B - len(starts))
        assert np.array_equal(got.view(np.uint32), su[g]), (starts, offset)
    assert sw.slots(TABLE, F41, T, B, [20])[0][0].tolist() == [20, 21, 22, 23, 24, 23, 22, 21, 20, 21, 22, 23, 24, 23, 22, 21]


def test_gather_refuses_a_start_inside_a_short_shot_and_a_table_past_the_store():
    from sap3d_tensorflow_amd import P3dError
    store = np.zeros((F41, 8), np.float32)
    for table, starts in ((TABLE, [21]), (TABLE, [5]), (TABLE, [41]), ([0, 20, 41], [0]), ([0, 20, 60], [20])):
        with pytest.raises(P3dError, match="video"):
            gather_slots(store, table, starts, 2, 0)


def scatter_shots(mode, pred, table, starts, F, last_start, store, count, offset):
    """pred [B, T, hw, ld]; store and count are updated in place."""
    from sap3d_tensorflow_amd import _lib
    from sap3d_tensorflow_amd._lib import check, fptr
    B, _, hw, ld = pred.shape
    tb, st = np.ascontiguousarray(table, np.int32), np.ascontiguousarray(starts, np.int32)
    check(_lib.lib().p3d_debug_video_scatter_shots(0, mode, fptr(pred), B, T, hw, ld, tb.ctypes.data_as(_i32p), len(tb),
                                                   st.ctypes.data_as(_lib._ip), len(st), F, last_start, fptr(store),
                                                   count.ctypes.data_as(_i32p), offset))


# the driver's law at stride 4 in two calls; and windows that leave frames 16 .. 19, 26 and 27 to what the store held
CALLS = {"stride4": [[0, 4, 20], [25, 26, 28]], "sparse": [[0, 20, 25], [28]]}


@pytest.mark.parametrize("mode", [vr.NEWEST, vr.MEAN], ids=["newest", "mean"])
@pytest.mark.parametrize("hw,ld", [(35, 1), (35, 4), (1024, 1), (1024, 4)])
@pytest.mark.parametrize("calls", sorted(CALLS))
def test_scatter_folds_the_live_slots_only_over_two_calls(mode, hw, ld, calls):
    B = 4
    for offset in range(4):
        rng = np.random.default_rng(hw * 8 + ld + offset)
        store = rng.standard_normal((F41, hw)).astype(np.float32)         # what an earlier video left: frames nothing reaches keep it
        before = store.copy()
        count = np.zeros(F41, np.int32)
        want_store, want_count, last = store.copy(), [0] * F41, -1
        for starts in CALLS[calls]:
            _, live = sw.slots(TABLE, F41, T, B, starts)
            pred = np.full((B, T, hw, ld), np.nan, np.float32)            # padding clips, non-live slots and the other columns hold
            for k in range(len(starts)):                                  # NaN: none of them may be read
                pred[k, :live[k], :, 0] = rng.standard_normal((live[k], hw)).astype(np.float32)
            pred[0, 0, :3, 0] = -0.0                                      # a first contribution of -0 stays -0
            scatter_shots(mode, pred, TABLE, starts, F41, last, store, count, offset)
            sw.scatter(mode, want_store, want_count, np.ascontiguousarray(pred[..., 0]), starts, live)
            last = starts[-1]
            assert count.tolist() == want_count, (calls, offset)
            assert np.array_equal(bits(store), bits(want_store)), (calls, offset)
        assert not np.isnan(store).any()
        untouched = [f for f in range(F41) if want_count[f] == 0]
        assert untouched == ([] if calls == "stride4" else [16, 17, 18, 19, 26, 27])
        assert np.array_equal(bits(store[untouched]), bits(before[untouched]))
        assert np.signbit(store[CALLS[calls][0][0], :3]).all()
        if mode == vr.MEAN and calls == "stride4":
            assert want_count[4:16] == [2] * 12 and max(want_count) == 2


def test_scatter_validates_as_predict_shots_does():
    from sap3d_tensorflow_amd import P3dError
    pred = np.zeros((2, T, 8, 1), np.float32)
    store, count = np.zeros((F41, 8), np.float32), np.zeros(F41, np.int32)
    for starts, last in (([21], -1), ([5], -1), ([20, 20], -1), ([4], 4), ([0, 4, 20], -1), ([41], -1)):
        with pytest.raises(P3dError, match="video"):
            scatter_shots(vr.MEAN, pred, TABLE, starts, F41, last, store, count, 0)
    assert not store.any() and not count.any()


# ---- the session ----------------------------------------------------------------------------------------------------------
SMALL = dict(batch=3, frames=16, height=32, width=32, base=16, blocks=(1, 1, 1))


def _session(structure="unet", **over):
    from sap3d_tensorflow_amd import P3DSession
    cfg = dict(SMALL)
    cfg.update(over)
    return P3DSession(structure, seed=2, **cfg)


def _frames(F, H, W, seed=0):
    return np.random.default_rng(seed).normal(0.0, 0.5, (F, H, W, 3)).astype(np.float32)


def _resident_shots(sess, frames, mode, table, starts, batch=3):
    sess.open_video(len(frames), mode)
    sess.video_put(0, frames)
    sess.video_set_shots(table)
    for i in range(0, len(starts), batch):
        sess.video_predict_shots(starts[i:i + batch])


@pytest.mark.parametrize("mode", ["newest", "mean"])
@pytest.mark.parametrize("stride", [1, 4])
def test_modes_and_strides_equal_the_replay_of_host_gathered_reflected_windows(mode, stride):
    sess = _session()
    frames = _frames(F41, 32, 32, seed=stride)
    starts = sw.window_starts(TABLE, F41, stride)

    def predict(g):                                                        # g [batch, T]: the frame of every slot
        return sess.predict_windows(frames[g])[..., 0]
    store, count = sw.run_video(MODES[mode], F41, T, 3, TABLE, starts, predict)
    want = vr.read_out(MODES[mode], store, count).reshape(F41, 32, 32)
    _resident_shots(sess, frames, mode, TABLE, starts)
    got, counts = sess.video_maps(0, F41, with_counts=True)
    assert counts.tolist() == count and min(count) >= 1
    assert np.array_equal(bits(got), bits(want))
    assert sess.video_info() == dict(frames=F41, mode=mode, last_start=28)
    ms = sess.video_last_ms()
    assert ms["gather"] > 0.0 and ms["scatter"] > 0.0
    if mode == "mean" and stride == 1:
        assert max(count) == 5 and count[20:28] == [1] * 8
    sess.close_video()
    sess.close()


def test_a_table_of_one_shot_returns_video_predicts_bits_and_the_calls_mix():
    F = 20
    sess = _session()
    frames = _frames(F, 32, 32, seed=3)
    starts = vr.window_starts(F, T, 3)                                     # 0, 3, 4
    assert starts == sw.window_starts([0], F, 3)
    sess.open_video(F, "mean")
    sess.video_put(0, frames)
    sess.video_predict(starts)
    want, want_counts = sess.video_maps(0, F, with_counts=True)
    _resident_shots(sess, frames, "mean", [0], starts)
    got, counts = sess.video_maps(0, F, with_counts=True)
    assert np.array_equal(counts, want_counts) and np.array_equal(bits(got), bits(want))
    sess.open_video(F, "mean")                                             # mixed: both share the stores and last_start
    sess.video_put(0, frames)
    sess.video_set_shots([0])
    sess.video_predict([0])
    sess.video_predict_shots([3])
    assert sess.video_info()["last_start"] == 3
    sess.video_predict([4])
    got, counts = sess.video_maps(0, F, with_counts=True)
    assert np.array_equal(counts, want_counts) and np.array_equal(bits(got), bits(want))
    sess.close_video()
    sess.close()


@pytest.mark.parametrize("shot", [0, 1], ids=["the_20_frame_shot", "the_5_frame_shot"])
def test_no_frame_of_another_shot_reaches_a_shots_maps(shot):
    """Every window runs in a call of its own, so the batch holds only copies of it; a copy of the video with NaN in every frame
    outside the shot must give the shot's maps bit for bit.  The same experiment through video_predict, whose windows at stride 4
    cross frame 20, must not: that is what the feature is for, and what shows that this test can fail."""
    sess = _session()
    frames = _frames(F41, 32, 32, seed=5)
    lo, hi = shots_ref.shot_of(TABLE, F41, TABLE[shot])
    poisoned = np.full_like(frames, np.nan)
    poisoned[lo:hi + 1] = frames[lo:hi + 1]

    def run(video, aware):
        sess.open_video(F41, "mean")
        sess.video_put(0, video)
        sess.video_set_shots(TABLE)
        for s in (sw.window_starts(TABLE, F41, 4) if aware else vr.window_starts(F41, T, 4)):
            (sess.video_predict_shots if aware else sess.video_predict)([s])
        return sess.video_maps(lo, hi - lo + 1)
    clean, alone = run(frames, True), run(poisoned, True)
    assert np.isfinite(clean).all() and np.isfinite(alone).all()
    assert np.array_equal(bits(alone), bits(clean))
    assert np.isfinite(run(frames, False)).all()
    assert not np.isfinite(run(poisoned, False)).all()
    sess.close_video()
    sess.close()


def test_refusals_change_nothing():
    from sap3d_tensorflow_amd import P3dError
    sess = _session()
    frames = _frames(F41, 32, 32, seed=6)
    with pytest.raises(P3dError, match="no video is open"):
        sess.video_predict_shots([0])
    sess.open_video(F41, "mean")
    sess.video_put(0, frames[:24])
    sess.video_put(25, frames[25:])                                        # all but frame 24
    with pytest.raises(P3dError, match="no shot table"):
        sess.video_predict_shots([0])
    assert sess.video_info()["last_start"] == -1
    sess.video_set_shots(TABLE)
    sess.video_predict_shots([0, 4])
    info, (maps, counts) = sess.video_info(), sess.video_maps(0, 20, with_counts=True)

    def unchanged():
        m, c = sess.video_maps(0, 20, with_counts=True)
        with pytest.raises(P3dError, match="frame 20"):                    # nothing has been folded past the first shot
            sess.video_maps(20, 1)
        return sess.video_info() == info and np.array_equal(bits(m), bits(maps)) and np.array_equal(c, counts)
    with pytest.raises(P3dError, match="frame 24"):
        sess.video_predict_shots([20])                                     # slot 4 reads frame 24, and so do the reflected slots
    assert unchanged()
    sess.video_put(24, frames[24:25])
    for starts, what in (([21], r"\[20, 24\]"), ([5], r"\[0, 19\]"), ([25, 20], "not after"), ([4], "not after"), ([2], "not after"),
                         ([], None), ([20, 25, 26, 28], "n_windows"), ([41], "outside")):
        with pytest.raises(P3dError, match=what):
            sess.video_predict_shots(starts)
        assert unchanged(), starts
    sess.video_set_shots(None)
    with pytest.raises(P3dError, match="no shot table"):
        sess.video_predict_shots([20])
    sess.video_set_shots(TABLE)
    assert unchanged()
    sess.video_predict_shots([20, 25, 26])                                 # and the video still works
    assert sess.video_info()["last_start"] == 26
    assert sess.video_maps(0, 28, with_counts=True)[1].tolist() == [1] * 4 + [2] * 12 + [1] * 12
    sess.close_video()
    sess.close()


def test_shot_windows_in_between_do_not_change_the_train_step():
    from sap3d_tensorflow_amd import synthetic
    shape = (3, 16, 32, 32)
    x, y = synthetic.synthetic_clip(0, shape + (3,)), synthetic.synthetic_target(1, shape)
    losses = []
    for with_video in (False, True):
        sess = _session()
        l0 = sess.train_step(x, y, dropout=0.5, seed=7)
        if with_video:
            _resident_shots(sess, _frames(F41, 32, 32), "mean", TABLE, sw.window_starts(TABLE, F41, 4))
            sess.video_maps(0, F41)
            sess.close_video()
        losses.append((l0, sess.train_step(x, y, dropout=0.5, seed=8), sess.train_step(x, y, dropout=0.5, seed=9)))
        sess.close()
    assert np.array_equal(np.float32(losses[0]).view(np.uint32), np.float32(losses[1]).view(np.uint32)), losses


# ---- the driver -----------------------------------------------------------------------------------------------------------
def test_driver_shot_windows_writes_the_session_paths_maps(tmp_path):
    from sap3d_tensorflow_amd import P3DSession
    gp = _gen_pred()
    videos = tmp_path / "videos"
    videos.mkdir()
    video = shots_ref.fixture((20, 5, 16))
    F = len(video)
    np.save(videos / "synth.npy", video)
    common = ["--structure", "unet", "--videos", str(videos), "--batch", "3", "--base", "16", "--blocks", "1,1,1", "--resident",
              "--stride", "4"]
    with pytest.raises(SystemExit):                                        # refused before anything runs
        gp.main(common + ["--out", str(tmp_path / "refused"), "--shot-windows"])
    assert not (tmp_path / "refused").exists()
    gp.main(common + ["--out", str(tmp_path / "aware"), "--shots", "detect", "--shot-windows", "--time"])
    gp.main(common + ["--out", str(tmp_path / "plain"), "--shots", "detect"])
    table = np.load(tmp_path / "aware" / "synth_shots.npy")
    assert table.tolist() == [0, 20, 25] == np.load(tmp_path / "plain" / "synth_shots.npy").tolist()
    got, plain = np.load(tmp_path / "aware" / "synth.npy"), np.load(tmp_path / "plain" / "synth.npy")
    sess = P3DSession("unet", batch=3, device=0, seed=0, base=16, blocks=(1, 1, 1))
    sess.open_video(F, "newest")
    sess.video_put_u8(0, video[..., ::-1])
    sess.video_set_shots(table)
    starts = sw.window_starts(table, F, 4)
    assert starts == [0, 4, 20, 25]
    for i in range(0, len(starts), 3):
        sess.video_predict_shots(starts[i:i + 3])
    want = sess.video_maps(0, F)
    sess.close_video()
    sess.close()
    assert got.shape == (F, 112, 112) and np.array_equal(bits(got), bits(want))
    assert any(not np.array_equal(bits(got[f]), bits(plain[f])) for f in range(16, 25))
