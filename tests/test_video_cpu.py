"""No-GPU checks of resident video inference: the symbols, the host-side plan of p3d_video_predict (p3d_debug_video_plan makes no
HIP call) against tests/video_ref.py, and the replay's NEWEST rule against the driver's host loop."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import video_ref        # noqa: E402

T = 16
SYMBOLS = ["p3d_video_open", "p3d_video_close", "p3d_video_info", "p3d_video_put_frames", "p3d_video_put_frames_u8",
           "p3d_video_predict", "p3d_video_get_maps", "p3d_video_maps_u8", "p3d_video_last_ms", "p3d_debug_video_gather",
           "p3d_debug_video_scatter", "p3d_debug_video_mean", "p3d_debug_video_plan"]
_i32p = C.POINTER(C.c_int32)


def test_video_symbols_are_exported_and_bound():
    from sap3d_tensorflow_amd import _lib
    lib = _lib.lib()
    for n in SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    hdr = open(os.path.join(ROOT, "include", "p3d_hip.h")).read()
    for n in SYMBOLS:
        assert n + "(" in hdr, n
    from sap3d_tensorflow_amd import P3DSession
    for m in ("open_video", "close_video", "video_info", "video_put", "video_put_u8", "video_predict", "video_maps", "video_maps_u8"):
        assert callable(getattr(P3DSession, m)), m


def plan(mode, F, B, last_start, count, starts, n_windows=None):
    """(rc, count_out) of p3d_debug_video_plan; count_out starts as a sentinel."""
    from sap3d_tensorflow_amd import _lib
    cin = np.ascontiguousarray(count, np.int32)
    st = np.ascontiguousarray(starts, np.int32)
    out = np.full(F, -7, np.int32)
    rc = _lib.lib().p3d_debug_video_plan(mode, F, T, B, last_start, cin.ctypes.data_as(_i32p), st.ctypes.data_as(_lib._ip),
                                         len(st) if n_windows is None else n_windows, out.ctypes.data_as(_i32p))
    return rc, out


@pytest.mark.parametrize("mode", [video_ref.NEWEST, video_ref.MEAN])
@pytest.mark.parametrize("starts", [[0, 1, 2, 3], [0, 5, 10, 15], [0, 20, 40], [3]], ids=["contiguous", "stride5", "stride20", "one"])
def test_plan_counts_match_the_replay(mode, starts):
    F = 60
    rc, out = plan(mode, F, 4, -1, [0] * F, starts)
    assert rc == 0
    want = video_ref.plan_counts(mode, F, T, 4, -1, [0] * F, starts)
    assert out.tolist() == want
    if starts == [0, 20, 40]:
        assert out[16:20].tolist() == [0] * 4              # a stride above T leaves frames at count 0
    if mode == video_ref.MEAN and starts == [0, 5, 10, 15]:
        assert out[15] == 4 and out[0] == 1


@pytest.mark.parametrize("mode", [video_ref.NEWEST, video_ref.MEAN])
def test_plan_carries_last_start_and_counts_over_two_calls(mode):
    F = 40
    rc, c1 = plan(mode, F, 3, -1, [0] * F, [0, 4, 8])
    assert rc == 0
    rc, c2 = plan(mode, F, 3, 8, c1, [12, 16])
    assert rc == 0
    w1 = video_ref.plan_counts(mode, F, T, 3, -1, [0] * F, [0, 4, 8])
    w2 = video_ref.plan_counts(mode, F, T, 3, 8, w1, [12, 16])
    assert c1.tolist() == w1 and c2.tolist() == w2
    assert max(c2) == (4 if mode == video_ref.MEAN else 1)


@pytest.mark.parametrize("case", ["not_ascending", "repeated", "le_last", "past_end", "negative", "zero_windows", "too_many", "bad_mode"])
def test_plan_refusals_leave_the_output_untouched(case):
    from sap3d_tensorflow_amd import _lib
    F, B = 40, 3
    mode, last, starts, nw = video_ref.MEAN, 4, [5, 9], None
    if case == "not_ascending":
        starts = [9, 5]
    elif case == "repeated":
        starts = [5, 5]
    elif case == "le_last":
        starts = [4, 9]
    elif case == "past_end":
        starts = [5, F - T + 1]
    elif case == "negative":
        last, starts = -1, [-1]
    elif case == "zero_windows":
        nw = 0
    elif case == "too_many":
        starts = [5, 6, 7, 8]
    elif case == "bad_mode":
        mode = 2
    rc, out = plan(mode, F, B, last, [0] * F, starts, nw)
    assert rc == -1
    assert out.tolist() == [-7] * F
    assert "video" in _lib.lib().p3d_last_error().decode()
    with pytest.raises(video_ref.Refused):
        video_ref.validate(mode, F, T, B, last, starts if nw is None else starts[:nw])
    rc, out = plan(video_ref.MEAN, F, B, 4, [0] * F, [5, 9])      # the neighbouring accepted call
    assert rc == 0 and out[9] == 2


def test_refusal_names_the_offending_window():
    from sap3d_tensorflow_amd import _lib
    rc, _ = plan(video_ref.NEWEST, 40, 3, -1, [0] * 40, [0, 7, 7])
    assert rc == -1
    assert "window 2" in _lib.lib().p3d_last_error().decode()


def _gen_pred():
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


class StubSession:
    """predict_windows as a deterministic numpy function of the clips: every map depends on its frame AND on its window."""

    def predict_windows(self, clips):
        clips = np.asarray(clips, np.float32)
        m = clips.mean(axis=4, keepdims=True)                                   # [B, T, H, W, 1]
        w = clips.reshape(len(clips), -1)[:, :7].sum(axis=1).astype(np.float32)  # a per-window term
        return (m * np.float32(0.5) + w[:, None, None, None, None] * np.float32(0.125)).astype(np.float32)


def test_newest_rule_at_stride_1_is_the_drivers_host_loop():
    gp = _gen_pred()
    F, batch = 20, 3
    rng = np.random.default_rng(5)
    frames = rng.standard_normal((F, 112, 112, 3)).astype(np.float32)
    sess = StubSession()
    want = gp.predict_video(sess, frames, batch)

    def predict(starts):
        return sess.predict_windows(np.stack([frames[s:s + T] for s in starts]))[..., 0]
    maps, count = video_ref.run_video(video_ref.NEWEST, F, T, batch, video_ref.window_starts(F, T, 1), predict)
    assert count == [1] * F
    got = video_ref.read_out(video_ref.NEWEST, maps, count).reshape(F, 112, 112)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_mean_replay_sums_in_window_order_and_keeps_minus_zero():
    F, batch = 18, 2
    pred = {0: np.full((T, 3), -0.0, np.float32), 1: np.full((T, 3), 0.1, np.float32), 2: np.full((T, 3), 0.7, np.float32)}

    def predict(starts):
        return np.stack([pred[s] for s in starts])
    maps, count = video_ref.run_video(video_ref.MEAN, F, T, batch, [0, 1, 2], predict)
    assert count[0] == 1 and count[2] == 3 and count[17] == 1
    assert np.signbit(maps[0]).all()                                           # the first contribution's bits, not 0 + (-0)
    assert np.array_equal(maps[2], (np.float32(-0.0) + np.float32(0.1)) + np.full(3, 0.7, np.float32))
    out = video_ref.read_out(video_ref.MEAN, maps, count)
    assert np.array_equal(out[2], maps[2] / np.float32(3)) and np.array_equal(out[0].view(np.uint32), maps[0].view(np.uint32))


def test_window_starts_cover_every_frame():
    assert video_ref.window_starts(20, T, 1) == [0, 1, 2, 3, 4]
    assert video_ref.window_starts(20, T, 4) == [0, 4]
    assert video_ref.window_starts(21, T, 4) == [0, 4, 5]
    assert video_ref.window_starts(40, T, 16) == [0, 16, 24]
    gp = _gen_pred()
    for F in (16, 20, 21, 40):
        for stride in (1, 4, 16, 20):
            assert gp.window_starts(F, stride) == video_ref.window_starts(F, T, stride)
