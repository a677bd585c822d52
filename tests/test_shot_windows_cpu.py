"""No-GPU checks of shot-aware windows (include/p3d_hip.h, "Shot-aware windows"): the host-side plan of p3d_video_predict_shots
(p3d_debug_video_plan_shots makes no HIP call) against tests/shot_windows_ref.py over random videos, tables and strides, the refusals,
the header's example to the letter, the driver's window law, and a table of one shot against p3d_debug_video_plan."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import shot_windows_ref as sw        # noqa: E402
import shots_ref                     # noqa: E402
import video_ref                     # noqa: E402

T = 16
STRIDES = (1, 3, 4, 16)
SYMBOLS = ["p3d_video_predict_shots", "p3d_debug_video_gather_slots", "p3d_debug_video_scatter_shots", "p3d_debug_video_plan_shots"]
_i32p = C.POINTER(C.c_int32)


def test_symbols_are_exported_and_bound():
    from sap3d_tensorflow_amd import P3DSession, _lib, dataflow
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "p3d_hip.h")).read()
    for n in SYMBOLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES and n + "(" in hdr, n
    assert callable(P3DSession.video_predict_shots) and callable(dataflow.shot_window_starts)


def plan(mode, F, B, last_start, count, table, starts, n_windows=None):
    """(rc, count_out [F], slots_out [B, T], live_out [B]) of p3d_debug_video_plan_shots; the outputs start as sentinels."""
    from sap3d_tensorflow_amd import _lib
    cin, tb, st = (np.ascontiguousarray(a, np.int32) for a in (count, table, starts))
    room = st if len(st) else np.zeros(1, np.int32)
    out, sl, lv = np.full(F, -7, np.int32), np.full((B, T), -7, np.int32), np.full(B, -7, np.int32)
    rc = _lib.lib().p3d_debug_video_plan_shots(mode, F, T, B, last_start, cin.ctypes.data_as(_i32p), tb.ctypes.data_as(_i32p), len(tb),
                                               room.ctypes.data_as(_lib._ip), len(st) if n_windows is None else n_windows,
                                               out.ctypes.data_as(_i32p), sl.ctypes.data_as(_lib._ip), lv.ctypes.data_as(_lib._ip))
    return rc, out, sl, lv


def random_table(rng, F):
    """A shot table of F frames: 1 .. 8 shots, short ones (1, 2, a few frames) as likely as long ones."""
    n = int(rng.integers(1, 9))
    cuts = set()
    while len(cuts) < min(n - 1, F - 1):
        c = int(rng.integers(1, F))
        cuts.add(c)
        if rng.random() < 0.4 and c + int(rng.integers(1, 4)) < F:      # a short shot right behind it
            cuts.add(c + int(rng.integers(1, 4)))
    return [0] + sorted(c for c in cuts if c < F)


def test_the_headers_example_to_the_letter():
    F, table = sw.EXAMPLE_F, sw.EXAMPLE_TABLE
    from sap3d_tensorflow_amd import dataflow
    starts = dataflow.shot_window_starts(table, F, stride=4)
    assert starts == [0, 4, 20, 25, 26, 28] == sw.window_starts(table, F, 4)
    want = {20: ([20, 21, 22, 23, 24, 23, 22, 21, 20, 21, 22, 23, 24, 23, 22, 21], 5), 25: ([25] * 16, 1), 26: ([26, 27] * 8, 2),
            28: (list(range(28, 41)) + [39, 38, 37], 13), 0: (list(range(16)), 16), 4: (list(range(4, 20)), 16)}
    for s, (g, live) in want.items():
        assert sw.window(table, F, T, s) == (g, live), s
    for mode in (sw.NEWEST, sw.MEAN):
        rc, count, sl, lv = plan(mode, F, 6, -1, [0] * F, table, starts)
        assert rc == 0
        assert [sl[k].tolist() for k in range(6)] == [want[s][0] for s in starts]
        assert lv.tolist() == [want[s][1] for s in starts]
        assert count.min() >= 1                                            # every frame ends with a count of at least 1
        assert count.tolist() == ([1] * F if mode == sw.NEWEST else [1] * 4 + [2] * 12 + [1] * 25)
    rc, _, sl, lv = plan(sw.NEWEST, F, 4, -1, [0] * F, table, [20])       # a short call: the padding repeats the slot row, live 0
    assert rc == 0 and lv.tolist() == [5, 0, 0, 0] and all(sl[k].tolist() == want[20][0] for k in range(4))


@pytest.mark.parametrize("seed", range(4))
def test_plan_equals_the_replay_on_random_videos_tables_and_strides(seed):
    from sap3d_tensorflow_amd import dataflow
    rng = np.random.default_rng(seed)
    short = False
    for case in range(750):
        F, stride, B = int(rng.integers(16, 81)), int(rng.choice(STRIDES)), int(rng.integers(1, 5))
        table, mode = random_table(rng, F), int(rng.integers(0, 2))
        starts = dataflow.shot_window_starts(table, F, stride, T)
        assert starts == sw.window_starts(table, F, stride, T)
        assert all(a < b for a, b in zip(starts, starts[1:]))
        count, last = [0] * F, -1
        for i in range(0, len(starts), B):
            chunk = starts[i:i + B]
            sw.validate(mode, F, T, B, last, table, chunk)                 # the driver's law is legal
            want = sw.plan_counts(mode, F, T, B, last, count, table, chunk)
            g, live = sw.slots(table, F, T, B, chunk)
            rc, out, sl, lv = plan(mode, F, B, last, count, table, chunk)
            assert rc == 0, (F, table, chunk)
            assert out.tolist() == want and np.array_equal(sl, g) and lv.tolist() == live, (F, table, chunk)
            for k, s in enumerate(chunk):
                lo, hi = shots_ref.shot_of(table, F, s)
                assert lo <= g[k].min() and g[k].max() <= hi               # no slot leaves its shot
                assert g[k, :live[k]].tolist() == list(range(s, s + live[k]))
                short = short or live[k] < T
            count, last = want, chunk[-1]
        assert min(count) >= 1, (F, table, stride)                         # ... and leaves no frame without a prediction
    assert short


@pytest.mark.parametrize("seed", range(2))
def test_random_start_lists_are_refused_exactly_when_the_replay_refuses(seed):
    from sap3d_tensorflow_amd import _lib
    rng = np.random.default_rng(100 + seed)
    refused = accepted = 0
    for case in range(1500):
        F, B = int(rng.integers(16, 81)), int(rng.integers(1, 5))
        table, mode = random_table(rng, F), int(rng.integers(0, 2))
        last = int(rng.integers(-1, F // 2))
        legal = [s for s in sw.window_starts(table, F, int(rng.choice(STRIDES))) if s > last]
        kind = int(rng.integers(0, 5))
        if kind == 0 and legal:                                            # a legal call
            i = int(rng.integers(0, len(legal)))
            starts = legal[i:i + int(rng.integers(1, B + 1))]
        elif kind == 1:                                                    # any frames, ascending
            starts = sorted(set(rng.integers(-1, F + 1, int(rng.integers(1, B + 2))).tolist()))
        elif kind == 2 and legal:                                          # a legal call with one start moved by a frame or two
            i = int(rng.integers(0, len(legal)))
            starts = list(legal[i:i + B])
            starts[int(rng.integers(0, len(starts)))] += int(rng.choice((-2, -1, 1, 2)))
        elif kind == 3:                                                    # any order, repeats
            starts = rng.integers(0, F, int(rng.integers(1, B + 1))).tolist()
        else:                                                              # too few, too many
            starts = list(range(last + 1, F))[:int(rng.choice((0, B + 1)))]
        count = rng.integers(0, 3, F).tolist() if mode == sw.MEAN else rng.integers(0, 2, F).tolist()
        try:
            want = sw.plan_counts(mode, F, T, B, last, count, table, starts)
        except sw.Refused:
            want = None
        rc, out, sl, lv = plan(mode, F, B, last, count, table, starts)
        if want is None:
            refused += 1
            assert rc == -1, (F, table, last, starts)
            assert "video" in _lib.lib().p3d_last_error().decode()
            assert (out == -7).all() and (sl == -7).all() and (lv == -7).all()
        else:
            accepted += 1
            assert rc == 0 and out.tolist() == want, (F, table, last, starts)
    assert refused > 300 and accepted > 300


def test_refusals_name_the_window_and_its_shot():
    from sap3d_tensorflow_amd import _lib
    F, table = sw.EXAMPLE_F, sw.EXAMPLE_TABLE

    def message(starts, last=-1, tb=table):
        rc = plan(sw.MEAN, F, 3, last, [0] * F, tb, starts)[0]
        assert rc == -1, starts
        return _lib.lib().p3d_last_error().decode()
    assert "window 1" in message([0, 21]) and "[20, 24]" in message([0, 21])      # the middle of a short shot
    assert "window 0" in message([5]) and "[0, 19]" in message([5])               # crosses hi = 19
    assert "window 2" in message([0, 4, 4])
    assert "window 0" in message([4], last=4)
    assert "[0, F - 1 = 40]" in message([41])
    for tb in ([1, 20], [0, 20, 20], [0, 41]):
        assert "shot table" in message([0], tb=tb)
    assert plan(sw.MEAN, F, 3, -1, [0] * F, table, [4, 20, 27])[0] == -1          # 27 is the second frame of [26, 27]
    assert plan(sw.MEAN, F, 3, -1, [0] * F, table, [4, 20, 26])[0] == 0


@pytest.mark.parametrize("mode", [video_ref.NEWEST, video_ref.MEAN])
def test_a_table_of_one_shot_gives_the_plain_plans_counts(mode):
    from sap3d_tensorflow_amd import _lib
    rng = np.random.default_rng(7)
    for case in range(200):
        F, B, stride = int(rng.integers(16, 81)), int(rng.integers(1, 5)), int(rng.choice(STRIDES))
        starts = video_ref.window_starts(F, T, stride)
        assert sw.window_starts([0], F, stride) == starts
        count, last = [0] * F, -1
        for i in range(0, len(starts), B):
            chunk = np.ascontiguousarray(starts[i:i + B], np.int32)
            plain = np.full(F, -7, np.int32)
            assert _lib.lib().p3d_debug_video_plan(mode, F, T, B, last, np.ascontiguousarray(count, np.int32).ctypes.data_as(_i32p),
                                                   chunk.ctypes.data_as(_lib._ip), len(chunk), plain.ctypes.data_as(_i32p)) == 0
            rc, out, sl, lv = plan(mode, F, B, last, count, [0], chunk)
            assert rc == 0 and np.array_equal(out, plain)
            assert lv[:len(chunk)].tolist() == [T] * len(chunk)
            assert np.array_equal(sl[:len(chunk)], chunk[:, None] + np.arange(T)[None])      # the identity: p3d_video_predict's windows
            count, last = out.tolist(), int(chunk[-1])


def _gen_pred():
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


def test_the_driver_refuses_shot_windows_without_shots_before_anything_runs(tmp_path, capsys):
    gp = _gen_pred()
    with pytest.raises(SystemExit):
        gp.parse_args(["--videos", str(tmp_path), "--resident", "--shot-windows"])
    assert "--shot-windows needs --shots" in capsys.readouterr().err
    args = gp.parse_args(["--videos", str(tmp_path), "--resident", "--shots", "detect", "--shot-windows", "--stride", "4"])
    assert args.shot_windows and args.shots_kw["detect"] is not None
    assert not gp.parse_args(["--videos", str(tmp_path), "--resident", "--shots", "detect"]).shot_windows


def test_shot_window_starts_refuses_a_bad_table():
    from sap3d_tensorflow_amd import dataflow
    for table, F in (([], 20), ([1, 5], 20), ([0, 5, 5], 20), ([0, 20], 20)):
        with pytest.raises(ValueError):
            dataflow.shot_window_starts(table, F)
    with pytest.raises(ValueError):
        dataflow.shot_window_starts([0], 20, stride=0)
    assert dataflow.shot_window_starts([0], 20, stride=4) == [0, 4]
    assert dataflow.shot_window_starts([0, 3], 40, stride=16) == [0, 3, 19, 24]
