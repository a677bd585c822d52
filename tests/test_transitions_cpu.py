"""include/p3d_hip.h's "Gradual transitions" without a GPU: the numpy replay (tests/transitions_ref.py) on the planted video, the
property that the decision with dissolves and fades off is the cut decision, the q, r split of floor(S1^2 / P) against Python
integers, the host-only plan hook against the header's scratch law, and the new names of the ABI."""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import shots_ref                     # noqa: E402
import transitions_ref as tr         # noqa: E402

OFF = dict(tr.GRADUAL_DEFAULTS, lag=0, mono_min=0)


@pytest.fixture(scope="module")
def planted():
    """{(H, W): (D, E, v)} of the planted video at the three sizes, 4 x 4 grid, K = 12."""
    return dict(((H, W), tr.signals(tr.fixture(H, W), *tr.FIXTURE_GRID, 12)) for H, W in ((24, 40), (23, 37), (16, 16)))


def test_the_replay_finds_what_was_planted(planted):
    for (H, W), (D, E, v) in planted.items():
        P = H * W
        starts, kinds = tr.transitions(D, E, v, P, tr.FIXTURE_RULE, tr.GRADUAL_DEFAULTS)
        assert starts == tr.FIXTURE_STARTS == [0, 24, 48, 77, 126, 188], (H, W, starts)
        assert kinds == tr.FIXTURE_KINDS == [tr.FIRST, tr.DISSOLVE, tr.CUT, tr.FADE, tr.DISSOLVE, tr.CUT]
        # nothing at the flash (103), in the dissolve of 20 frames (148 .. 167) or in the pan (208 .. 220)
        assert not [s for s in starts if 100 <= s <= 106 or 140 <= s <= 180 or 200 <= s <= 235]
        cand, mono, high, fade, diss = tr.flags(D, E, v, P, tr.FIXTURE_RULE, tr.GRADUAL_DEFAULTS)
        assert [f for f in range(len(D)) if cand[f]] == [48, 188]
        assert tr.runs(mono) == [(74, 76), (103, 103)]      # the black frames, and the flash: too short for a fade
        assert [f for f in range(len(D)) if fade[f]] == [77] and [f for f in range(len(D)) if diss[f]] == [24, 126]
        # the pan and the long dissolve do raise E: DIP and LENGTH reject them, not HIGH
        assert any(p <= 214 <= q for p, q in tr.runs(high)) and any(p <= 158 <= q and q - p + 1 > 24 for p, q in tr.runs(high))
        # the three signals are what they claim to be
        assert np.array_equal(D, shots_ref.distances(tr.fixture(H, W), *tr.FIXTURE_GRID)) and not E[:12].any() and E[12:].any()
        assert v[75] == 0 and v[103] == 0 and v[10] > 0


def test_off_is_the_cut_decision(planted):
    for (H, W), (D, E, v) in planted.items():
        starts, kinds = tr.transitions(D, E, v, H * W, tr.FIXTURE_RULE, OFF)
        assert starts == tr.FIXTURE_OFF_STARTS == shots_ref.cuts(D, H * W, **tr.FIXTURE_RULE)
        assert kinds == [tr.FIRST, tr.CUT, tr.CUT]
    rng = np.random.default_rng(5)
    for F, window, ratio, min_length in ((300, 2, 300, 3), (257, 32, 256, 1), (64, 0, 512, 5), (1, 1, 256, 1)):
        D = rng.integers(0, 150, F).astype(np.uint32)
        D[0] = 0
        D[rng.integers(0, F, F // 10)] = 600
        E, v = rng.integers(0, 601, F), rng.integers(0, 2 ** 40, F)
        rule = dict(threshold=500, window=window, ratio=ratio, min_length=min_length)
        for off in (OFF, dict(OFF, high=1, dip=256, mono=65535)):
            starts, kinds = tr.transitions(D, E, v, 100, rule, off)
            assert starts == shots_ref.cuts(D, 100, **rule) and set(kinds[1:]) <= {tr.CUT}


def test_the_split_of_the_square_is_exact():
    """floor(S1^2 / P) = q^2 P + 2 q r + floor(r^2 / P), q = S1 / P, r = S1 - q P: for every P up to 2^28 and S1 up to 63 P, with no
    term above 64 bits (square_over asserts that)."""
    rng = np.random.default_rng(9)
    cases = [(63 * 2 ** 28, 2 ** 28), (63 * 2 ** 28 - 1, 2 ** 28), (2 ** 28 - 1, 2 ** 28), (0, 1), (63, 1), (62 * 2 ** 28 + 2 ** 28 - 1, 2 ** 28),
             (63 * (2 ** 28 - 1), 2 ** 28 - 1), (31 * 2073600 + 2073599, 2073600)]
    for _ in range(2000):
        P = int(rng.integers(1, 2 ** 28 + 1))
        cases.append((int(rng.integers(0, 63 * P + 1)), P))
    for S1, P in cases:
        assert 0 <= S1 <= 63 * P and tr.square_over(S1, P) == S1 * S1 // P, (S1, P)
    # and the spread built from it is the spread as written, on a frame whose S1 is large
    frame = np.full((16, 16, 3), 255, np.uint8)
    frame[:8] = 0
    h = shots_ref.histograms(frame, 2, 2)
    assert tr.spread_exact(h, 256) == 3 * (63 * 63 * 128 - (63 * 128) ** 2 // 256) == 3 * 63 * 63 * 64


def test_the_plan_hook_follows_the_stated_scratch_law():
    from sap3d_tensorflow_amd import _lib, dataflow
    chunk = dataflow.shots_plan(5, 7, (2, 3), 65535)["frames_per_chunk"]
    assert chunk == 64
    for H, W, grid, n, lag in ((5, 7, (2, 3), 1, 12), (5, 7, (2, 3), 64, 2), (5, 7, (1, 1), 65, 64), (1080, 1920, (4, 4), 65535, 12), (23, 37, (4, 4), 79, 0),
                               (1, 1, (1, 1), 2, 64)):
        plan = dataflow.transitions_plan(H, W, grid, n, lag)
        assert plan["tables"] == min(n, chunk) + max(lag, 1), (H, W, grid, n, lag, plan)
        assert plan["scratch_bytes"] == plan["tables"] * grid[0] * grid[1] * 192 * 4
    for kw in (dict(lag=1), dict(lag=65), dict(lag=-1), dict(grid=(5, 1)), dict(n=0), dict(n=65536)):
        args = dict(H=5, W=7, grid=(2, 3), n=3, lag=12)
        args.update(kw)
        with pytest.raises(_lib.P3dError):
            dataflow.transitions_plan(**args)


def test_symbols_are_exported_and_bound():
    from sap3d_tensorflow_amd import P3DSession, _lib, dataflow
    lib = _lib.lib()
    for name in ("p3d_shot_signals_u8", "p3d_shot_transitions", "p3d_video_detect_transitions", "p3d_video_get_shot_kinds",
                 "p3d_debug_shot_signals_u8", "p3d_debug_transitions_plan", "p3d_debug_transitions_time"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes is not None, name
    assert [_lib.K[k] for k in ("P3D_GRADUAL_LAG", "P3D_GRADUAL_HIGH", "P3D_GRADUAL_DIP", "P3D_GRADUAL_MONO", "P3D_GRADUAL_MONO_MIN")] == [0, 1, 2, 3, 4]
    assert [_lib.K[k] for k in ("P3D_SHOT_FIRST", "P3D_SHOT_CUT", "P3D_SHOT_FADE", "P3D_SHOT_DISSOLVE")] == [tr.FIRST, tr.CUT, tr.FADE, tr.DISSOLVE]
    assert list(dataflow.gradual_cfg()) == [12, 250, 230, 768, 2] == [tr.GRADUAL_DEFAULTS[k] for k in ("lag", "high", "dip", "mono", "mono_min")]
    for name in ("video_detect_transitions", "video_shot_kinds"):
        assert callable(getattr(P3DSession, name))
    for name in ("shot_signals_u8", "shot_transitions", "transitions_plan", "transitions_time"):
        assert callable(getattr(dataflow, name))


def _gen_pred():
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


def test_the_driver_checks_the_gradual_flags_before_anything_runs(tmp_path, capsys):
    gp = _gen_pred()
    head = ["--videos", str(tmp_path)]
    assert gp.GRADUAL_DEFAULTS == tr.GRADUAL_DEFAULTS
    args = gp.parse_args(head + ["--resident", "--shots", "detect"])
    assert "gradual" not in args.shots_kw and args.shots_kw["detect"] == gp.SHOTS_DEFAULTS      # without the flag: today's request
    args = gp.parse_args(head + ["--resident", "--shots", "detect", "--shots-gradual", "--shots-lag", "20", "--shots-mono-min", "0"])
    assert args.shots_kw["gradual"] == dict(tr.GRADUAL_DEFAULTS, lag=20, mono_min=0)
    for tail, word in ((["--shots-gradual"], "--shots detect"), (["--resident", "--shots", "detect", "--shots-lag", "8"], "--shots-gradual"),
                       (["--resident", "--shots", "detect", "--shots-gradual", "--shots-lag", "1"], "--shots-lag"),
                       (["--resident", "--shots", "detect", "--shots-gradual", "--shots-lag", "65"], "--shots-lag"),
                       (["--resident", "--shots", "detect", "--shots-gradual", "--shots-high", "0"], "--shots-high"),
                       (["--resident", "--shots", "detect", "--shots-gradual", "--shots-dip", "257"], "--shots-dip"),
                       (["--resident", "--shots", "detect", "--shots-gradual", "--shots-mono", "65536"], "--shots-mono"),
                       (["--resident", "--shots", "detect", "--shots-gradual", "--shots-mono-min", "-1"], "--shots-mono-min")):
        with pytest.raises(SystemExit):
            gp.parse_args(head + tail)
        assert word in capsys.readouterr().err, tail
