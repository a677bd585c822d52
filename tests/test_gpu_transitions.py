"""The kernels of csrc/shots.hip behind "Gradual transitions": the signal through p3d_debug_shot_signals_u8 (every device buffer, the
scratch included, between guards) and the decision through p3d_shot_transitions (guards as well), against tests/transitions_ref.py,
tolerance 0.  Shapes and frame counts are the smallest at which each path can go wrong: one pixel, rows shorter than a 16-byte word,
odd sizes, 1, 2, K, K + 1 frames and a chunk of tables plus its carry plus three, at the least, a middle and the largest lag."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import shots_ref as S          # noqa: E402
import transitions_ref as T    # noqa: E402

SHAPES = [(1, 1), (5, 7), (23, 37), (24, 40)]
LAGS = [2, 12, 64]
GRIDS = [(1, 1), (1, 4), (4, 1), (4, 4), (2, 3)]


def grid_in(grid, H, W):
    return min(grid[0], H), min(grid[1], W)


def moving_frames(n, H, W, lag, seed):
    """Noise whose frames differ from the one before and from the one `lag` before in different ways: some frames repeat the frame
    before (D = 0, E > 0), some the frame `lag` before (E = 0, D > 0), some are flat (v = 0)."""
    frames = S.noise_frames(n, H, W, seed=seed)
    for f in range(1, n):
        if f % 7 == 3:
            frames[f] = frames[f - 1]
        elif lag and f >= lag and f % 5 == 1:
            frames[f] = frames[f - lag]
        elif f % 11 == 6:
            frames[f] = 4 * (f % 64)
    return frames


def check(frames, grid, lag, offset=0, what=""):
    from sap3d_tensorflow_amd import dataflow
    want = T.signals(frames, *grid, lag)
    got = dataflow.shot_signals_u8(frames, grid, lag, offset=offset)
    for name, g, w, dtype in zip("DEv", got, want, (np.uint32, np.uint32, np.int64)):
        assert g.dtype == dtype and g.shape == w.shape
        assert np.array_equal(g, w), (what, name, frames.shape, grid, "lag", lag, "offset", offset, g[:8].tolist(), w[:8].tolist())
    return want


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("lag", LAGS)
def test_shapes_frame_counts_and_lags(shape, lag):
    from sap3d_tensorflow_amd import dataflow
    H, W = shape
    grid = grid_in((4, 4), H, W)
    for n in (1, 2, lag, lag + 1, 64 + lag + 3):
        D, E, v = check(moving_frames(n, H, W, lag, seed=n), grid, lag, offset=(H + n) % 16, what="shapes")
        assert D[0] == 0 and not E[:lag].any()
        assert dataflow.transitions_plan(H, W, grid, n, lag)["tables"] == min(n, 64) + lag
        if n > lag + 8 and H * W > 1:
            assert E[lag:].any() and (E[lag:] == 0).any() and (E != D).any() and (v == 0).any() and v.any()


def test_lag_zero_leaves_E_zero():
    D, E, v = check(moving_frames(70, 5, 7, 0, seed=1), (2, 3), 0, offset=9, what="lag 0")
    assert not E.any() and D.any()


@pytest.mark.parametrize("grid", GRIDS)
def test_every_corner_of_the_grid(grid):
    """23 x 37: cells of 5 and 6 rows, of 9 and 10 columns.  v does not depend on the grid."""
    frames = moving_frames(17, 23, 37, 12, seed=3)
    _, _, v = check(frames, grid, 12, offset=7, what="grids")
    assert np.array_equal(v, T.signals(frames, 1, 1, 0)[2])


@pytest.mark.parametrize("offset", range(16))
def test_every_offset_off_the_16_byte_boundary(offset):
    frames = moving_frames(5, 5, 7, 2, seed=offset)
    check(frames, (2, 3), 2, offset=offset, what="5x7")


def test_the_32_bit_headroom():
    """1080 x 1920, as the cut signal's headroom test: all 0 against all 255 two frames apart, so E = D = 6 P, and a frame half 0 and
    half 255, whose spread is the largest a frame of P pixels has: 3 * 63^2 * P / 4, from S1 = 63 P / 2 with q = 31 and r = P / 2."""
    from sap3d_tensorflow_amd import dataflow
    H, W = 1080, 1920
    P = H * W
    frames = np.zeros((4, H, W, 3), np.uint8)
    frames[2] = 255
    frames[3, H // 2:] = 255
    for grid in ((1, 1), (4, 4)):
        D, E, v = dataflow.shot_signals_u8(frames, grid, 2)
        assert D.tolist() == [0, 0, 6 * P, 3 * P] and E.tolist() == [0, 0, 6 * P, 3 * P]
        assert v.tolist() == [0, 0, 0, 3 * 63 * 63 * P // 4]
    h = np.zeros((1, 1, 3, 64), np.int64)
    h[..., 0] = h[..., 63] = P // 2
    assert T.spread_exact(h, P) == 3 * 63 * 63 * P // 4 and T.square_over(63 * P // 2, P) == (63 * P // 2) ** 2 // P


def test_op_level_entry_equals_the_hook():
    from sap3d_tensorflow_amd import dataflow
    frames = T.fixture(23, 37)[:90]
    for grid, lag in (((1, 1), 2), ((2, 3), 12), ((4, 4), 64)):
        want = T.signals(frames, *grid, lag)
        for got in (dataflow.shot_signals_u8(frames, grid, lag), dataflow.shot_signals_u8(frames, grid, lag, offset=5)):
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), (grid, lag)


def decide(D, E, v, P, rule, gradual, cap=None):
    from sap3d_tensorflow_amd import dataflow
    starts, kinds, count = dataflow.shot_transitions(D, E, v, P, cap=cap, **rule, **gradual)
    assert starts.dtype == np.int32 and kinds.dtype == np.int32
    return starts.tolist(), kinds.tolist(), count


@pytest.mark.parametrize("shape", [(24, 40), (23, 37), (16, 16)])
def test_the_decision_on_the_planted_video(shape):
    """The signals are the replay's, so that this holds the decision alone."""
    H, W = shape
    D, E, v = T.signals(T.fixture(H, W), *T.FIXTURE_GRID, 12)
    starts, kinds, count = decide(D, E, v, H * W, T.FIXTURE_RULE, T.GRADUAL_DEFAULTS)
    assert (starts, kinds) == T.transitions(D, E, v, H * W, T.FIXTURE_RULE, T.GRADUAL_DEFAULTS) == (T.FIXTURE_STARTS, T.FIXTURE_KINDS)
    assert count == len(T.FIXTURE_STARTS)
    off = dict(T.GRADUAL_DEFAULTS, lag=0, mono_min=0)
    assert decide(D, E, v, H * W, T.FIXTURE_RULE, off)[0] == T.FIXTURE_OFF_STARTS == S.cuts(D, H * W, **T.FIXTURE_RULE)
    for gradual in (dict(T.GRADUAL_DEFAULTS, lag=0), dict(T.GRADUAL_DEFAULTS, mono_min=0), dict(T.GRADUAL_DEFAULTS, dip=256), dict(T.GRADUAL_DEFAULTS, lag=20),
                    dict(T.GRADUAL_DEFAULTS, mono_min=1)):
        E2 = T.signals(T.fixture(H, W), *T.FIXTURE_GRID, gradual["lag"])[1] if gradual["lag"] not in (0, 12) else E
        assert decide(D, E2, v, H * W, T.FIXTURE_RULE, gradual)[:2] == T.transitions(D, E2, v, H * W, T.FIXTURE_RULE, gradual), gradual


def random_signals(rng, F, K):
    """P = 100.  D with spikes; E low with runs of 600 of every length about K; v high, with dips inside some runs and runs of 0."""
    D = rng.integers(0, 150, F).astype(np.uint32)
    D[0] = 0
    D[rng.integers(0, F, F // 25)] = 600
    E = rng.integers(0, 100, F).astype(np.uint32)
    v = rng.integers(20000, 40000, F).astype(np.int64)
    f = 0
    while f < F:
        n = int(rng.integers(1, 3 * max(K, 2) + 2))
        kind = int(rng.integers(0, 4))
        if kind == 0:
            E[f:f + n] = rng.integers(150, 601, len(E[f:f + n]))
            if rng.integers(0, 2):
                mid = f + n // 2 - K // 2
                v[max(mid - 1, 0):mid + 2] //= int(rng.integers(1, 4))
        elif kind == 1:
            v[f:f + min(n, 6)] = rng.choice([0, 300, 25599, 25600], 1)[0]
        f += n + int(rng.integers(0, 2 * max(K, 2)))
    return D, E, v


def test_the_decision_on_random_signals_over_the_config_range():
    rng = np.random.default_rng(21)
    seen = set()
    cases = [(F, K) for K in (0, 2, 5, 12, 64) for F in (1, 2, K + 1, 300, 257)] + [(2000, 12)]
    for i, (F, K) in enumerate(cases):
        D, E, v = random_signals(rng, F, K)
        rule = dict(threshold=int(rng.choice([250, 1000])), window=int(rng.choice([0, 2, 32])), ratio=int(rng.choice([256, 512])),
                    min_length=int(rng.choice([1, 3, 10])))
        for high, dip, mono, mono_min in ((250, 230, 768, 2), (1, 256, 0, 1), (1000, 1, 65535, 0), (25, 128, 768, 5), (250, 256, 65535, 1)):
            gradual = dict(lag=K, high=high, dip=dip, mono=mono, mono_min=mono_min)
            want = T.transitions(D, E, v, 100, rule, gradual)
            assert decide(D, E, v, 100, rule, gradual)[:2] == want, (F, rule, gradual)
            seen |= set(want[1])
            if K == 0 and mono_min == 0:
                assert want[0] == S.cuts(D, 100, **rule)
    assert seen == {T.FIRST, T.CUT, T.FADE, T.DISSOLVE}
    # 64-bit products at the largest P
    P = 2 ** 28
    D = np.array([0, 3, 6 * P, 3, 3, 3, 3, 3, 3, 3], np.uint32)
    E = np.array([0, 0, 6 * P, 6 * P, 6 * P - 1, 0, 0, 0, 0, 0], np.uint32)
    v = np.array([2 ** 40 - 1] * 5 + [0, 0, 65535 * 2 ** 20, 65535 * 2 ** 20 + 1, 2 ** 40 - 1], np.int64)
    for gradual in (dict(lag=2, high=1000, dip=256, mono=65535, mono_min=2), dict(lag=2, high=1000, dip=256, mono=0, mono_min=2)):
        rule = dict(threshold=1000, window=32, ratio=65535, min_length=1)
        assert decide(D, E, v, P, rule, gradual)[:2] == T.transitions(D, E, v, P, rule, gradual), gradual


def test_a_small_cap_keeps_the_count():
    D = np.array([0] + [600] * 9, np.uint32)
    E, v = np.zeros(10, np.uint32), np.full(10, 5000, np.int64)
    rule = dict(threshold=1000, window=0, ratio=256, min_length=1)
    starts, kinds, count = decide(D, E, v, 100, rule, T.GRADUAL_DEFAULTS, cap=3)
    assert count == 10 and starts == [0, 1, 2] and kinds == [T.FIRST, T.CUT, T.CUT]


def test_refusals_launch_nothing():
    """Every refusal leaves p3d_last_error set, and happens ahead of any launch: the outputs keep what they held."""
    from sap3d_tensorflow_amd import _lib, dataflow
    lib = _lib.lib()
    frames = S.noise_frames(3, 5, 7)
    u8, u32, i32, i64 = _lib._u8p, _lib._u32p, _lib._i32p, _lib._i64p

    def signal(n=3, H=5, W=7, gy=2, gx=3, lag=2, offset=0, hook=False, fr=frames, without=None):
        D, E, v = np.full(3, 7, np.uint32), np.full(3, 7, np.uint32), np.full(3, 7, np.int64)
        out = [D.ctypes.data_as(u32), E.ctypes.data_as(u32), v.ctypes.data_as(i64)]
        if without is not None:
            out[without] = None
        head = (0, None if fr is None else fr.ctypes.data_as(u8), n, H, W, gy, gx, lag)
        rc = lib.p3d_debug_shot_signals_u8(*head, offset, *out) if hook else lib.p3d_shot_signals_u8(*head, *out)
        return rc, lib.p3d_last_error().decode(), bool((D == 7).all() and (E == 7).all() and (v == 7).all())

    for hook in (False, True):
        rc, _, untouched = signal(hook=hook)
        assert rc == 0 and not untouched
        for kw, word in ((dict(n=0), "frames"), (dict(n=65536), "frames"), (dict(H=0), "empty"), (dict(W=0), "empty"), (dict(H=2 ** 14, W=2 ** 14 + 1), "2^28"),
                         (dict(gy=0), "grid"), (dict(gy=5), "grid"), (dict(gx=5), "grid"), (dict(H=1, gy=2), "grid"), (dict(lag=1), "lag"),
                         (dict(lag=65), "lag"), (dict(lag=-2), "lag"), (dict(fr=None), "null"), (dict(without=0), "null"), (dict(without=1), "null"),
                         (dict(without=2), "null")):
            rc, err, untouched = signal(hook=hook, **kw)
            assert rc == -1 and word in err and untouched, (hook, kw, rc, err)
    for kw, word in ((dict(offset=16), "offset"), (dict(offset=-1), "offset")):
        rc, err, untouched = signal(hook=True, **kw)
        assert rc == -1 and word in err and untouched, (kw, rc, err)

    def decision(F=4, P=100, cap=4, without=None, v3=5000, rule=None, **gradual):
        D, E, v = np.array([0, 600, 0, 600], np.uint32), np.zeros(4, np.uint32), np.array([5000, 5000, 5000, v3], np.int64)
        starts, kinds, count = np.full(4, -7, np.int32), np.full(4, -7, np.int32), C.c_int(-7)
        r = dict(threshold=500, window=1, ratio=256, min_length=1)
        r.update(rule or {})
        g = dict(T.GRADUAL_DEFAULTS)
        g.update(gradual)
        args = [D.ctypes.data_as(u32), E.ctypes.data_as(u32), v.ctypes.data_as(i64), F, P, dataflow.shots_cfg((1, 1), **r), dataflow.gradual_cfg(**g),
                starts.ctypes.data_as(i32), kinds.ctypes.data_as(i32), cap, C.byref(count)]
        if without is not None:
            args[without] = None
        rc = lib.p3d_shot_transitions(0, *args)
        return rc, lib.p3d_last_error().decode(), bool((starts == -7).all() and (kinds == -7).all() and count.value == -7)

    rc, _, untouched = decision()
    assert rc == 0 and not untouched
    for kw, word in ((dict(F=0), "frames"), (dict(F=65536), "frames"), (dict(P=0), "2^28"), (dict(P=2 ** 28 + 1), "2^28"), (dict(cap=0), "room"),
                     (dict(rule=dict(threshold=0)), "threshold"), (dict(rule=dict(window=33)), "window"), (dict(rule=dict(ratio=255)), "ratio"),
                     (dict(rule=dict(min_length=0)), "minimum length"), (dict(lag=1), "lag"), (dict(lag=65), "lag"), (dict(high=0), "high"),
                     (dict(high=1001), "high"), (dict(dip=0), "dip"), (dict(dip=257), "dip"), (dict(mono=-1), "mono"), (dict(mono=65536), "mono"),
                     (dict(mono_min=-1), "mono_min"), (dict(v3=-1), "2^40"), (dict(v3=2 ** 40), "2^40"), (dict(without=0), "null"), (dict(without=1), "null"),
                     (dict(without=2), "null"), (dict(without=5), "null"), (dict(without=6), "null"), (dict(without=7), "null"), (dict(without=8), "null")):
        rc, err, untouched = decision(**kw)
        assert rc == -1 and word in err and untouched, (kw, rc, err)
