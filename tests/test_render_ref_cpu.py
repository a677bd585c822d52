"""What tests/render_ref.py claims, without a GPU: the shifted-array replay of include/p3d_hip.h's "Rendering 8-bit maps" equals a
per-pixel loop written from the contract, the blend is round-to-nearest over every triple, the contour's edge cases are the
contract's, dataflow.render_table builds the stated tables, and the boundary (symbols, plan hook) answers without a device."""
import math
import os

import numpy as np
import pytest

import render_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("p3d_render_u8", "p3d_video_keep_source", "p3d_video_source_info", "p3d_video_render", "p3d_debug_render_u8",
           "p3d_debug_render_plan")
SHAPES = [(1, 1), (2, 3), (3, 5), (7, 19)]


def loop_render(s, frame, table, L, t, cbgr):
    """One map, pixel by pixel, from the contract's sentences."""
    H, W = s.shape
    out = np.zeros((H, W, 3), np.uint8)
    for y in range(H):
        for x in range(W):
            e = int(table[s[y, x]])
            c, o = (e & 255, (e >> 8) & 255, (e >> 16) & 255), e >> 24
            for k in range(3):
                out[y, x, k] = c[k] if frame is None else (int(frame[y, x, k]) * (255 - o) + c[k] * o + 127) // 255
            if L > 0 and s[y, x] >= L:
                near = False
                for yy in range(y - t, y + t + 1):
                    for xx in range(x - t, x + t + 1):
                        if 0 <= yy < H and 0 <= xx < W and s[yy, xx] < L:
                            near = True
                if near:
                    out[y, x] = cbgr
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_replay_equals_the_per_pixel_loop(shape):
    rng = np.random.default_rng(shape)
    table = R.tables()["random"]
    cbgr = (3, 250, 77)
    for trial in range(3):
        s = rng.integers(0, 256, shape, dtype=np.uint8) if trial else R.blob(1, *shape)[0]
        if trial == 2:
            s = np.where(s >= 128, 255, s).astype(np.uint8)        # some pixels reach the top level
        frame = R.frames_for(s)
        for f in (frame, None):
            for L in (1, 128, 255):
                for t in (1, 2, 3, 4):
                    want = loop_render(s, f, table, L, t, cbgr)
                    got = R.render(s, f, table, L, t, cbgr)
                    assert np.array_equal(got, want), (shape, L, t, f is None)
            assert np.array_equal(R.render(s, f, table), loop_render(s, f, table, 0, 1, cbgr))
    # a batch is its maps, one by one
    sal = R.blob(3, *shape)
    fr = R.frames_for(sal)
    got = R.render(sal, fr, table, 128, 2, cbgr)
    for i in range(3):
        assert np.array_equal(got[i], loop_render(sal[i], fr[i], table, 128, 2, cbgr))


def test_blend_is_round_to_nearest_over_every_triple():
    f, c, o = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    x = f * (255 - o) + c * o
    got = R.blend(f, c, o)
    assert int(x.max()) + 127 == 65152
    assert np.array_equal(got, np.floor(x / 255. + 0.5).astype(np.int64))
    assert not np.any((2 * x) % 510 == 255)                              # 255 is odd: x / 255 is never k + 1/2, no tie exists
    assert np.array_equal(got[:, :, 0], f[:, :, 0]) and np.array_equal(got[:, :, 255], c[:, :, 255])
    # round-to-nearest, from the integers: |255 got - x| <= 127
    assert int(np.abs(255 * got - x).max()) <= 127


def test_contour_edge_cases():
    for t in (1, 2, 3, 4):
        full = np.full((9, 11), 200, np.uint8)
        assert not R.contour_mask(full, 128, t).any()                       # all at or above L
        assert not R.contour_mask(full, 201, t).any()                       # all below L
        # a region touching the border: no line along the border
        s = np.zeros((20, 24), np.uint8)
        s[:10, :12] = 255
        m = R.contour_mask(s, 128, t)
        want = np.zeros_like(m)
        want[10 - t:10, :12] = True
        want[:10, 12 - t:12] = True
        assert np.array_equal(m, want)
        assert not m[0, :12 - t].any() and not m[:10 - t, 0].any()
        # a single pixel below L in a map of ones: a (2t + 1)^2 ring minus the pixel itself, clipped at the border
        for (y, x) in ((10, 12), (0, 0), (1, 22), (19, 3)):
            s = np.ones((20, 24), np.uint8)
            s[y, x] = 0
            m = R.contour_mask(s, 1, t)
            want = np.zeros_like(m)
            want[max(0, y - t):y + t + 1, max(0, x - t):x + t + 1] = True
            want[y, x] = False
            assert np.array_equal(m, want)
            inside = min(y + t, 19) - max(0, y - t) + 1, min(x + t, 23) - max(0, x - t) + 1
            assert int(m.sum()) == inside[0] * inside[1] - 1
    # the counts the issue records for the blob maps at L = 128, t = 1 are of this kind: some, not all, of the level set
    for shape in ((3, 5), (7, 19), (263, 251)):
        s = R.blob(1, *shape)[0]
        m = R.contour_mask(s, 128, 1)
        assert 0 < int(m.sum()) < int((s >= 128).sum()), shape


def test_render_table():
    from sap3d_tensorflow_amd import dataflow
    jet = dataflow.render_table("jet", 1.0, "constant")
    c, o = R.unpack(jet)
    assert tuple(c[0]) == (128, 0, 0) and tuple(c[128]) == (126, 255, 130) and tuple(c[255]) == (0, 0, 128)
    assert np.all(o == 255)
    grey, _ = R.unpack(dataflow.render_table("grey", 0.5, "ramp"))
    assert np.array_equal(grey, np.repeat(np.arange(256)[:, None], 3, axis=1))
    hot, _ = R.unpack(dataflow.render_table("hot", 0.5, "ramp"))
    for tab in (grey, hot):
        assert np.all(np.diff(tab, axis=0) >= 0)
    assert tuple(hot[0]) == (0, 0, 0) and tuple(hot[255]) == (255, 255, 255) and tuple(hot[85]) == (0, 0, 255)      # B, G, R
    for alpha in (0., 0.6, 1.):
        _, oc = R.unpack(dataflow.render_table("jet", alpha, "constant"))
        _, orr = R.unpack(dataflow.render_table("jet", alpha, "ramp"))
        assert np.all(oc == math.floor(255. * alpha + 0.5))
        assert [int(v) for v in orr] == [math.floor(alpha * v + 0.5) for v in range(256)]
    assert int(R.unpack(dataflow.render_table("jet", 0.6, "constant"))[1][7]) == 153
    assert np.array_equal(R.unpack(dataflow.render_table("jet", 1., "ramp"))[1], np.arange(256))
    for op in ("constant", "ramp"):
        _, og = R.unpack(dataflow.render_table("hot", 0.6, op, gate=40))
        _, o0 = R.unpack(dataflow.render_table("hot", 0.6, op))
        assert np.all(og[:40] == 0) and np.array_equal(og[40:], o0[40:]) and og[40] > 0
    t = dataflow.render_table()
    assert t.dtype == np.uint32 and t.shape == (256,)
    for bad in (dict(colormap="viridis"), dict(opacity="step"), dict(alpha=1.5), dict(gate=-1)):
        with pytest.raises(ValueError):
            dataflow.render_table(**bad)


def test_symbols_are_declared_exported_and_bound():
    """The seven new names of the header: the six functions, exported and bound, and the p3d_render struct."""
    from test_abi_cpu import declared_symbols
    from sap3d_tensorflow_amd import _lib, P3DSession, dataflow
    assert set(SYMBOLS) <= set(declared_symbols())
    hdr = open(os.path.join(ROOT, "include", "p3d_hip.h")).read()
    assert "} p3d_render;" in hdr
    for n in SYMBOLS:
        assert hasattr(_lib.lib(), n) and n in _lib.SIGNATURES
    import ctypes as C
    assert C.sizeof(_lib.P3dRender) == 1024 + 4 + 4 + 4 and _lib.P3dRender.contour_bgr.offset == 1032
    for m in ("video_keep_source", "video_source_info", "video_render"):
        assert hasattr(P3DSession, m)
    cfg = dataflow.render_cfg(R.tables()["random"], 128, 2, (1, 2, 3))
    assert list(cfg.contour_bgr) == [3, 2, 1] and cfg.contour_level == 128 and cfg.table[5] == int(R.tables()["random"][5])


def test_plan_hook_needs_no_device():
    from sap3d_tensorflow_amd import P3dError, dataflow
    r, c, p = dataflow.render_plan(1080, 1920)
    assert (r, c) == (0, 0) and p % 16 == 0 and p >= 256          # flat runs that keep a map's alignment
    r, c, p = dataflow.render_plan(1080, 1920, thickness=1)
    assert r >= 4 and c >= 16 and p == r * c
    assert dataflow.render_plan(3, 5, n=5, thickness=4, offset=15) == (r, c, p)
    for bad in ((0, 5, 1, 0, 0), (2 ** 14, 2 ** 14 + 1, 1, 0, 0), (3, 5, 0, 0, 0), (3, 5, 1, 5, 0), (3, 5, 1, 0, 16)):
        with pytest.raises(P3dError):
            dataflow.render_plan(*bad)


def test_python_refusals_come_before_the_library():
    from sap3d_tensorflow_amd import dataflow
    t = R.tables()["random"]
    z = np.zeros((4, 4), np.uint8)
    with pytest.raises(ValueError):
        dataflow.render_overlay(z.astype(np.float32), None, t)
    with pytest.raises(ValueError):
        dataflow.render_overlay(z, np.zeros((4, 5, 3), np.uint8), t)
    with pytest.raises(ValueError):
        dataflow.render_overlay(z, None, t.astype(np.int64))
    with pytest.raises(ValueError):
        dataflow.render_overlay(z, None, t, contour=10, contour_color=(1, 2))


def test_driver_refuses_render_flags_that_cannot_apply(tmp_path):
    """drivers/gen_pred.py: --render without --resident, a --render-* flag without --render and values video_render would refuse
    end the run before anything is loaded."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_pred_render_cpu", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    base = ["--videos", str(tmp_path)]
    for bad in (["--render", str(tmp_path / "r")], ["--resident", "--render-alpha", "0.5"],
                ["--resident", "--render", str(tmp_path / "r"), "--render-thickness", "5"],
                ["--resident", "--render", str(tmp_path / "r"), "--render-contour", "256"],
                ["--resident", "--render", str(tmp_path / "r"), "--render-contour-color", "1,2"]):
        with pytest.raises(SystemExit):
            gp.parse_args(base + bad)
    ok = gp.parse_args(base + ["--resident", "--render", str(tmp_path / "r"), "--render-contour", "128", "--render-contour-color", "1,2,3"])
    assert ok.render_kw["contour"] == 128 and ok.render_kw["contour_color"] == (1, 2, 3) and ok.render_kw["colormap"] == "jet"
    assert gp.parse_args(base).render_kw is None
