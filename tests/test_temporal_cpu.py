"""No-GPU checks of the temporal smoothing of a resident video's maps (include/p3d_hip.h, "Temporal smoothing"): the numpy replay
tests/temporal_ref.py against float64 within derived bounds, its symmetries, the frames a read needs and every refusal against the
library's host-only paths (the plan hook, and the op-level hook, which decides its refusals before its first HIP call), the
bindings, and the driver's argument handling."""
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import temporal_ref as tr        # noqa: E402
import video_ref as vr           # noqa: E402

U = 2.0 ** -24
NEW = ["p3d_set_video_temporal", "p3d_get_video_temporal", "p3d_video_temporal_last_ms", "p3d_temporal_filter", "p3d_debug_video_temporal",
       "p3d_debug_video_temporal_plan", "p3d_debug_video_temporal_desc"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gamma(n):
    return n * U / (1.0 - n * U)


def _video(F, hw, seed):
    return np.random.default_rng(seed).standard_normal((F, hw)).astype(np.float32)


# ---- the replay against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,r,sigma", [(41, 1, 0.8), (41, 15, 5.0), (41, 24, 9.0), (16, 15, 4.0), (16, 6, 1.5)])
def test_gauss_replay_is_within_the_derived_bound_of_float64(F, r, sigma):
    """|err| <= gamma_{r+2} * sum_k |w_k| |v_k|: every term w (a + b) sees two roundings (the inner add and the product) and then at
    most r adds of the running sum; gamma_n = n u / (1 - n u), u = 2^-24."""
    cfg = tr.parse(tr.GAUSS, sigma, r)
    assert cfg["r"] == r and len(cfg["w"]) == 2 * r + 1
    v = _video(F, 50, F * 100 + r)
    got = tr.gauss(v, cfg["w"], r).astype(np.float64)
    w64, v64 = cfg["w"].astype(np.float64), v.astype(np.float64)
    want, mag = np.zeros_like(v64), np.zeros_like(v64)
    for f in range(F):
        want[f] = w64[r] * v64[f]
        mag[f] = abs(w64[r]) * abs(v64[f])
        for d in range(1, r + 1):
            a, b = v64[tr.rho(f - d, F)], v64[tr.rho(f + d, F)]
            want[f] += w64[r + d] * (a + b)
            mag[f] += abs(w64[r + d]) * (abs(a) + abs(b))
    err = np.abs(got - want)
    assert np.all(err <= gamma(r + 2) * mag), float(np.max(err / mag))
    assert np.max(err) > 0.0      # (float32 arithmetic: the comparison is not vacuous)


@pytest.mark.parametrize("alpha", [0.0, 0.5, 0.75, 0.9375, 0.99])
def test_ema_replay_is_within_the_derived_bound_of_the_float64_recurrence(alpha):
    """|err| <= 4 u max|v| / (1 - alpha) (1 + 1e-3): three roundings a step (two products, one add) on values of at most max|v|, plus
    the rounding of b = 1 - alpha; the recurrence contracts errors by alpha, so they sum to 1 / (1 - alpha); the last factor covers
    the second-order terms."""
    F = 300
    v = _video(F, 40, 7)
    got = tr.ema(v, alpha).astype(np.float64)
    a = float(np.float32(alpha))
    want = np.empty((F, 40))
    m = v[0].astype(np.float64)
    for f in range(F):
        if f:
            m = a * m + (1.0 - a) * v[f].astype(np.float64)
        want[f] = m
    assert np.array_equal(bits(got[0].astype(np.float32)), bits(v[0]))
    bound = 4 * U * float(np.max(np.abs(v))) / (1.0 - a) * (1 + 1e-3)
    assert np.max(np.abs(got - want)) <= bound


def test_gauss_commutes_with_time_reversal_bit_for_bit():
    for F, r, sigma in ((41, 24, 7.0), (16, 15, 3.0), (20, 6, 1.5)):
        cfg = tr.parse(tr.GAUSS, sigma, r)
        v = _video(F, 33, F + r)
        a = tr.gauss(np.ascontiguousarray(v[::-1]), cfg["w"], r)
        b = tr.gauss(v, cfg["w"], r)[::-1]
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("kind", ["gauss", "ema"])
def test_a_partial_read_is_the_slice_of_the_full_read(kind):
    F = 20
    cfg = tr.parse(tr.GAUSS, 1.5) if kind == "gauss" else tr.parse(tr.EMA, alpha=0.75)
    rng = np.random.default_rng(3)
    store = rng.standard_normal((F, 17)).astype(np.float32)
    count = rng.integers(1, 6, F).tolist()
    for mode in (vr.NEWEST, vr.MEAN):
        full = tr.filter_maps(cfg, mode, store, count)
        for first, n in ((0, F), (0, 1), (F - 1, 1), (5, 7), (3, 5)):
            assert np.array_equal(bits(tr.filter_maps(cfg, mode, store, count, first, n)), bits(full[first:first + n])), (mode, first, n)
    # MEAN's division on load is the read-out's: sum / float32(count), a count of 1 the bits
    v = tr.inputs(vr.MEAN, store, count, 0, F - 1)
    assert np.array_equal(bits(v), bits(vr.read_out(vr.MEAN, store, count)))


def test_the_radius_and_taps_are_the_postprocess_sections():
    from sap3d_tensorflow_amd import dataflow
    for sigma, radius in ((1.5, 0), (1.0, 0), (0.3, 0), (2.9, 0), (5.0, 24), (0.8, 1), (4.0, 15)):
        cfg = tr.parse(tr.GAUSS, sigma, radius)
        taps = dataflow.blur_taps(sigma, radius)
        assert len(taps) == 2 * cfg["r"] + 1 and np.array_equal(bits(taps), bits(cfg["w"])), (sigma, radius)
    assert tr.parse(tr.GAUSS, 1.5)["r"] == 6 and tr.parse(tr.GAUSS, 2.9)["r"] == 12


# ---- the library's host-only paths ------------------------------------------------------------------------------------------
def _hook(kind, sigma, radius, alpha, count, first, n, mode=vr.MEAN, hw=5):
    """"ok" when p3d_debug_video_temporal accepts the call (it ran, or only the HIP device is missing), else its refusal's text."""
    from sap3d_tensorflow_amd import _lib
    from sap3d_tensorflow_amd._lib import fptr
    F = len(count)
    store = np.ones((F, hw), np.float32)
    cnt = np.ascontiguousarray(count, np.int32)
    out = np.full((max(n, 1), hw), 7.0, np.float32)
    cfg = _lib.P3dVideoTemporal(kind, sigma, radius, alpha)
    rc = _lib.lib().p3d_debug_video_temporal(0, mode, C.byref(cfg), fptr(store), cnt.ctypes.data_as(C.POINTER(C.c_int32)), F, hw, first, n, 0,
                                             fptr(out))
    if rc == 0:
        return "ok"
    msg = _lib.lib().p3d_last_error().decode()
    assert np.all(out == 7.0), "a refusal left the output untouched"
    return "ok" if "temporal" not in msg and "device" in msg.lower() else msg


def _replay(kind, sigma, radius, alpha, count, first, n):
    try:
        tr.check(tr.parse(kind, sigma, radius, alpha), count, first, n)
    except tr.Refused as e:
        return str(e)
    return "ok"


def test_set_time_refusals_match_the_replay():
    nan, inf = float("nan"), float("inf")
    ones = [1] * 60
    bad = [(3, 1.0, 0, 0.0), (-1, 1.0, 0, 0.0),                                    # an unknown kind
           (tr.GAUSS, 0.0, 0, 0.0), (tr.GAUSS, -1.0, 2, 0.0), (tr.GAUSS, nan, 2, 0.0), (tr.GAUSS, inf, 2, 0.0),
           (tr.GAUSS, 1.0, -1, 0.0), (tr.GAUSS, 1.0, 25, 0.0), (tr.GAUSS, 7.0, 0, 0.0),   # sigma 7 -> r 28
           (tr.GAUSS, 0.0, 3, 0.0),                                                 # a radius without sigma
           (tr.GAUSS, 0.01, 0, 0.0),                                                # sigma -> r 0
           (tr.EMA, 0.0, 0, 1.0), (tr.EMA, 0.0, 0, -0.25), (tr.EMA, 0.0, 0, nan), (tr.EMA, 0.0, 0, inf), (tr.EMA, 0.0, 0, 1.5)]
    for kind, sigma, radius, alpha in bad:
        assert _replay(kind, sigma, radius, alpha, ones, 0, 60) != "ok", (kind, sigma, radius, alpha)
        msg = _hook(kind, sigma, radius, alpha, ones, 0, 60)
        assert msg != "ok" and "video_temporal" in msg, (kind, sigma, radius, alpha, msg)
    good = [(tr.GAUSS, 1.5, 0, 0.0), (tr.GAUSS, 6.0, 24, 0.0), (tr.GAUSS, 3.0, 0, 0.0), (tr.GAUSS, 0.1, 1, 0.0), (tr.GAUSS, 1.0, 2, nan),
            (tr.EMA, 0.0, 0, 0.0), (tr.EMA, nan, -5, 0.9375), (tr.EMA, 0.0, 0, float(np.nextafter(np.float32(1), np.float32(0))))]
    for kind, sigma, radius, alpha in good:
        assert _replay(kind, sigma, radius, alpha, ones, 0, 60) == "ok"
        assert _hook(kind, sigma, radius, alpha, ones, 0, 60) == "ok", (kind, sigma, radius, alpha)
    assert "kind" in _hook(tr.OFF, 0.0, 0, 0.0, ones, 0, 60)                        # the hook has nothing to launch when off


def test_read_out_refusals_and_the_frames_a_read_needs():
    F = 20
    # GAUSS r = 3: a read of 5 .. 11 needs 2 .. 14; EMA: 0 .. 11
    cfg_g, cfg_e = tr.parse(tr.GAUSS, 1.0, 3), tr.parse(tr.EMA, alpha=0.5)
    assert tr.needed(cfg_g, F, 5, 7) == (2, 14) and tr.needed(cfg_g, F, 0, 2) == (0, 4) and tr.needed(cfg_g, F, 18, 2) == (15, 19)
    assert tr.needed(cfg_e, F, 5, 7) == (0, 11) and tr.needed(cfg_e, F, 19, 1) == (0, 19)
    for zero in range(F):
        count = [1 + f % 3 for f in range(F)]
        count[zero] = 0
        for kind, sigma, radius, alpha, (lo, hi) in ((tr.GAUSS, 1.0, 3, 0.0, (2, 14)), (tr.EMA, 0.0, 0, 0.5, (0, 11))):
            want = "ok" if not lo <= zero <= hi else "frame %d" % zero
            assert _replay(kind, sigma, radius, alpha, count, 5, 7) == want
            for mode in (vr.NEWEST, vr.MEAN):
                got = _hook(kind, sigma, radius, alpha, count, 5, 7, mode)
                assert (got == "ok") if want == "ok" else re.search(r"frame %d\b" % zero, got), (kind, zero, mode, got)
    # the first needed frame of count 0 is the one named
    count = [1] * F
    count[3] = count[9] = 0
    assert re.search(r"frame 3\b", _hook(tr.GAUSS, 1.0, 3, 0.0, count, 5, 7))
    assert re.search(r"frame 9\b", _hook(tr.GAUSS, 1.0, 3, 0.0, count, 7, 3))
    # r > F - 1
    ones = [1] * 16
    assert _hook(tr.GAUSS, 4.0, 15, 0.0, ones, 0, 16) == "ok" and _replay(tr.GAUSS, 4.0, 15, 0.0, ones, 0, 16) == "ok"
    msg = _hook(tr.GAUSS, 4.0, 16, 0.0, ones, 0, 16)
    assert "F - 1" in msg and _replay(tr.GAUSS, 4.0, 16, 0.0, ones, 0, 16) != "ok"
    # a range outside the video
    for first, n in ((0, 0), (-1, 2), (15, 2), (0, 17)):
        assert "outside" in _hook(tr.EMA, 0.0, 0, 0.5, ones, first, n) and _replay(tr.EMA, 0.0, 0, 0.5, ones, first, n) != "ok"
    assert "mode" in _hook(tr.EMA, 0.0, 0, 0.5, ones, 0, 16, mode=2)


def test_plan_hook_keeps_lds_within_64_kb_and_needs_no_device():
    from sap3d_tensorflow_amd import P3dError, dataflow
    for r in (1, 7, 8, 15, 24):
        for hw, n in ((35, 16), (1024, 41), (112 * 112, 300), (1080 * 960, 16)):
            ppb, fpb, lds = dataflow.temporal_plan("gauss", r, hw, n)
            assert 0 < lds <= 65536 and 1 <= fpb <= n and ppb >= 64 and ppb % 4 == 0, (r, hw, n, ppb, fpb, lds)
            assert lds == (2 * r + 1) * ppb * 4                      # the ring: 2r + 1 inputs per pixel
            assert (n + fpb - 1) // fpb <= 65535
    assert dataflow.temporal_plan("gauss", 1, 1024, 41)[1] < 41      # (the GPU tests aim at this seam)
    assert dataflow.temporal_plan("gauss", 7, 4096, 41)[0] == 4 * dataflow.temporal_plan("gauss", 8, 4096, 41)[0]      # four pixels a lane up to r = 7
    ppb, fpb, lds = dataflow.temporal_plan("ema", 0, 12544, 300)
    assert ppb >= 64 and fpb == 300 and lds == 0
    assert dataflow.temporal_plan("ema", 0, 1 << 18, 16)[0] == 4 * ppb          # four elements per lane only where hw is large
    for kind, r, hw, n in (("gauss", 0, 10, 10), ("gauss", 25, 10, 10), ("gauss", 1, 0, 10), ("ema", 0, 10, 0)):
        with pytest.raises(P3dError, match="video_temporal_plan"):
            dataflow.temporal_plan(kind, r, hw, n)
    with pytest.raises(ValueError):
        dataflow.temporal_plan("off", 1, 10, 10)


def test_launch_description_counts_every_frame_a_run_loads():
    from sap3d_tensorflow_amd import dataflow
    F, hw, r = 300, 112 * 112, 24
    _, fpb, _ = dataflow.temporal_plan("gauss", r, hw, F)
    loaded = sum(min(F - 1, min(f0 + fpb, F) - 1 + r) - max(0, f0 - r) + 1 for f0 in range(0, F, fpb))
    d = dataflow.temporal_desc("gauss", F, hw, sigma=8.0, radius=r, mode="mean")
    assert d["kernel"] == "video_temporal_gauss_kernel<1>" and d["bytes"] == (loaded + F) * hw * 4.0
    assert F * hw * 8.0 < d["bytes"] <= F * hw * 4.0 * 4                  # a run's halo at most triples its loads
    assert d["flops"] == (1 + 3 * r) * F * hw
    d = dataflow.temporal_desc("ema", F, hw, first=100, n=50, alpha=0.5)
    assert d["kernel"] == "video_temporal_ema_kernel<0>" and d["bytes"] == (150 + 50) * hw * 4.0 and d["flops"] == 3 * 149 * hw


def test_header_declares_and_the_binding_binds_the_new_symbols():
    from sap3d_tensorflow_amd import _lib
    src = open(os.path.join(ROOT, "include", "p3d_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(p3d_[a-z0-9_]+)\s*\(", code))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"enum\s*\{\s*P3D_TEMPORAL_OFF = 0, P3D_TEMPORAL_GAUSS = 1, P3D_TEMPORAL_EMA = 2\s*\}", code)
    assert re.search(r"#define P3D_TEMPORAL_MAX_RADIUS 24\b", code)
    assert _lib.TEMPORAL_KINDS == {"off": tr.OFF, "gauss": tr.GAUSS, "ema": tr.EMA} and _lib.P3D_TEMPORAL_MAX_RADIUS == tr.MAX_RADIUS == 24
    assert [f[0] for f in _lib.P3dVideoTemporal._fields_] == ["kind", "sigma", "radius", "alpha"] and C.sizeof(_lib.P3dVideoTemporal) == 16


# ---- the driver -------------------------------------------------------------------------------------------------------------
def _gen_pred():
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


def test_driver_temporal_arguments(capsys):
    gp = _gen_pred()
    base = ["--videos", "v"]
    assert not gp.parse_args(base).resident and gp.parse_args(base).temporal == "off"
    a = gp.parse_args(base + ["--temporal", "gauss", "--temporal-sigma", "1.5"])
    assert a.resident and (a.temporal, a.temporal_sigma, a.temporal_radius) == ("gauss", 1.5, 0) and a.write == "npy"
    a = gp.parse_args(base + ["--temporal", "ema", "--temporal-alpha", "0.75", "--write", "jpg"])
    assert a.resident and a.temporal_alpha == 0.75
    a = gp.parse_args(base + ["--temporal", "gauss", "--temporal-sigma", "9", "--temporal-radius", "24", "--write", "png"])
    assert a.resident and a.temporal_radius == 24
    bad = [["--temporal", "gauss"], ["--temporal", "gauss", "--temporal-sigma", "-1"], ["--temporal", "gauss", "--temporal-sigma", "nan"],
           ["--temporal", "gauss", "--temporal-sigma", "2", "--temporal-radius", "25"],
           ["--temporal", "gauss", "--temporal-sigma", "2", "--temporal-radius", "-1"],
           ["--temporal", "gauss", "--temporal-sigma", "7"],                      # r 28: a radius must be given
           ["--temporal", "gauss", "--temporal-sigma", "0.01"],
           ["--temporal", "gauss", "--temporal-sigma", "2", "--temporal-alpha", "0.5"],
           ["--temporal", "ema", "--temporal-alpha", "1"], ["--temporal", "ema", "--temporal-alpha", "-0.1"],
           ["--temporal", "ema", "--temporal-alpha", "nan"], ["--temporal", "ema", "--temporal-alpha", "0.5", "--temporal-sigma", "2"],
           ["--temporal-sigma", "2"], ["--temporal-alpha", "0.5"], ["--temporal", "median"]]
    for extra in bad:
        with pytest.raises(SystemExit) as e:
            gp.parse_args(base + extra)
        assert e.value.code == 2, extra
        assert "temporal" in capsys.readouterr().err, extra
