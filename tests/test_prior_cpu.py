"""No-GPU checks of the fixation priors: what the replay (tests/prior_ref.py) claims, against plain numpy; the boundary (symbols,
signatures, the launcher's plan, which is host only); the Python-side refusals and the drivers' argument checks."""
import importlib.util
import os

import numpy as np
import pytest

import postprocess_ref as pref
import prior_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("p3d_prior_open", "p3d_prior_add", "p3d_prior_counts", "p3d_prior_info", "p3d_prior_finish", "p3d_prior_close",
               "p3d_prior_last_ms", "p3d_set_prior_map", "p3d_get_prior_map", "p3d_set_prior_stage", "p3d_get_prior_stage",
               "p3d_set_eval_extra_prior", "p3d_debug_prior_count", "p3d_debug_prior_count_plan", "p3d_debug_prior_apply",
               "p3d_postprocess_maps_prior", "p3d_debug_eval_maps_prior")


def _driver(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "drivers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 7), (300, 3, 5)])
def test_count_replay_is_plain_integer_arithmetic(shape):
    fix = P.edge_maps(np.random.default_rng(1), *shape)
    c, flag = P.count(fix, "fixations")
    assert not flag and c.dtype == np.uint32 and np.array_equal(c, (fix >= 128).sum(0))
    c, flag = P.count(fix, "bytes")
    assert not flag and np.array_equal(c.astype(np.uint64), fix.astype(np.uint64).sum(0))
    # any split into calls, and + then -, leave the same words
    a, _ = P.count(fix[:1], "bytes")
    a, _ = P.count(fix[1:], "bytes", counts=a) if shape[0] > 1 else (a, False)
    assert np.array_equal(a, c)
    back, flag = P.count(fix, "bytes", sign=-1, counts=c)
    assert not flag and not back.any()
    # one map too many taken out: the flag, and words that wrapped
    extra = np.full((1,) + shape[1:], 255, np.uint8)
    under, flag = P.count(np.concatenate([fix, extra]), "bytes", sign=-1, counts=c)
    assert flag and (under == np.uint32(2 ** 32 - 255)).all()


def test_finish_replay_is_the_postprocess_replay():
    rng = np.random.default_rng(2)
    counts = rng.integers(0, 40, size=(24, 20)).astype(np.uint32)
    for sigma, r in ((1.0, 2), (1.5, 0)):
        taps = pref.taps(sigma, pref.radius(sigma, r))
        got = P.finish(counts, taps)
        want = pref.postprocess(counts.astype(np.float32)[None], taps, "max")[0]
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert got.max() == 1.0 and got.min() >= 0.0
    # no blur: count / max
    got = P.finish(counts, np.zeros(0, np.float32))
    assert np.array_equal(got, counts.astype(np.float32) / np.float32(counts.max()))
    # the conversion rounds to nearest even above 2^24
    big = np.array([[2 ** 24 + 1, 2 ** 24 + 3, 2 ** 32 - 1]], np.uint32)
    assert (big.astype(np.float32) == np.array([[2.0 ** 24, 2.0 ** 24 + 4, 2.0 ** 32]], np.float32)).all()


def test_apply_replay_at_the_ends_of_the_weight():
    rng = np.random.default_rng(3)
    v = rng.normal(0.3, 0.4, (2, 5, 7)).astype(np.float32)
    g = rng.random((5, 7)).astype(np.float32)
    assert np.array_equal(P.apply(v, g, "mul", 0.0), v * g)                    # a = 0: b = 1, fmul(1, g) = g, fadd(g, 0) = g
    assert np.array_equal(P.apply(v, g, "mix", 0.0), v)                        # 1 * v + 0 * g
    assert np.array_equal(P.apply(v, g, "mul", 1.0), v)                        # v * (0 * g + 1)
    assert np.array_equal(P.apply(v, g, "mix", 1.0), np.broadcast_to(g, v.shape))
    quarter = P.apply(v, g, "mul", 0.25)
    assert quarter.dtype == np.float32 and np.array_equal(quarter, v * (np.float32(0.75) * g + np.float32(0.25)))
    with pytest.raises(ValueError):
        P.apply(v, g, "add", 0.5)


def test_symbols_are_declared_exported_and_bound():
    from sap3d_tensorflow_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "p3d_hip.h")).read()
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n + "(" in hdr and hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert "P3D_PRIOR_MAX_MAPS 16000000" in hdr and _lib.P3D_PRIOR_MAX_MAPS == P.MAX_MAPS
    kern = open(os.path.join(ROOT, "sap3d_tensorflow_amd", "csrc", "p3d_kernels.h")).read()
    assert "POST_BLUR_V = 2, POST_PRIOR = 3, POST_MATCH = 4" in kern


def test_the_launchers_plan_takes_each_path_where_the_tests_expect_it():
    """Host only: the cut of the count launch (p3d_debug_prior_count_plan).  tests/test_gpu_prior.py's shapes were chosen for
    these paths."""
    from sap3d_tensorflow_amd import P3dError
    from sap3d_tensorflow_amd import dataflow as gdf
    assert gdf.prior_count_plan(1, 1, 1) == (0, 1, 1)
    assert gdf.prior_count_plan(3, 5, 7) == (0, 35, 1)                         # H W % 4 != 0: bytes only
    assert gdf.prior_count_plan(5, 16, 16, 0) == (64, 0, 1)                    # words only
    for off in (1, 2, 3):
        assert gdf.prior_count_plan(5, 16, 16, off) == (63, 4, 1)              # a head of 4 - off, a tail of off
    words, singles, slices = gdf.prior_count_plan(300, 3, 5)
    assert (words, singles) == (0, 15) and slices > 1                          # many maps on a tiny grid: sliced
    words, singles, slices = gdf.prior_count_plan(4, 1080, 960)
    assert (words, singles, slices) == (1080 * 960 // 4, 0, 1)
    words, singles, slices = gdf.prior_count_plan(100000, 112, 112)
    assert (words, singles) == (3136, 0) and 13 * slices >= 1024
    for bad in ((0, 4, 4), (P.MAX_MAPS + 1, 4, 4), (1, 0, 4)):
        with pytest.raises(P3dError):
            gdf.prior_count_plan(*bad)


def test_python_side_refusals_need_no_device():
    from sap3d_tensorflow_amd import dataflow as gdf
    from sap3d_tensorflow_amd import metrics as gm
    u8 = np.zeros((2, 4, 4), np.uint8)
    f32 = np.zeros((2, 4, 4), np.float32)
    with pytest.raises(ValueError, match="uint8"):
        gdf.prior_count(f32)
    with pytest.raises(ValueError, match="kind"):
        gdf.prior_count(u8, kind="density")
    with pytest.raises(ValueError, match="counts"):
        gdf.prior_count(u8, counts=np.zeros((4, 5), np.uint32))
    with pytest.raises(ValueError, match="prior is"):
        gdf.apply_prior(f32, np.zeros((4, 5), np.float32))
    with pytest.raises(ValueError, match="mode"):
        gdf.apply_prior(f32, f32[0], mode="add")
    with pytest.raises(ValueError, match="mode"):
        gdf.apply_prior(f32, f32[0], mode="off")
    for a in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="weight"):
            gdf.apply_prior(f32, f32[0], mode="mix", a=a)
    with pytest.raises(ValueError, match="prior is"):
        gdf.postprocess_maps(f32, (4, 4), prior=np.zeros((3, 4), np.float32), prior_mode="mul")
    with pytest.raises(ValueError, match="prior is"):
        gm.evaluate_maps(f32, u8, u8, prior=np.zeros((3, 4), np.float32), prior_mode="mul")
    with pytest.raises(ValueError, match="baseline"):
        gm.evaluate_maps(f32, u8, u8, prior=np.ones((4, 4), np.float32), extra="info_gain", baseline="centre")


def test_driver_argument_checks():
    t = _driver("test")
    ok = t.parse_args(["--info-gain", "prior", "--prior-sigma", "32", "--prior-leave-out", "--prior", "mul", "--prior-weight", "0.25"])
    assert t.prior_plan(ok) == dict(source="set", leave_out=True, sigma=32.0, radius=0, mode="mul", weight=0.25, baseline="prior")
    assert t.prior_plan(t.parse_args([])) is None
    assert t.prior_plan(t.parse_args(["--info-gain", "base.npy"])) is None      # a file baseline: as before
    other = t.prior_plan(t.parse_args(["--prior-from", "train.npz", "--prior", "mix", "--prior-weight", "1"]))
    assert other["source"] == "train.npz" and other["baseline"] is None and other["mode"] == "mix"
    for argv, word in ((["--prior", "mul", "--prior-weight", "1.5"], "weight"), (["--prior-weight", "0.5"], "--prior"),
                       (["--prior-leave-out"], "--info-gain prior"), (["--info-gain", "prior", "--prior-from", "o.npz", "--prior-leave-out"], "own"),
                       (["--info-gain", "prior", "--prior-sigma", "-1"], "sigma"), (["--prior-sigma", "3"], "prior")):
        with pytest.raises(SystemExit, match=word):
            t.prior_plan(t.parse_args(argv))
    g = _driver("gen_pred")
    a = g.parse_args(["--videos", "v", "--prior", "p.npy", "--prior-mode", "mix", "--prior-weight", "0.5", "--write", "png", "--resident"])
    assert g.prior_stage_args(a) == ("p.npy", "mix", 0.5)
    assert g.prior_stage_args(g.parse_args(["--videos", "v"])) is None
    for argv, word in ((["--prior-mode", "mix"], "--prior FILE"), (["--prior", "p.npy", "--prior-weight", "2", "--write", "jpg"], "weight"),
                       (["--prior", "p.npy"], "png")):
        with pytest.raises(SystemExit, match=word):
            g.prior_stage_args(g.parse_args(["--videos", "v"] + argv))
