"""The read-out hooks are ladders: every p3d_debug_eval_maps* symbol is a superset of the one before it, and so is every
p3d_postprocess_maps* symbol.  Called through the library directly, a rung with its added arguments off / NULL returns the bits
of the rung below it, the two richest evaluation rungs agree with everything on, the postprocess rungs agree across a chunk
boundary and equal the numpy replay, and a chunk boundary inside a run of the handle's prediction writes the bytes
dataflow.postprocess_maps writes."""
import ctypes as C

import numpy as np
import pytest

import hist_match_ref as href
import postprocess_ref as pref
import prior_ref as P

pytestmark = pytest.mark.gpu

FP, DP, IP, U8, U32 = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_int, C.c_ubyte, C.c_uint32))
SIZE = (9, 11)
SENTINEL = -12345.0
RUNGS = ("", "_post", "_match", "_extra", "_prior", "_shuffled")


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


@pytest.fixture(scope="module")
def case():
    """2 maps of 5x7 as channel 0 of [2, 5, 7, 3]; density [2, 6, 8]; fixation [2, 9, 11] with 4 and 0 fixated pixels; the draws
    of one evaluation with n_rep = 3 and jitter; a pool of 3 fixation maps with M = 1 and its ranks."""
    from sap3d_tensorflow_amd import dataflow as gdf
    from sap3d_tensorflow_amd import metrics as gm
    rng = np.random.default_rng(21)
    H, W = SIZE
    maps = rng.normal(0.3, 0.4, (2, 5, 7, 3)).astype(np.float32)
    dens = rng.integers(0, 256, (2, 6, 8)).astype(np.uint8)
    fix = np.zeros((2, H, W), np.uint8)
    fix[0].reshape(-1)[[5, 40, 41, 98]] = 255
    n_fix, jit, idx = gm.eval_draws(fix, True, 3, np.random.RandomState(7))
    assert list(n_fix) == [4, 0]
    pool = (rng.random((3, H, W)) < 0.2).astype(np.uint8) * 255
    ids = np.array([[1], [2]], np.int32)
    n_other = gdf.union_fixations(gdf.pack_fixations(pool), SIZE, ids)[2]
    assert n_other.min() >= 4
    ranks, n_rows = gm.shuffled_draws(n_fix, n_other, 2, np.random.RandomState(8))
    base = (rng.random((H, W)) + 0.1).astype(np.float32)
    fixs = (rng.random((11, H, W)) < 0.1).astype(np.uint8) * 255
    prior = P.finish(P.count(fixs, "fixations")[0], pref.taps(1.5, 2))
    return dict(maps=maps, dens=dens, fix=fix, n_fix=n_fix, jit=jit, idx=idx, pool=pool, ids=ids, ranks=ranks, n_rows=n_rows, base=base,
                prior=prior)


def _eval(c, rung, cfg=None, mc=None, flags=0, base=None, prior=None, mode=0, a=0.0):
    """One rung of the evaluation ladder on the case's inputs -> (out [2, 5], xout [2, 2] that started as SENTINEL)."""
    from sap3d_tensorflow_amd import lib
    m, dens, fix = c["maps"], c["dens"], c["fix"]
    out = np.full((2, 5), SENTINEL, np.float64)
    xout = np.full((2, 2), SENTINEL, np.float64)
    args = (0, _ptr(m, FP), 2, 5, 7, 3, _ptr(dens, U8), 6, 8, _ptr(fix, U8), SIZE[0], SIZE[1], _ptr(c["jit"], DP), _ptr(c["idx"], IP),
            _ptr(c["n_fix"], IP), 3, 0.1, _ptr(out, DP))
    level = RUNGS.index(rung)
    if level >= 1:
        args += (C.byref(cfg) if cfg is not None else None,)
    if level >= 2:
        args += (C.byref(mc) if mc is not None else None,)
    if level >= 3:
        args += (flags, _ptr(base, FP), _ptr(xout, DP))
    if level >= 4:
        args += (_ptr(prior, FP), mode, a)
    if level == 5:
        got_other, per_rep = np.empty(2, np.uint32), np.empty((2, 2), np.float64)
        args += (_ptr(c["pool"], U8), 3, _ptr(c["ids"], IP), 1, _ptr(c["ranks"], IP), _ptr(c["n_rows"], IP), 2, 0.1, _ptr(got_other, U32),
                 _ptr(per_rep, DP))
    rc = getattr(lib(), "p3d_debug_eval_maps" + rung)(*args)
    assert rc == 0, (rung, lib().p3d_last_error())
    return out, xout


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want, equal_nan=True), (what, got, want)


def test_eval_rungs_with_everything_off_return_the_bare_hooks_bits(case):
    want, _ = _eval(case, "")
    assert not (want == SENTINEL).any()
    for rung in RUNGS[1:]:
        out, xout = _eval(case, rung)
        _same(out, want, rung)
        assert (xout == SENTINEL).all(), rung           # flags == 0: the extras' output is not written


def test_eval_rungs_with_everything_on_agree(case):
    from sap3d_tensorflow_amd import _lib
    cfg = _lib.P3dPostprocess(1.0, 2, _lib.NORMS["range"])
    mc = _lib.P3dHistMatch(_lib.MATCH_MODES["density"], 16, 0, None, None)
    both = _lib.EVAL_EXTRA["kldiv"] | _lib.EVAL_EXTRA["info_gain"]
    on = dict(cfg=cfg, mc=mc, flags=both, base=case["base"])
    mix = dict(prior=case["prior"], mode=_lib.PRIOR_MODES["mix"], a=0.25)
    out_p, x_p = _eval(case, "_prior", **on, **mix)
    out_s, x_s = _eval(case, "_shuffled", **on, **mix)
    _same(out_s, out_p, "out: _shuffled against _prior")
    _same(x_s, x_p, "xout: _shuffled against _prior")
    assert not (x_p == SENTINEL).any()
    out_x, x_x = _eval(case, "_extra", **on)
    out_o, x_o = _eval(case, "_prior", prior=case["prior"], mode=_lib.PRIOR_MODES["off"], **on)
    _same(out_x, out_o, "out: _extra against _prior with the stage off")
    _same(x_x, x_o, "xout: _extra against _prior with the stage off")
    assert not np.array_equal(out_p[0], out_o[0])       # the stage did something


@pytest.fixture(scope="module")
def post_case():
    """17 maps of 5x7 -> 9x11: one more than P3D_POST_CHUNK, so the second chunk starts inside the one run."""
    from oracle.dataflow import resize_linear
    rng = np.random.default_rng(22)
    src = rng.normal(0.3, 0.4, (17, 5, 7)).astype(np.float32)
    full = np.stack([resize_linear(m, SIZE[0], SIZE[1]) for m in src]).astype(np.float32)
    cdf, centre, _ = href.cumulative_distribution(href.values("skewed", (16, 16), np.random.default_rng(9)), 16)
    return dict(src=src, full=full, table=(np.ascontiguousarray(cdf, np.float64), np.ascontiguousarray(centre, np.float64)))


def _post(src, rung, cfg, scale, mc=None, prior=None, mode=0, a=0.0):
    from sap3d_tensorflow_amd import lib
    n = src.shape[0]
    out = np.empty((n,) + SIZE, np.float32 if scale is None else np.uint8)
    args = (0, _ptr(src, FP), n, src.shape[1], src.shape[2], 1, SIZE[0], SIZE[1], C.byref(cfg))
    if rung != "":
        args += (C.byref(mc) if mc is not None else None,)
    if rung == "_prior":
        args += (_ptr(prior, FP), mode, a)
    args += (0.0 if scale is None else scale, _ptr(out, FP) if scale is None else None, _ptr(out, U8) if scale is not None else None)
    rc = getattr(lib(), "p3d_postprocess_maps" + rung)(*args)
    assert rc == 0, (rung, lib().p3d_last_error())
    return out


@pytest.mark.parametrize("scale", [None, 255.0], ids=["f32", "u8"])
def test_postprocess_rungs_agree_and_equal_the_replay(case, post_case, scale):
    from sap3d_tensorflow_amd import _lib
    from sap3d_tensorflow_amd import dataflow as gdf
    src, sigma, r, nb, a = post_case["src"], 1.0, 2, 32, 0.25
    cfg = _lib.P3dPostprocess(sigma, r, _lib.NORMS["range"])
    want = _post(src, "", cfg, scale)
    _same(_post(src, "_match", cfg, scale), want, "_match, stage off")
    _same(_post(src, "_prior", cfg, scale), want, "_prior, stages off")
    blurred = pref.blur(post_case["full"], gdf.blur_taps(sigma, r))
    plain = pref.normalise(blurred, "range")
    _same(want, plain if scale is None else pref.quantise(plain, scale), "the bare chain against the replay")
    cdf, centre = post_case["table"]
    mc = _lib.P3dHistMatch(_lib.MATCH_MODES["table"], nb, cdf.size, _ptr(cdf, DP), _ptr(centre, DP))
    got = _post(src, "_prior", cfg, scale, mc=mc, prior=case["prior"], mode=_lib.PRIOR_MODES["mul"], a=a)
    staged = P.apply(blurred, case["prior"], "mul", a)
    replay = pref.normalise(href.match_table(staged, cdf, centre, nb), "range")
    _same(got, replay if scale is None else pref.quantise(replay, scale), "blur + PRIOR + MATCH + range against the replay")


def test_a_chunk_boundary_inside_a_run_of_the_prediction():
    """first_frame = [3, 0] on 16 frames: runs of 13 and 16 maps, so the chunk boundary at map 16 falls inside the second run."""
    from sap3d_tensorflow_amd import P3DSession
    from sap3d_tensorflow_amd import dataflow as gdf
    s = P3DSession("unet", batch=2, seed=4, base=16, blocks=(1, 1, 2))
    x = np.random.default_rng(3).normal(0.0, 0.5, s.x_shape).astype(np.float32)
    pred = s.predict_windows(x)[..., 0]
    first, size, scale = [3, 0], (37, 53), 255.0
    maps = np.concatenate([pred[b, f:] for b, f in enumerate(first)])
    assert len(maps) == 13 + 16
    s.set_postprocess(2.0, 0, "range")
    got = s.pred_maps_u8(first, size=size, scale=scale)
    s.close()
    _same(got, gdf.postprocess_maps(maps, size, 2.0, 0, "range", scale=scale), "pred_maps_u8 against postprocess_maps")
