"""Fixation priors on the GPU (csrc/prior.hip through the C ABI), held bit for bit to the numpy replay of include/p3d_hip.h
(tests/prior_ref.py, itself held to plain numpy by tests/test_prior_cpu.py): the counts on every path of the launch (bytes only,
words with a head and a tail, map slices that meet in integer atomics, the real geometry), the finish, the apply stage alone and
inside the shared chain, the evaluation pass with the prior as a stage and as the information-gain baseline, the session, the
refusals.  Tolerance 0 wherever the law is the reference; the five metric columns at their existing gates, IG at
tests/kl_ig_ref.py's 1e-9."""
import numpy as np
import pytest

import hist_match_ref as href
import kl_ig_ref as K
import postprocess_ref as pref
import prior_ref as P

pytestmark = pytest.mark.gpu

CFG = dict(base=16, blocks=(2, 2, 3))


def _exact(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bits = np.uint64 if got.dtype == np.float64 else np.uint32 if got.dtype == np.float32 else got.dtype
    bad = np.argwhere(got.view(bits) != want.view(bits))
    assert bad.size == 0, (what, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


# ---- count ---------------------------------------------------------------------------------------------------------------
COUNT_CASES = [(1, 1, 1, 0), (3, 5, 7, 0), (3, 5, 7, 1)] + [(5, 16, 16, off) for off in range(4)] + [(300, 3, 5, 0), (300, 3, 5, 3)]


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("n,H,W,off", COUNT_CASES, ids=["%dx%dx%d+%d" % c for c in COUNT_CASES])
def test_counts_are_the_integer_sums_however_the_work_is_cut(kind, n, H, W, off):
    from sap3d_tensorflow_amd import dataflow as gdf
    maps = P.edge_maps(np.random.default_rng(n * 100 + H), n, H, W)
    want, _ = P.count(maps, kind)
    got, flag = gdf.prior_count(maps, kind, offset=off)
    assert not flag
    _exact(got, want, "one call")
    # the maps split over three calls (fewer where there are fewer maps), each on the words the last one left
    cuts = sorted({0, n // 3, (2 * n) // 3 + (1 if n > 1 else 0), n})
    acc = None
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        acc, flag = gdf.prior_count(maps[lo:hi], kind, counts=acc, offset=off)
        assert not flag
    _exact(acc, want, "split over %d calls" % (len(cuts) - 1))
    # + then - restores the previous words exactly, whatever they were
    before = np.random.default_rng(5).integers(0, 2 ** 32 - 255 * n, size=(H, W), dtype=np.uint32)
    up, flag = gdf.prior_count(maps, kind, counts=before, offset=off)
    assert not flag
    _exact(up, P.count(maps, kind, counts=before)[0], "on top of earlier counts")
    down, flag = gdf.prior_count(maps, kind, sign=-1, counts=up, offset=off)
    assert not flag
    _exact(down, before, "+ then -")


def test_counts_at_the_real_geometry():
    from sap3d_tensorflow_amd import dataflow as gdf
    maps = P.edge_maps(np.random.default_rng(8), 4, 1080, 960)
    for kind in P.KINDS:
        got, flag = gdf.prior_count(maps, kind)
        assert not flag
        _exact(got, P.count(maps, kind)[0], kind)


@pytest.mark.parametrize("n,H,W", [(2, 16, 16), (3, 5, 7), (300, 3, 5)], ids=["words", "bytes", "slices"])
def test_a_subtraction_below_zero_raises_the_flag_and_nothing_faults(n, H, W):
    from sap3d_tensorflow_amd import dataflow as gdf
    maps = P.edge_maps(np.random.default_rng(9), n, H, W)
    have, _ = P.count(maps, "bytes")
    short = have.copy()
    short[H // 2, W // 2] -= 1                                   # one pixel holds one less than is taken out
    assert maps[:, H // 2, W // 2].any()
    got, flag = gdf.prior_count(maps, "bytes", sign=-1, counts=short)
    want, wflag = P.count(maps, "bytes", sign=-1, counts=short)
    assert flag and wflag
    _exact(got, want, "the words wrap modulo 2^32")
    got, flag = gdf.prior_count(maps, "bytes", sign=-1, counts=have)
    assert not flag and not got.any()                            # exactly to zero is no underflow


# ---- finish --------------------------------------------------------------------------------------------------------------
def _session(batch, **kw):
    from sap3d_tensorflow_amd import P3DSession
    return P3DSession("unet", batch=batch, seed=0, **dict(CFG, **kw))


@pytest.fixture(scope="module")
def sess():
    s = _session(2, height=48, width=48)
    yield s
    s.close()


@pytest.mark.parametrize("H,W,sigma,radius", [(24, 20, 1.0, 2), (40, 33, 1.5, 0)], ids=["24x20 r2", "40x33 sigma1.5"])
def test_finish_is_the_blur_and_max_replay_on_the_float_counts(sess, H, W, sigma, radius):
    from sap3d_tensorflow_amd import dataflow as gdf
    rng = np.random.default_rng(H)
    maps = (rng.random((37, H, W)) < 0.08).astype(np.uint8) * 255
    sess.open_prior((H, W), "fixations")
    assert sess.prior_info() == dict(size=(H, W), kind="fixations", n_maps=0)
    sess.prior_add(maps[:20])
    sess.prior_add(maps[20:])
    counts, n_maps = sess.prior_counts()
    assert n_maps == 37
    _exact(counts, P.count(maps, "fixations")[0], "the handle's counts")
    got = sess.finish_prior(sigma, radius)
    want = P.finish(counts, gdf.blur_taps(sigma, radius))
    _exact(got, want, "finish")
    _exact(sess.prior_map, want, "the resident prior")
    assert got.max() == 1.0
    _exact(gdf.fixation_prior(maps, "fixations", sigma, radius), want, "dataflow.fixation_prior")
    # leave-one-out: four maps out, the prior of the rest, the maps back in
    sess.prior_add(maps[3:7], -1)
    _exact(sess.finish_prior(sigma, radius), P.finish(P.count(np.delete(maps, slice(3, 7), axis=0), "fixations")[0], gdf.blur_taps(sigma, radius)),
           "leave four out")
    sess.prior_add(maps[3:7], 1)
    _exact(sess.prior_counts()[0], counts, "back in")
    # bytes: densities
    dens = rng.integers(0, 256, size=(5, H, W), dtype=np.uint8)
    sess.open_prior((H, W), "bytes")
    sess.prior_add(dens)
    _exact(sess.finish_prior(sigma, radius), P.finish(P.count(dens, "bytes")[0], gdf.blur_taps(sigma, radius)), "bytes")
    sess.close_prior()
    assert sess.prior_map is not None                             # the finished prior stays


def test_finish_and_readout_refusals(sess):
    import ctypes as C
    from sap3d_tensorflow_amd import P3dError, lib
    H, W = 12, 9
    sess.set_prior_map(None)
    sess.close_prior()
    for call in (lambda: sess.finish_prior(1.0, 1), lambda: sess.prior_add(np.zeros((1, H, W), np.uint8)), sess.prior_counts):
        with pytest.raises(P3dError, match="no accumulator"):
            call()
    assert lib().p3d_prior_open(sess._h, H, W, 2) != 0 and b"kind" in lib().p3d_last_error()
    sess.open_prior((H, W), "bytes")
    with pytest.raises(P3dError, match="holds no maps"):
        sess.finish_prior(1.0, 1)
    sess.prior_add(np.zeros((2, H, W), np.uint8))
    with pytest.raises(P3dError, match="every count is zero"):
        sess.finish_prior(1.0, 1)
    assert sess.prior_map is None                                 # a refusal leaves no prior behind
    one = np.zeros((1, H, W), np.uint8)
    one[0, 2, 3] = 200
    sess.prior_add(one)
    with pytest.raises(P3dError, match="radius"):
        sess.finish_prior(1.0, 9)                                 # r > min(H, W) - 1
    with pytest.raises(P3dError, match="sigma"):
        sess.finish_prior(-1.0, 0)
    with pytest.raises(P3dError, match="cannot leave"):
        sess.prior_add(np.zeros((4, H, W), np.uint8), -1)         # more maps than are in: refused on the host
    assert sess.prior_info()["n_maps"] == 3
    assert lib().p3d_prior_add(sess._h, one.ctypes.data_as(C.POINTER(C.c_ubyte)), P.MAX_MAPS + 1, 1) != 0      # refused before any launch
    assert b"P3D_PRIOR_MAX_MAPS" in lib().p3d_last_error()
    good = sess.finish_prior(1.0, 1)
    # a map that was never added goes out: the flag, then finish and read-out refuse with a text, and the process carries on
    other = np.zeros((1, H, W), np.uint8)
    other[0, 5, 5] = 9
    sess.prior_add(other, -1)
    for call in (lambda: sess.finish_prior(1.0, 1), sess.prior_counts):
        with pytest.raises(P3dError, match="below zero"):
            call()
    _exact(sess.prior_map, good, "the prior of before the underflow is still the handle's")
    sess.open_prior((H, W), "bytes")                              # a fresh accumulator clears the flag
    sess.prior_add(one)
    _exact(sess.finish_prior(1.0, 1), P.finish(P.count(one, "bytes")[0], pref.taps(1.0, 1)), "after reopening")
    sess.close_prior()
    sess.set_prior_map(None)


# ---- apply ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("n,H,W", [(3, 5, 7), (2, 16, 16), (2, 100, 97)], ids=["3x5x7", "2x16x16", "2x100x97"])
def test_apply_is_the_float32_law_at_every_alignment(mode, n, H, W):
    from sap3d_tensorflow_amd import dataflow as gdf
    rng = np.random.default_rng(H + n)
    v = rng.normal(0.3, 0.4, (n, H, W)).astype(np.float32)
    g = rng.random((H, W)).astype(np.float32)
    g[0, 0], g[-1, -1] = 0.0, 1.0
    for a in (0.0, 0.25, 1.0):
        want = P.apply(v, g, mode, a)
        for off in (0, 1, 2, 3, 5, 10, 12):                       # the maps at 0 .. 3; 5, 10: the prior alike (16 bytes per lane); 12: not
            _exact(gdf.apply_prior(v, g, mode, a, offset=off), want, (mode, a, off))
    _exact(gdf.apply_prior(v, g, "mul", 0.0), v * g, "MUL at a = 0 is v g")
    _exact(gdf.apply_prior(v, g, "mix", 0.0), v, "MIX at a = 0 is v")


# ---- the chain -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_case():
    """2 maps at 8x8 (channel 0 of 3) -> 24x20, a prior at 24x20, a 16-entry target table."""
    from oracle.dataflow import resize_linear
    rng = np.random.default_rng(31)
    src = rng.normal(0.3, 0.4, (2, 8, 8, 3)).astype(np.float32)
    full = np.stack([resize_linear(m, 24, 20) for m in np.ascontiguousarray(src[..., 0])]).astype(np.float32)
    fixs = (rng.random((11, 24, 20)) < 0.1).astype(np.uint8) * 255
    prior = P.finish(P.count(fixs, "fixations")[0], pref.taps(1.5, 2))
    cdf, centre, _ = href.cumulative_distribution(href.values("skewed", (16, 16), np.random.default_rng(9)), 16)
    return dict(src=src, full=full, prior=prior, table=(cdf, centre))


@pytest.mark.parametrize("mode,a", [("mul", 0.25), ("mix", 0.5)])
def test_stage_in_the_postprocess_chain(chain_case, mode, a):
    from sap3d_tensorflow_amd import dataflow as gdf
    c = chain_case
    size, sigma, r, nb = (24, 20), 1.0, 2, 32
    blurred = pref.blur(c["full"], gdf.blur_taps(sigma, r))
    staged = P.apply(blurred, c["prior"], mode, a)
    want = pref.normalise(href.match_table(staged, c["table"][0], c["table"][1], nb), "range")
    kw = dict(sigma=sigma, radius=r, norm="range", hist_match=c["table"], nbins=nb)
    _exact(gdf.postprocess_maps(c["src"], size, prior=c["prior"], prior_mode=mode, prior_weight=a, **kw), want, "blur + PRIOR + MATCH + range")
    _exact(gdf.postprocess_maps(c["src"], size, scale=255.0, prior=c["prior"], prior_mode=mode, prior_weight=a, **kw), pref.quantise(want, 255.0),
           "... + bytes")
    _exact(gdf.postprocess_maps(c["src"], size, prior=c["prior"], prior_mode=mode, prior_weight=a), P.apply(c["full"], c["prior"], mode, a),
           "PRIOR alone, after the float32 resize")
    # the stage off: bit for bit what p3d_postprocess_maps_match returns, floats and bytes
    for scale in (None, 255.0):
        _exact(gdf.postprocess_maps(c["src"], size, scale=scale, prior=c["prior"], prior_mode="off", **kw), gdf.postprocess_maps(c["src"], size, scale=scale, **kw),
               ("off", scale))


def test_chain_refusals(chain_case):
    from sap3d_tensorflow_amd import P3dError
    from sap3d_tensorflow_amd import dataflow as gdf
    import ctypes as C
    from sap3d_tensorflow_amd import _lib, lib
    c = chain_case
    flat = np.ones((24, 20), np.float32)
    bad = c["prior"].copy()
    bad[1, 1] = np.nan
    for g, word in ((flat, "constant"), (bad, "finite")):
        with pytest.raises(P3dError, match=word):
            gdf.postprocess_maps(c["src"], (24, 20), prior=g, prior_mode="mul", prior_weight=0.5)
    fp = C.POINTER(C.c_float)
    m = np.ascontiguousarray(c["full"])
    out = np.empty_like(m)
    for mode, a in ((3, 0.5), (1, 1.5), (2, -0.25), (1, float("nan"))):
        assert lib().p3d_debug_prior_apply(0, mode, a, m.ctypes.data_as(fp), 2, 24, 20, c["prior"].ctypes.data_as(fp), 0, out.ctypes.data_as(fp)) != 0
        assert b"prior_stage" in lib().p3d_last_error()


# ---- evaluation ----------------------------------------------------------------------------------------------------------
def test_evaluation_scores_the_staged_map_and_takes_the_prior_as_baseline(chain_case):
    import eval_maps_ref as R
    from oracle import evaluation as oev
    from sap3d_tensorflow_amd import dataflow as gdf
    from sap3d_tensorflow_amd import metrics as gm
    from test_gpu_eval import _check
    c = chain_case
    size, sigma, r, mode, a = (24, 20), 1.0, 2, "mul", 0.25
    rng = np.random.default_rng(4)
    spread = np.stack([(f - f.min()) / (f.max() - f.min()) for f in c["full"]])
    dens = np.stack([R._density(rng, f) for f in spread])
    fix = np.stack([R._fixation(rng, f, k) for f, k in zip(spread, (40, 25))])
    maps = np.ascontiguousarray(c["src"])
    post = dict(sigma=sigma, radius=r, norm="none")
    opts = dict(size=size, n_rep=5, postprocess=post)
    five, x = gm.evaluate_maps(maps, dens, fix, rng=np.random.RandomState(11), extra=("kldiv", "info_gain"), baseline="prior", prior=c["prior"],
                               prior_mode=mode, prior_weight=a, **opts)
    scored = P.apply(pref.blur(c["full"], gdf.blur_taps(sigma, r)), c["prior"], mode, a)
    rs = np.random.RandomState(11)
    for b in range(2):
        with np.errstate(all="ignore"):
            want = oev.test_py_clip_metrics(scored[b], dens[b], fix[b], n_rep=5, rng=rs)      # the float64 oracle of test.py's loop body
        print(b, five[b], want)
        _check(five[b], want)
        ig = K.info_gain(scored[b], K.fixated_bytes(fix[b]), c["prior"])
        print("IG", x[b, 1], ig)
        assert np.isfinite(ig) and x[b, 1] == pytest.approx(ig, rel=K.GPU_GATE, abs=0)
    # the prior copied on the device scores what the same map uploaded as a baseline scores: the same bits
    five2, x2 = gm.evaluate_maps(maps, dens, fix, rng=np.random.RandomState(11), extra=("kldiv", "info_gain"), baseline=c["prior"], prior=c["prior"],
                                 prior_mode=mode, prior_weight=a, **opts)
    _exact(x2, x, "device copy against upload")
    _exact(five2, five, "the five columns")
    # the five columns are the ones of the hook on the replay's scored map, at any extra setting
    plain = gm.evaluate_maps(scored, dens, fix, size=size, n_rep=5, rng=np.random.RandomState(11))
    _exact(five, plain, "the five columns against the bare hook on the scored map")
    # stage off and no extras: the hook returns what p3d_debug_eval_maps_post returns
    off, xoff = gm.evaluate_maps(maps, dens, fix, rng=np.random.RandomState(11), prior=c["prior"], prior_mode="off", **opts)
    _exact(off, gm.evaluate_maps(maps, dens, fix, rng=np.random.RandomState(11), **opts), "off")
    assert np.isnan(xoff).all()


def test_session_prior_as_stage_and_baseline_and_off_means_untouched(sess):
    from sap3d_tensorflow_amd import P3dError, synthetic
    from sap3d_tensorflow_amd import metrics as gm
    size = (90, 80)
    s = sess
    x = np.random.default_rng(3).normal(0.0, 0.5, s.x_shape).astype(np.float32)
    _, dens, fix = synthetic.synthetic_test_set(2, 2, size=size, density_size=(45, 40))
    sched = s.schedule()
    plain = s.evaluate(x, dens, fix, size=size, n_rep=5, rng=np.random.RandomState(11))
    pred = s.activation("pred")[:, -1, :, :, 0]
    _exact(plain, gm.evaluate_maps(pred, dens, fix, size=size, n_rep=5, rng=np.random.RandomState(11)), "evaluate, everything off")
    with pytest.raises(P3dError, match="no prior"):
        s.set_prior_stage("mul", 0.5)
    with pytest.raises(P3dError, match="no prior"):
        s.set_eval_extra(baseline="prior")
    assert s.prior_stage is None and s.eval_extra is None
    # a prior from other fixation maps, on the device
    others = (np.random.default_rng(6).random((9,) + size) < 0.02).astype(np.uint8) * 255
    s.open_prior(size)
    s.prior_add(others)
    prior = s.finish_prior(3.0)
    # ... as the baseline: the same IG as the map read back and handed to p3d_set_eval_extra
    s.set_eval_extra(kldiv=True, baseline="prior")
    now = s.eval_extra
    assert now["kldiv"] and now["info_gain"]
    _exact(now["baseline"], prior, "the baseline is the prior")
    _exact(s.evaluate(x, dens, fix, size=size, n_rep=5, rng=np.random.RandomState(11)), plain, "evaluate returns what it returned")
    e_dev = s.last_eval_extra()
    s.set_eval_extra(kldiv=True, info_gain=True, baseline=s.prior_map)
    s.evaluate(x, dens, fix, size=size, n_rep=5, rng=np.random.RandomState(11))
    e_host = s.last_eval_extra()
    print(e_dev.tolist())
    _exact(e_dev, e_host, "baseline='prior' against p3d_set_eval_extra with prior_map()")
    assert np.isfinite(e_dev).all()
    s.set_eval_extra(False)
    # ... as the stage: evaluate, the byte writer, and the hook on the same maps agree bit for bit
    s.set_prior_stage("mix", 0.25)
    assert s.prior_stage == dict(mode="mix", weight=0.25)
    got = s.evaluate(x, dens, fix, size=size, n_rep=5, rng=np.random.RandomState(11))
    hook, _ = gm.evaluate_maps(pred, dens, fix, size=size, n_rep=5, rng=np.random.RandomState(11), prior=prior, prior_mode="mix", prior_weight=0.25)
    _exact(got, hook, "evaluate under the stage")
    assert not np.array_equal(got, plain)
    from sap3d_tensorflow_amd import dataflow as gdf
    win = s.predict_windows(x)[..., 0]
    first = [15, 14]
    maps = np.concatenate([win[b, f:] for b, f in enumerate(first)])
    want = pref.quantise(P.apply(gdf.resize_linear(maps, size), prior, "mix", 0.25), 255.0)
    _exact(s.pred_maps_u8(first, size=size), want, "pred_maps_u8 under the stage (postprocess off: the float32-resize chain)")
    with pytest.raises(P3dError, match="prior is 90 x 80"):
        s.pred_maps_u8(first, size=(45, 40))                      # a prior of another size than the stage's
    for mode, a, word in (("mul", 1.5, "weight"), ("mix", -0.5, "weight")):
        with pytest.raises(ValueError, match=word):
            s.set_prior_stage(mode, a)
    assert s.prior_stage == dict(mode="mix", weight=0.25)
    # off again: the same bits as before anything was set, and training never saw any of it
    s.set_prior_stage("off")
    _exact(s.pred_maps_u8(first, size=size), gdf.resize_linear_u8(maps, size), "pred_maps_u8, off again")
    _exact(s.evaluate(x, dens, fix, size=size, n_rep=5, rng=np.random.RandomState(11)), plain, "evaluate, off again")
    s.set_prior_stage("mul", 0.5)
    assert s.schedule() == sched                                  # the train step's launches, stage on
    s.set_prior_stage("off")
    s.close_prior()
    s.set_prior_map(None)
    assert s.prior_map is None
