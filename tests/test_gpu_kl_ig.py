"""KL divergence and information gain on the GPU (full_pass_kl / full_stats3 of csrc/metrics_full.hip through the C ABI) against
the numpy replay of include/p3d_hip.h (tests/kl_ig_ref.py, held to the two formulas by tests/test_kl_ig_cpu.py) at relative
1e-9 -- the project's full-resolution gate for CC and NSS (tests/test_gpu_eval.py); tests/test_kl_ig_cpu.py shows on these very
inputs that the order of the sums stays under 1e-11.  Exact where the law is exact: NaN placement, the zeros, reruns, and the five
existing columns with the option off, half on and on."""
import numpy as np
import pytest

import hist_match_ref as href
import kl_ig_ref as K
import postprocess_ref as pref

pytestmark = pytest.mark.gpu

CFG = dict(base=16, blocks=(2, 2, 3))
BOTH = ("kldiv", "info_gain")
SEED = 21


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), (what, a, b)


def _close(got, want, nan, what):
    """NaN exactly where `nan` says, the rest at relative 1e-9."""
    print(what)
    print("  got ", np.asarray(got).tolist())
    print("  want", np.asarray(want).tolist())
    assert np.array_equal(np.isnan(got), nan), (what, got)
    assert np.array_equal(np.isnan(want), nan), (what, want)
    ok = ~nan
    assert np.asarray(got)[ok] == pytest.approx(np.asarray(want)[ok], rel=K.GPU_GATE, abs=0), (what, got, want)


def _run(c, extra=BOTH, baseline="case", density=None, maps=slice(None), **kw):
    from sap3d_tensorflow_amd import metrics as gm
    base = c["baseline"] if isinstance(baseline, str) else baseline
    dens = c["density"] if density is None else density
    args = (c["maps"][maps], dens[maps], c["fixation"][maps])
    opts = dict(jitter=True, n_rep=5, rng=np.random.RandomState(SEED), **kw)
    if extra is None:
        return gm.evaluate_maps(*args, **opts)
    return gm.evaluate_maps(*args, extra=extra, baseline=base if "info_gain" in extra else None, **opts)


@pytest.mark.parametrize("elem_stride", [1, 3])
@pytest.mark.parametrize("k", range(len(K.SHAPES)), ids=["%dx%d" % s[1] for s in K.SHAPES])
def test_chain_matches_the_replay_and_leaves_the_five_columns_alone(k, elem_stride):
    c = K.case(k, elem_stride)
    five, x = _run(c)
    assert five.shape == (4, 5) and x.shape == (4, 2)
    _close(x, K.replay(K.case(k)), K.expected_nan(), "KL, IG of %s, elem_stride %d" % (K.SHAPES[k], elem_stride))
    five2, x2 = _run(c)
    _same(x, x2, "a second call")
    off = _run(c, extra=None)
    five_kl, x_kl = _run(c, extra="kldiv")
    five_ig, x_ig = _run(c, extra=("info_gain",))
    for name, f in (("both", five), ("both again", five2), ("KL only", five_kl), ("IG only", five_ig)):
        _same(off, f, "the five columns, " + name)
    _same(x_kl[:, 0], x[:, 0], "KL alone")
    _same(x_ig[:, 1], x[:, 1], "IG alone")
    assert np.isnan(x_kl[:, 1]).all() and np.isnan(x_ig[:, 0]).all()          # a metric that is off reports NaN


@pytest.mark.parametrize("k", range(len(K.SHAPES)), ids=["%dx%d" % s[1] for s in K.SHAPES])
def test_exact_zeros(k):
    c = K.case(k)
    # an all-zero density: q = 0 everywhere, every term 0 * log(eps) = -0
    _, x = _run(c, density=np.zeros_like(c["density"]))
    print(x.tolist())
    assert (x[[K.ORDINARY, K.NO_FIX, K.CONSTANT], 0] == 0.0).all() and np.isnan(x[K.HAS_NAN, 0])
    # the prediction as its own baseline: P_i and B_i are the same doubles (pass A's sums of the map, full_stats3's of the baseline)
    _, x = _run(c, baseline=c["full"][K.ORDINARY])
    print(x.tolist())
    assert x[K.ORDINARY, 1] == 0.0
    with np.errstate(all="ignore"):
        want = K.info_gain(c["full"][K.CONSTANT], K.fixated_bytes(c["fixation"][K.CONSTANT]), c["full"][K.ORDINARY])
    assert np.isnan(want) and np.isnan(x[K.CONSTANT, 1]) and np.isnan(x[K.NO_FIX, 1])


def test_extras_score_the_postprocessed_map():
    from sap3d_tensorflow_amd import dataflow as gdf
    c = K.case(1)
    keep = [K.ORDINARY, K.NO_FIX]                                                # (maps that hold NaN are not pinned by MATCH)
    post, nb = dict(sigma=1.5, radius=0, norm="range"), 64
    five, x = _run(c, maps=keep, postprocess=post, hist_match="density", nbins=nb)
    dens_f64 = c["dens_bytes"][keep] / 255.0
    maps = pref.blur(c["full"][keep], gdf.blur_taps(post["sigma"]))
    maps = href.match_hist_maps(maps, dens_f64, nb)
    maps = pref.normalise(maps, post["norm"])
    sub = dict(dens_bytes=c["dens_bytes"][keep], fixation=c["fixation"][keep], baseline=c["baseline"])
    want = K.replay(sub, full=maps)
    _close(x, want, K.expected_nan()[keep], "blur + match + range")
    bare = K.replay(K.case(1))[keep]
    assert abs(want[0, 0] - bare[0, 0]) > 1e-3 * abs(bare[0, 0])                 # the stages moved the numbers
    _same(five, _run(c, extra=None, maps=keep, postprocess=post, hist_match="density", nbins=nb), "the five columns")


@pytest.mark.parametrize("k", range(len(K.SHAPES)), ids=["%dx%d" % s[1] for s in K.SHAPES])
def test_op_level_entry_points(k):
    from sap3d_tensorflow_amd import dataflow as gdf
    from sap3d_tensorflow_amd import metrics as gm
    c = K.case(k)
    (h, w), (H, W) = K.SHAPES[k]
    keep = [K.ORDINARY, K.NO_FIX, K.CONSTANT]
    # bytes 0 / 255 at the scored size: the uint8 resize is a copy and byte / 255. is exact in float32 -- the chain's own numbers
    dens = np.where(c["dens_bytes"] >= 128, 255, 0).astype(np.uint8)
    _, x = _run(c, density=dens, maps=keep)
    full = gdf.resize_linear(np.ascontiguousarray(c["maps"][keep]), (H, W))
    assert np.array_equal(full, c["full"][keep])
    dmap = np.stack([gdf.mapf_density(d[None], (H, W))[0] for d in dens[keep]])
    assert set(np.unique(dmap).tolist()) <= {0.0, 1.0}
    fmap = (c["fixation"][keep] >= 128).astype(np.float32)
    kl = gm.KLdiv_batch(full, dmap)
    ig = gm.InfoGain_batch(full, fmap, c["baseline"])
    print(x.tolist(), kl.tolist(), ig.tolist())
    _same(kl, x[:, 0], "KLdiv_batch against the chain")
    _same(ig, x[:, 1], "InfoGain_batch against the chain")
    assert gm.KLdiv(full[0], dmap[0]) == kl[0] and gm.InfoGain(full[0], fmap[0], c["baseline"]) == ig[0]
    # any float32 density: the law takes it widened to double
    q = K.density_f32(c["dens_bytes"][keep])
    with np.errstate(all="ignore"):
        want = np.array([K.kldiv(full[b], q[b].astype(np.float64)) for b in range(3)])
    _close(gm.KLdiv_batch(full, q), want, np.zeros(3, bool), "KLdiv_batch on float32 densities")
    # a constant that is not zero, a NaN, no fixation
    flat = np.full((H, W), 0.25, np.float32)
    with np.errstate(all="ignore"):
        assert gm.KLdiv(flat, q[0]) == pytest.approx(K.kldiv(flat, q[0].astype(np.float64)), rel=K.GPU_GATE, abs=0)
    assert np.isnan(gm.InfoGain(flat, fmap[0], c["baseline"]))
    assert np.isnan(gm.KLdiv(c["full"][K.HAS_NAN], q[0])) and np.isnan(gm.InfoGain(c["full"][K.HAS_NAN], fmap[0], c["baseline"]))
    assert np.isnan(gm.InfoGain(full[0], np.zeros_like(fmap[0]), c["baseline"]))
    assert gm.KLdiv(full[0], np.zeros_like(q[0])) == 0.0
    assert gm.InfoGain(full[0], fmap[0], full[0]) == 0.0
    with pytest.raises(ValueError):
        gm.InfoGain(full[0], fmap[0], c["baseline"][:, :-1])


def _session(batch):
    from sap3d_tensorflow_amd import P3DSession
    return P3DSession("unet", batch=batch, seed=0, **CFG)


def test_session_keeps_the_last_evaluations_extras():
    from sap3d_tensorflow_amd import P3dError, synthetic
    from sap3d_tensorflow_amd import metrics as gm
    size = (1080, 960)
    x, dens, fix = synthetic.synthetic_test_set(2, 3, size=size, density_size=(270, 480))       # clip 2 has no fixation
    s = _session(3)
    assert s.eval_extra is None
    with pytest.raises(P3dError, match="off"):
        s.last_eval_extra()
    plain = s.evaluate(x, dens, fix, rng=np.random.RandomState(11))
    base = K.prior(*size)
    s.set_eval_extra(kldiv=True, info_gain=True, baseline=base)
    now = s.eval_extra
    assert now["kldiv"] and now["info_gain"] and np.array_equal(now["baseline"], base)
    with pytest.raises(P3dError, match="no evaluation"):
        s.last_eval_extra()                                                     # the evaluation above ran before the option went on
    got = s.evaluate(x, dens, fix, rng=np.random.RandomState(11))
    _same(got, plain, "evaluate returns what it returned")
    e = s.last_eval_extra()
    pred = s.activation("pred")[:, -1, :, :, 0]
    five, hook = gm.evaluate_maps(pred, dens, fix, rng=np.random.RandomState(11), extra=BOTH, baseline=base)
    print(e.tolist())
    _same(e, hook, "last_eval_extra against evaluate_maps on the session's own last frames")
    _same(five, plain, "the hook's five columns")
    assert np.isfinite(e[:2]).all() and np.isfinite(e[2, 0]) and np.isnan(e[2, 1])
    # an evaluation at another size than the baseline's: its five columns come back, the extras are refused
    xs, ds, fs = synthetic.synthetic_test_set(2, 3, size=(90, 80), density_size=(45, 40))
    small = s.evaluate(xs, ds, fs, size=(90, 80), rng=np.random.RandomState(11))
    with pytest.raises(P3dError, match="baseline"):
        s.last_eval_extra()
    s.set_eval_extra(kldiv=True)                                                # KL alone needs no baseline, at any size
    assert s.eval_extra == dict(kldiv=True, info_gain=False, baseline=None)
    _same(s.evaluate(xs, ds, fs, size=(90, 80), rng=np.random.RandomState(11)), small, "the five columns at 90x80")
    e = s.last_eval_extra()
    assert np.isfinite(e[:, 0]).all() and np.isnan(e[:, 1]).all()
    s.set_eval_extra(False)
    assert s.eval_extra is None
    with pytest.raises(P3dError, match="off"):
        s.last_eval_extra()
    s.close()


def test_refusals_leave_the_setting_alone():
    from sap3d_tensorflow_amd import P3dError, lib
    s = _session(2)
    base = K.prior(9, 11)
    s.set_eval_extra(kldiv=False, info_gain=True, baseline=base)
    bad = base.copy(); bad[3, 3] = np.inf
    for kw, word in ((dict(kldiv=True, info_gain=True), "needs a baseline"), (dict(kldiv=True, baseline=base), "without"),
                     (dict(info_gain=True, baseline=bad), "finite"), (dict(info_gain=True, baseline=np.ones_like(base)), "constant")):
        with pytest.raises(P3dError, match=word):
            s.set_eval_extra(**kw)
        now = s.eval_extra
        assert not now["kldiv"] and now["info_gain"] and np.array_equal(now["baseline"], base)
    assert lib().p3d_set_eval_extra(s._h, 4, None, 0, 0) != 0 and b"flags" in lib().p3d_last_error()
    s.close()
