"""The non-finite contract (include/p3d_hip.h, "Non-finite values") without a GPU: the oracle's max-pool obeys item 3, the
helpers of nonfinite_ref.py do what the GPU tests rely on, and the motivation is kept runnable -- one NaN pixel in one clip
makes the oracle's training loss NaN, while the same step with relu = fmax (what the kernels' fmaxf ReLU computed) gives a
finite loss and a finite prediction, i.e. a poisoned stem that nothing reports."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nonfinite_ref as nf          # noqa: E402
from oracle import nn, p3d          # noqa: E402
from test_gpu_ops import POOL_CASES  # noqa: E402

NAN = np.nan


def pool(x, k, s, dy=None, pins=None):
    t = nn.Tape()
    if pins is not None:
        t.pins = pins
    X = nn.Var(np.asarray(x, np.float64))
    Y = nn.max_pool3d(t, X, k, s)
    if dy is None:
        return Y.data, None
    Y.grad = np.asarray(dy, np.float64)
    t.ops[-1]()
    return Y.data, X.grad


# ---- oracle.nn.max_pool3d, item 3 ----------------------------------------------------------------------------------------------
def test_pool_all_nan_window_gives_nan_and_routes_to_its_first_tap():
    x = np.arange(1.0, 9.0).reshape(1, 4, 2, 1, 1)
    x[0, 2:4] = NAN                                        # the second (2,1,1) window of a k = s = (2,2,1) pool over D, H
    dy = np.array([3.0, 5.0]).reshape(1, 2, 1, 1, 1)
    y, dx = pool(x, (2, 2, 1), (2, 2, 1), dy)
    assert y[0, 0, 0, 0, 0] == 4.0 and np.isnan(y[0, 1, 0, 0, 0])           # (the old pool gave -inf here)
    want = np.zeros_like(x)
    want[0, 1, 1] = 3.0                                    # the maximum of the clean window
    want[0, 2, 0] = 5.0                                    # the first NaN tap of the poisoned one
    assert np.array_equal(dx, want)


@pytest.mark.parametrize("tap", [0, 3, 8])                 # first, middle and last tap of a 1x3x3 window
def test_pool_one_nan_among_finite_taps(tap):
    rng = np.random.default_rng(tap)
    x = rng.standard_normal((1, 1, 3, 3, 2))
    x[0, 0, tap // 3, tap % 3, 1] = NAN                    # channel 1 only
    y, dx = pool(x, (1, 3, 3), (1, 3, 3), np.full((1, 1, 1, 1, 2), 2.0))
    assert y[0, 0, 0, 0, 0] == x[..., 0].max() and np.isnan(y[0, 0, 0, 0, 1])
    want = np.zeros_like(x)
    want[..., 0][x[..., 0] == x[..., 0].max()] = 2.0
    want[0, 0, tap // 3, tap % 3, 1] = 2.0
    assert np.array_equal(dx, want)


def test_pool_two_nans_route_to_the_first_in_scan_order():
    x = np.zeros((1, 2, 2, 2, 1))
    x[0, 0, 1, 1, 0] = NAN
    x[0, 1, 0, 0, 0] = NAN
    _, dx = pool(x, (2, 2, 2), (2, 2, 2), np.ones((1, 1, 1, 1, 1)))
    want = np.zeros_like(x)
    want[0, 0, 1, 1, 0] = 1.0                              # tap 3 comes before tap 4
    assert np.array_equal(dx, want)


def test_pool_nan_in_a_padded_border_window():
    """(1,3,7,9) under k (2,3,3), s 2: SAME pads one cell after D and W and one before / after H.  A NaN in the last cell is seen
    by the one border window that holds it, whose other taps are padding or finite."""
    xs, k, s = POOL_CASES[2]
    rng = np.random.default_rng(0)
    x = rng.standard_normal(xs)
    x[0, 2, 6, 8, :] = NAN
    y, dx = pool(x, k, s, np.ones((1, 2, 4, 5, xs[4])))
    want = np.zeros(y.shape, bool)
    want[0, 1, 3, 4, :] = True
    assert np.array_equal(np.isnan(y), want)
    assert np.all(dx[0, 2, 6, 8, :] == 1.0)
    yr, dxr = nf.max_pool_ref(x, k, s, np.ones(y.shape))
    assert np.array_equal(y, yr, equal_nan=True) and np.array_equal(dx, dxr)


@pytest.mark.parametrize("xs,k,s", POOL_CASES)
def test_pool_ref_from_the_definition_agrees_with_the_oracle(xs, k, s):
    """nonfinite_ref.max_pool_ref (per-window argmax) and the oracle's tap loop agree on clean post-ReLU input (tied zeros) and on
    input holding NaN, -inf and +inf; finite input gives the oracle the bits it gave before the NaN rule."""
    rng = np.random.default_rng(5)
    x = np.maximum(rng.standard_normal(xs), 0)
    xp, _ = nf.plant(rng, x, [np.nan, np.nan, -np.inf, np.inf], max(4, x.size // 40))
    for a in (x, xp):
        dy = rng.standard_normal(nf.max_pool_ref(a, k, s)[0].shape)
        y, dx = pool(a, k, s, dy)
        yr, dxr = nf.max_pool_ref(a, k, s, dy)
        assert np.array_equal(y, yr, equal_nan=True)
        assert np.abs(dx - dxr).max() <= 1e-12       # (overlapping windows add in another order)
    assert np.isnan(pool(xp, k, s)[0]).any()


def test_pool_pinned_branch_follows_the_same_rule():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((1, 2, 4, 4, 3))
    x[0, 1, 2, 3, 1] = NAN
    dy = rng.standard_normal((1, 1, 2, 2, 3))
    free = pool(x, (2, 2, 2), (2, 2, 2), dy)
    t = nn.Tape()
    t.pins = {"pool": [np.nan_to_num(x, nan=50.0).astype(np.float32)], "pool_tol": np.inf}     # the pin's arg-max is that tap too
    t.pin_log = {"pool": 0, "pool_flips": 0}
    X = nn.Var(x)
    Y = nn.max_pool3d(t, X, (2, 2, 2), (2, 2, 2))
    Y.grad = dy
    t.ops[-1]()
    assert np.array_equal(Y.data, free[0], equal_nan=True) and np.array_equal(X.grad, free[1])
    assert t.pin_log["pool_flips"] == 0


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def test_plant_and_footprint_helpers():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((5, 7)).astype(np.float32)
    b, pos = nf.plant(rng, a, [nf.NAN, nf.PINF, nf.NINF], 6)
    assert len(set(pos.tolist())) == 6 and np.isfinite(a).all()
    assert (~np.isfinite(b)).sum() == 6 and np.array_equal(np.flatnonzero(~np.isfinite(b)), np.sort(pos))
    fin = nf.footprint_equal(b, b.astype(np.float64))
    assert fin.sum() == a.size - 6
    nf.clean_bits_equal(b, a, fin)
    for wrong in (a, np.where(np.isposinf(b), np.nan, b), np.where(np.isneginf(b), np.inf, b)):
        if not np.array_equal(np.isnan(wrong), np.isnan(b)) or not np.array_equal(np.isposinf(wrong), np.isposinf(b)):
            with pytest.raises(AssertionError):
                nf.footprint_equal(wrong, b)
    c = a.copy()
    c[0, 0] = -c[0, 0]
    with pytest.raises(AssertionError):
        nf.clean_bits_equal(c, a, fin | True)
    with pytest.raises(AssertionError):                      # -0.f and +0.f are different bits
        nf.clean_bits_equal(np.float32([-0.0]), np.float32([0.0]), np.array([True]))


def test_cbam_ref_poisons_only_the_sample_that_holds_the_nan():
    rng = np.random.default_rng(1)
    N, C = 2, 16
    x = np.maximum(rng.standard_normal((N, 2, 4, 4, C)), 0)
    p = [0.3 * rng.standard_normal(s) for s in ((C, C // 8), (C // 8,), (C // 8, C), (C,), (7, 7, 7, 2, 1))]
    clean = nf.cbam_forward_ref(x, *p)
    x[0, 1, 2, 3, 5] = NAN
    cs, sp, ss = nf.cbam_forward_ref(x, *p)
    assert np.isnan(cs[0]).all() and np.isnan(sp[0]).all() and np.isnan(ss[0]).all()     # the MLP mixes every channel
    for a, b in zip((cs, sp, ss), clean):
        assert np.array_equal(a[1], b[1])


# ---- the motivation: what one NaN pixel does to a step -----------------------------------------------------------------------------
CFG = p3d.NetConfig(base=8, blocks=(1, 1, 1))
SHAPE = (2, 16, 32, 32)


def poisoned_batch():
    x = p3d.synthetic_clip(0, SHAPE + (3,)).copy()
    y = p3d.synthetic_target(3, SHAPE)
    x[0, 3, 5, 7, 1] = NAN                                   # one pixel of clip 0
    return x, y


def test_one_nan_pixel_makes_the_oracles_training_step_nan():
    x, y = poisoned_batch()
    params = p3d.init_params(1, "unet", CFG)
    with np.errstate(all="ignore"):
        loss, pred, grads, _ = p3d.loss_and_grads(dict(params), x, y, 0.0, True, "unet", CFG)
    assert np.isnan(loss) and np.isnan(pred).all()           # batch statistics couple the clips
    # every pre-activation is NaN, so every ReLU gate is closed (a select, item 4): the BatchNorm betas receive sums of zeros,
    # and every other gradient is NaN through the statistics sums (dgamma = sum(0 * NaN)) or the loss
    finite = sorted(n for n, g in grads.items() if np.isfinite(g).all())
    assert finite == sorted(n for n in grads if n.endswith("/beta")) and len(finite) == 19 and len(grads) == 70
    assert all(not grads[n].any() for n in finite)


def test_an_fmax_relu_launders_the_same_step(monkeypatch):
    """relu = fmax is what `fmaxf(v, 0.f)` computes: the NaN reaches the stem's batch statistics, every stem output is NaN, the
    ReLU turns them into zeros, and the loss and the prediction come out finite -- only the stem's own gradients show it."""
    x, y = poisoned_batch()
    params = p3d.init_params(1, "unet", CFG)
    fake = type(np)("numpy_with_fmax_relu")
    fake.__dict__.update(np.__dict__)
    fake.maximum = np.fmax
    monkeypatch.setattr(nn, "np", fake)
    with np.errstate(all="ignore"):
        loss, pred, grads, _ = p3d.loss_and_grads(dict(params), x, y, 0.0, True, "unet", CFG)
    assert np.isfinite(loss) and np.isfinite(pred).all()
    bad = sorted(n for n, g in grads.items() if not np.isfinite(g).all())
    assert bad == ["batch_normalization/gamma", "firstconv1"]


def test_in_inference_the_nan_stays_in_its_clip_up_to_the_backbone():
    """With training=False the stem's BatchNorm uses its moving statistics, so the NaN stays inside clip 0's receptive field through
    the stem conv, its BatchNorm + ReLU and pool1 (which the old `v > best` pool silently dropped: both clips' pred came out
    finite).  The backbone blocks keep batch statistics whatever `training` says (make_block, as the reference builds them), so
    from block0 on both clips are NaN, and so is every pred element: the issue's expectation that the clean clip stays clean in
    inference holds for the stem only on this network, and for the whole GroupNorm network."""
    x, y = poisoned_batch()
    params = p3d.init_params(1, "unet", CFG)
    with np.errstate(all="ignore"):
        pred, g = p3d.forward(dict(params), x, 0.0, False, "unet", CFG)
    for name in ("conv1_custom", "conv1_custom_bn_relu", "pool1"):
        d = g.tape.taps[name].data
        assert np.isnan(d[0]).any() and not np.isnan(d[0]).all() and np.isfinite(d[1]).all(), name
    assert np.isnan(g.tape.taps["block0/conv1_bn_relu"].data).all()
    assert np.isnan(np.asarray(pred)).all()
