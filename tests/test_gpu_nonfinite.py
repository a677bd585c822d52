"""The non-finite contract of include/p3d_hip.h ("Non-finite values"), kernel by kernel through the hooks of
sap3d_tensorflow_amd/ops.py, then on whole graphs.

Every case plants NaN / +inf / -inf / -0 into otherwise ordinary operands and asks three things of the result:
  1. footprint: it is NaN, +inf and -inf exactly where the float64 reference of the same operation is
     (nonfinite_ref.footprint_equal; the references are the existing *_ref.py modules and oracle.nn, which propagate);
  2. the finite elements meet the tolerance the hook's own test file uses for it;
  3. where the operation couples nothing across the poisoned element -- other channels under BatchNorm, other (sample, group)
     slabs under GroupNorm, other samples under CBAM, other batches / rows under attention, other maps in the per-map losses, other
     elements in the optimisers, positions outside a conv's receptive field -- the result has the BITS of the clean launch.
Outputs are prefilled with NaN by the hooks, so a store that is skipped fails item 1 as well.

The normalise / ReLU passes draw their operands as tests/test_gpu_bn.py and tests/test_gpu_gn.py do (every ReLU argument kept
away from zero) instead of N(0,1): a ReLU decision that differs between float32 and float64 would move a whole gradient element
and, through the statistics sums, its channel -- that is those files' reason, and it is independent of where the specials go.

On the kernels as they were before this contract (fmaxf ReLUs, `v > best` pools) 380 of the 715 cases here fail: test_bn_pass
200 and test_gn_pass 102 + 2 (z finite where the reference is NaN; a channel holding +inf normalised to zeros), test_max_pool
23, test_cbam 4, test_fused_relu_forward 32, test_fused_filter_gradient 4, the four whole-graph cases (finite loss), and three
findings outside the ReLUs and pools: test_elementwise_losses 6 (Smooth-L1 / L1 on a raw head: sign(NaN) came out 0) and, with
the ReLU fixed, bn_small's moving mean of a channel holding +inf (NaN where the unshifted sums of the other paths and the
reference give +inf).  A third finding is documented, not fixed: see test_head.

Two expectations of the issue that the references corrected: select gates (item 4) make the oracle's ReLU backward a where(), so
with every gate closed the BatchNorm betas' gradients are zeros, not NaN; and `unet++ds` and `gn_p3d_decoder` run at base 16,
the smallest their attention blocks / decoder head take (base 8 is refused)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attention_ref as ar                  # noqa: E402
import conv_launch_ref as cref              # noqa: E402
import fused_bn_ref as fref                 # noqa: E402
import map_loss_ref                         # noqa: E402
import nonfinite_ref as nf                  # noqa: E402
from oracle import nn, p3d                  # noqa: E402
from test_gpu_bn import bn_inputs, bn_oracle                         # noqa: E402
from test_gpu_conv_launch import TILE_NAMES, TOL, forced, out_shape  # noqa: E402
from test_gpu_gn import cbam_inputs, cbam_oracle, gn_inputs, gn_oracle, small_ok     # noqa: E402
from test_gpu_ops import POOL_CASES         # noqa: E402

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
EPS32 = float(np.finfo(np.float32).eps)
NAN, INF = np.float32(np.nan), np.float32(np.inf)
NORM_SPECIALS = ["nan", "+inf", "-inf", "-0"]


def ops():
    from sap3d_tensorflow_amd import ops as o
    return o


def rnd(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(f32)


def check(got, want, what, tol=None, scale=None, clean=None, region=None):
    """Items 1-3 of the docstring for one output.  region: where item 3 holds (default: wherever the reference is finite)."""
    fin = nf.footprint_equal(got, want, what)
    if tol is not None:
        sc = scale if scale is not None else max(float(np.abs(np.asarray(want, f64)[fin]).max()) if fin.any() else 0.0, 1e-30)
        nf.close_where(np.asarray(got), np.asarray(want, f64), fin, tol, sc, what)
    if clean is not None:
        nf.clean_bits_equal(got, clean, fin if region is None else (np.broadcast_to(region, fin.shape) & fin), what)
    return fin


def cols(C, *poisoned):
    m = np.ones(C, bool)
    m[list(poisoned)] = False
    return m


# ---- BatchNorm normalise / ReLU / add passes ---------------------------------------------------------------------------------------
# path 1 (bn_small.hip) takes M <= 1024, path 2 (fold-apply) C % 64 == 0 and M >= 1024, path 3 (finalize + apply) everything
BN_SHAPES = [(50, 16, 1), (50, 64, 1), (50, 16, 3), (50, 64, 3), (1500, 64, 2), (1500, 16, 3), (1500, 64, 3), (9000, 64, 2),
             (9000, 16, 3), (9000, 64, 3)]


def bn_run(mode, y1, y2, params, moving, dz, batch, path):
    z, dy1, dy2, grads, mv, info = ops().bn_pass(mode, y1, y2, params, moving, dz, batch=(batch, batch), path=path)
    assert info[0] == path
    return dict(z=z, dy1=dy1, dy2=dy2, grads=grads, mv=mv)


@pytest.mark.parametrize("special", NORM_SPECIALS)
@pytest.mark.parametrize("batch", [1, 0])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("M,C,path", BN_SHAPES)
def test_bn_pass(M, C, path, mode, batch, special):
    """One special in channel ca of y1 and (modes 1-4) one in channel cb of y2; with +inf under batch statistics also a channel
    cc of y1 that holds nothing but +inf (its mean is +inf, every x - mean is NaN).  Batch statistics: the poisoned channels are
    NaN in z and in the moving statistics as the reference has them, every other channel has the clean launch's bits in z, dy1,
    dy2, the parameter gradients and the moving statistics.  Moving statistics: only the element is touched."""
    rng = np.random.default_rng([M, C, path, mode, batch, NORM_SPECIALS.index(special)])
    y1, y2 = bn_inputs(rng, M, C, mode)
    bns = 2 if mode in (2, 3) else 1
    params = np.stack([np.stack([rng.uniform(0.5, 1.5, C), rng.uniform(-0.1, 0.1, C)]) for _ in range(bns)]).astype(f32)
    if batch:
        moving = np.array([[rng.standard_normal(C), rng.uniform(0.5, 2.0, C)] for _ in range(bns)], f32)
    else:
        moving = np.array([[y.astype(f64).mean(0), y.astype(f64).var(0)] for y in [y1, y2][:bns]], f32)
    dz = rnd(rng, (M, C))
    clean = bn_run(mode, y1, y2, params, moving, dz, batch, path)
    sig2 = min(float(np.var(y.astype(f64), 0).min()) for y in [y1, y2][:bns])

    ca, cb, cc = (int(c) for c in rng.choice(C, 3, replace=False))
    v = nf.SPECIALS[special]
    p1, p2 = y1.copy(), (y2.copy() if y2 is not None else None)
    planted = np.zeros((M, C), bool)
    r1, r2 = int(rng.integers(M)), int(rng.integers(M))
    p1[r1, ca] = v
    planted[r1, ca] = True
    touched = [ca]
    if p2 is not None:
        p2[r2, cb] = v
        planted[r2, cb] = True
        touched.append(cb)
    if special == "+inf" and batch:
        p1[:, cc] = INF
        touched.append(cc)
    got = bn_run(mode, p1, p2, params, moving, dz, batch, path)
    with np.errstate(all="ignore"):
        zw, g1w, g2w, gw, mvw = bn_oracle(mode, p1, p2, params, moving, dz, (batch, batch))
    if special == "nan" and batch:
        assert np.isnan(zw[:, ca]).all() and np.isnan(mvw[0][:, ca]).all()        # what the reference says, stated once

    tol = 1e-4 + 64 * EPS32
    gis = np.abs(params[:, 0]).max() / np.sqrt(sig2 + nn.BN_EPS)
    gscale = np.abs(dz).max() * max(gis, 1.0)
    other = cols(C, *touched)
    what = "bn mode %d M %d C %d path %d batch %d %s " % (mode, M, C, path, batch, special)
    reg = other if batch else ~planted        # moving statistics: elementwise, every other element keeps its bits
    check(got["z"], zw, what + "z", tol, max(np.abs(clean["z"]).max(), 1.0), clean["z"], reg)
    check(got["dy1"], g1w, what + "dy1", tol, gscale, clean["dy1"], reg)
    if mode != 0:
        check(got["dy2"], g2w, what + "dy2", tol, gscale, clean["dy2"], reg)
    pscale = np.abs(clean["grads"]).max() + np.sqrt(M) * np.abs(dz).max() * 2.0
    check(got["grads"], gw, what + "grads", tol, pscale, clean["grads"], other)
    check(got["mv"], mvw, what + "moving", 12 * EPS32 + 1e-2 * 64 * EPS32, max(np.abs(clean["mv"]).max(), sig2), clean["mv"], other)
    if special == "-0":
        assert np.isfinite(got["z"]).all()


# ---- GroupNorm passes -----------------------------------------------------------------------------------------------------------
# path 1 (the small kernels) takes C / G % 4 == 0 and has no mode 2 (test_gn_mode2_forward); path 2 takes everything
GN_CASES = [(R, G, path, mode) for R in (49, 800) for G in (4, 32) for path in (1, 2) for mode in range(7)
            if path == 2 or (small_ok(R, 32, G) and mode != 2)]


def gn_run(mode, y1, y2, params, dz, G, cs, ss, path, drop=0.0):
    z, dy1, dy2, grads, tables, taken, pads = ops().gn_pass(mode, y1, y2, params, dz, G, cs=cs, ss=ss, path=path, drop_rate=drop,
                                                            seed=77)
    assert taken == path
    for p in pads:
        assert p is None or p.size == 0 or np.isnan(p).all()
    return dict(z=z, dy1=dy1, dy2=dy2, grads=grads, tables=tables)


@pytest.mark.parametrize("special", NORM_SPECIALS)
@pytest.mark.parametrize("R,G,path,mode", GN_CASES)
def test_gn_pass(R, G, path, mode, special):
    """N = 2, C = 32.  One special in (sample 0, group ga) of y1: that slab is NaN in z and in the four tables, the parameter
    gradients of the group's channels are NaN, and everything else -- sample 1, the other groups -- has the clean launch's bits."""
    N, C = 2, 32
    cg = C // G
    rng = np.random.default_rng([R, G, path, mode, NORM_SPECIALS.index(special)])
    y1, y2, cs, ss = gn_inputs(rng, mode, N, R, C, G, 0.0)
    gns = 2 if mode in (2, 3) else 1
    params = np.stack([np.stack([rng.uniform(0.5, 1.5, C), rng.uniform(-0.05, 0.05, C)]) for _ in range(gns)]).astype(f32)
    dz = rnd(rng, (N, R, C))
    clean = gn_run(mode, y1, y2, params, dz, G, cs, ss, path)
    ga = int(rng.integers(G))
    p1 = y1.copy()
    p1[0, rng.integers(R), ga * cg + int(rng.integers(cg))] = nf.SPECIALS[special]
    got = gn_run(mode, p1, y2, params, dz, G, cs, ss, path)
    with np.errstate(all="ignore"):
        zw, g1w, g2w, gw = gn_oracle(mode, p1, y2, params, dz, G, 1e-5, cs, ss)
    slab = np.zeros((N, 1, C), bool)
    slab[0, 0, ga * cg:(ga + 1) * cg] = True
    chans = ~slab[0, 0]
    what = "gn mode %d R %d G %d path %d %s " % (mode, R, G, path, special)
    sig2 = float(np.var(y1.astype(f64).reshape(N, R, G, -1), axis=(1, 3)).min())
    tol = 1e-4 + 64 * EPS32
    gscale = np.abs(dz).max() * max(np.abs(params[:, 0]).max() / np.sqrt(sig2 + 1e-5), 1.0)
    fin = check(got["z"], zw, what + "z", tol, max(np.abs(clean["z"]).max(), 1.0), clean["z"], ~slab)
    if special != "-0":
        assert not fin[0, :, ga * cg:(ga + 1) * cg].any() and fin[1].all(), what
        t = got["tables"][:1, :, 0, ga * cg:(ga + 1) * cg]
        assert not np.isfinite(t[:, 2]).any() and np.isnan(t[:, [0, 1, 3]]).all(), (what, "tables of the poisoned slab")
    tmask = np.ones((gns, 4, N, C), bool)
    tmask[0, :, 0, ga * cg:(ga + 1) * cg] = False
    nf.clean_bits_equal(got["tables"], clean["tables"], tmask, what + "tables")
    if mode == 2:
        return
    check(got["dy1"], g1w, what + "dy1", tol, gscale, clean["dy1"], ~slab)
    if g2w is not None:
        check(got["dy2"], g2w, what + "dy2", tol, gscale, clean["dy2"], ~slab)
    pscale = np.abs(clean["grads"]).max() + np.sqrt(N * R) * np.abs(dz).max() * 2.0
    check(got["grads"], gw, what + "grads", tol, pscale, clean["grads"], chans)


@pytest.mark.parametrize("mode", [0, 5])
@pytest.mark.parametrize("R,G", [(49, 4), (800, 32)])
def test_gn_pass_dropout_keeps_a_dropped_nan(mode, R, G):
    """drop_rate 0.5 on z (the statistics path; the small kernels have no dropout): about half of the poisoned slab is dropped, and
    NaN * 0 is NaN, so the whole slab stays NaN; the other slabs keep the clean launch's bits, zeros included."""
    N, C = 2, 32
    cg = C // G
    rng = np.random.default_rng([R, G, mode])
    y1, _, _, _ = gn_inputs(rng, mode, N, R, C, G, 0.0)
    params = np.stack([np.stack([rng.uniform(0.5, 1.5, C), rng.uniform(-0.05, 0.05, C)])]).astype(f32)
    dz = rnd(rng, (N, R, C))
    clean = gn_run(mode, y1, None, params, dz, G, None, None, 2, drop=0.5)
    assert 0.3 < (clean["z"] == 0).mean() < 0.8
    p1 = y1.copy()
    p1[1, R // 2, 0] = NAN
    got = gn_run(mode, p1, None, params, dz, G, None, None, 2, drop=0.5)
    slab = np.zeros((N, 1, C), bool)
    slab[1, 0, :cg] = True
    assert np.isnan(got["z"][1, :, :cg]).all() and np.isnan(got["dy1"][1, :, :cg]).all()
    nf.clean_bits_equal(got["z"], clean["z"], ~slab, "gn dropout z")
    nf.clean_bits_equal(got["dy1"], clean["dy1"], ~slab, "gn dropout dy1")
    assert np.isfinite(got["z"][~np.broadcast_to(slab, got["z"].shape)]).all()


# ---- max-pool ------------------------------------------------------------------------------------------------------------------
def pool_poison(kind, x, k, s, rng):
    """The planted inputs of the issue, on a copy of x."""
    x = x.copy()
    N, D, H, W, C = x.shape
    (Do, Ho, Wo), taps = nn._conv_taps(x.shape, tuple(k) + (C, C), s)
    pads = [nn.same_pads(v, kk, st)[1] for v, kk, st in zip((D, H, W), k, s)]

    def cell(o, tap):          # input cell of tap (a, b, c) of window o, or None in the padding
        i = [o[q] * s[q] - pads[q] + tap[q] for q in range(3)]
        return tuple(i) if all(0 <= i[q] < (D, H, W)[q] for q in range(3)) else None

    mid = (Do // 2, Ho // 2, Wo // 2)
    all_taps = [(a, b, c) for a in range(k[0]) for b in range(k[1]) for c in range(k[2])]
    if kind == "one":
        x, _ = nf.plant(rng, x, [NAN], 3)
    elif kind == "window":
        for t in all_taps:
            if cell(mid, t) is not None:
                x[(slice(None),) + cell(mid, t)] = NAN
    elif kind == "first_last":
        valid = [t for t in all_taps if cell(mid, t) is not None]
        x[(0,) + cell(mid, valid[0]) + (0,)] = NAN
        x[(N - 1,) + cell(mid, valid[-1]) + (C - 1,)] = NAN
    elif kind == "border":
        x[0, 0, 0, 0, :] = NAN
        x[N - 1, D - 1, H - 1, W - 1, :] = NAN
    elif kind == "neginf":
        keep = x[0, D // 2, H // 2, W // 2].copy()
        x[:] = -INF
        x[0, D // 2, H // 2, W // 2] = keep
    return x


@pytest.mark.parametrize("kind", ["one", "window", "first_last", "border", "neginf"])
@pytest.mark.parametrize("xs,k,s", POOL_CASES)
def test_max_pool(xs, k, s, kind):
    """Forward values bit for bit, and the gradient routed to the first NaN tap of a window that holds one, else to the first
    maximum (an all -inf window: its first tap inside the tensor), overwriting NaN and accumulating onto a prior -- the disjoint
    kernel (case 1), the gather fast path (cases 0, 2, 3) and the gather general loops (case 4)."""
    o = ops()
    rng = np.random.default_rng([POOL_CASES.index((xs, k, s)), len(kind)])
    x = pool_poison(kind, np.maximum(rnd(rng, xs), 0), k, s, rng)
    dy = rnd(rng, nf.max_pool_ref(x, k, s)[0].shape)
    yw, dxw = nf.max_pool_ref(x, k, s, dy.astype(f64))
    y, outside = o.max_pool3d_launch(x, k, s)
    assert np.array_equal(y, yw.astype(f32), equal_nan=True), ("pool fwd", kind)
    assert np.isnan(y).any() == (kind != "neginf")
    t = nn.Tape()                                          # the oracle and the definition agree on this input
    Y = nn.max_pool3d(t, nn.Var(x.astype(f64)), k, s)
    assert np.array_equal(Y.data, yw, equal_nan=True)
    dx, _, kernel = o.max_pool3d_grad_launch(x, k, s, dy)
    assert np.isfinite(dx).all(), ("pool bwd leaves NaN", kind, kernel)
    assert np.abs(dx - dxw).max() <= TOL * np.abs(dxw).max(), ("pool bwd", kind, kernel)
    prior = rnd(rng, xs) * 3
    dxa, _, kernel = o.max_pool3d_grad_launch(x, k, s, dy, accumulate=True, prior=prior)
    want = prior.astype(f64) + dxw
    assert np.abs(dxa - want).max() <= TOL * np.abs(want).max(), ("pool bwd +=", kind, kernel)
    untouched = dxw == 0
    nf.clean_bits_equal(dxa, prior, untouched & (prior != 0), "pool bwd += leaves the other cells")


# ---- CBAM ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunks", [0, 2])
@pytest.mark.parametrize("C", [16, 64])
def test_cbam(C, chunks):
    """One NaN in sample 0: its channel scale, spatial maps, spatial scale and input gradient are NaN as the float64 reference has
    them (the shared MLP mixes every channel, the 7x7x7 conv covers the 2x4x4 map), every parameter gradient is NaN (they sum
    over samples), and sample 1's cs, sp, ss and dx have the clean launch's bits."""
    o = ops()
    N, D, H, W = 2, 2, 4, 4
    rng = np.random.default_rng([C, chunks])
    x, p, dout = cbam_inputs(rng, N, D, H, W, C)
    run = lambda a: o.cbam(a, p["k0"], p["b0"], p["k1"], p["b1"], p["k7"], dout, chunks=chunks)
    clean = run(x)
    xp = x.copy()
    xp[0, 1, 2, 3, C // 2 + 1] = NAN
    cs, sp, ss, dx, pg, used, pad = run(xp)
    assert used == clean[5] and np.isnan(pad).all()
    with np.errstate(all="ignore"):
        csw, spw, ssw = nf.cbam_forward_ref(xp, p["k0"], p["b0"], p["k1"], p["b1"], p["k7"])
        grads, xv, _ = cbam_oracle(xp, p, dout)
    assert np.isnan(csw[0]).all() and np.isnan(ssw[0]).all() and np.isfinite(csw[1]).all()
    s1 = np.arange(N).reshape(N, *([1] * 4)) == 1
    check(cs, csw, "cbam cs", 1e-4, 1.0, clean[0], s1.reshape(N, 1))
    check(sp, spw, "cbam sp", 1e-4, None, clean[1], s1)
    check(ss, ssw, "cbam ss", 1e-4, 1.0, clean[2], s1.reshape(N, 1, 1, 1))
    check(dx, xv.grad, "cbam dx", 1e-4, None, clean[3], s1)
    for name, g in zip(("k0", "b0", "k1", "b1", "k7"), pg):
        nf.footprint_equal(g, grads[name].reshape(g.shape), "cbam d" + name)


# ---- fused operand transforms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["source", "scale"])
@pytest.mark.parametrize("splits", [0, 2])
@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("K", [40, 64])
@pytest.mark.parametrize("at", [1, 2])
def test_fused_relu_forward(at, K, tile, splits, where):
    """relu(s x + t) (+ relu(s2 x2 + t2)) between LDS and the matrix cores, 1x3x3 over (2, 4, 7, 7): a NaN in the raw source
    poisons the receptive field of that element, a NaN in the scale table every position (SAME padding pads the transformed
    operand, so the borders are decided by the taps inside the tensor -- every position has its centre tap)."""
    from sap3d_tensorflow_amd import ops as o
    sp, k, Nc = (2, 4, 7, 7), (1, 3, 3), 36
    rng = np.random.default_rng([at, K, tile, splits, where == "scale"])
    xs = sp + (K,)
    M = int(np.prod(sp))
    x = [rnd(rng, xs) for _ in range(at)]
    st = [[f32(rng.uniform(0.5, 1.5, K) * rng.choice([-1.0, 1.0], K)), rnd(rng, K)] for _ in range(at)]
    w = rnd(rng, k + (K, Nc), 0.2)
    z = np.zeros(K, f32)

    def run(x, st):
        src = [dict(y=x[q].reshape(M, K), off=0, scale=st[q][0], shift=st[q][1], mean=z, invstd=z) for q in range(at)]
        with forced(tile, splits):
            res = o.fused_conv("forward", xs, w, (1, 1, 1), np.full((M, Nc), NAN, f32), src=src)
        assert (",relu%d" % at) in res["kernels"] and TILE_NAMES[tile] + "," in res["kernels"], res["kernels"]
        return res["out"].reshape(sp + (Nc,))

    clean = run(x, st)
    xp, stp = [a.copy() for a in x], [[a.copy() for a in q] for q in st]
    q = at - 1
    if where == "source":
        xp[q][1, 2, 3, 4, K - 1] = NAN
    else:
        stp[q][0][K - 1] = NAN
    got = run(xp, stp)
    with np.errstate(all="ignore"):
        a = fref.relu_operand(xp[0], *stp[0], *((xp[1],) + tuple(stp[1]) if at == 2 else ()))
        want = fref.conv(a, w)
    fin = check(got, want, "fused relu%d %s" % (at, where), TOL, None, clean)
    assert fin.any() == (where == "source") and not fin.all()


@pytest.mark.parametrize("where", ["source", "scale"])
@pytest.mark.parametrize("xt", [1, 2])
def test_fused_filter_gradient(xt, where):
    """The same transform on the filter gradient's x operand (xt = 1 / 2), two problems in one launch: the NaN of problem 0 stays
    out of problem 1's gradient, bit for bit."""
    from sap3d_tensorflow_amd import ops as o
    sp, k, K, Nc = (2, 4, 7, 7), (1, 3, 3), 40, 36
    M = int(np.prod(sp))
    rng = np.random.default_rng([xt, where == "scale"])

    def problem():
        pr = dict(x=rnd(rng, (M, K)), offx=0, dy=rnd(rng, (M, Nc)), offdy=0, input_sizes=sp + (K,), filter_sizes=k + (K, Nc),
                  strides=(1, 1, 1), dw=rnd(rng, k + (K, Nc)), xt=xt, dyt=0,
                  xs1=f32(rng.uniform(0.5, 1.5, K)), xt1=rnd(rng, K))
        if xt == 2:
            pr.update(x2=rnd(rng, (M, K)), offx2=0, xs2=f32(rng.uniform(0.5, 1.5, K)), xt2=rnd(rng, K))
        return pr

    def want(pr):
        a = fref.relu_operand(pr["x"].reshape(sp + (K,)), pr["xs1"], pr["xt1"],
                              *((pr["x2"].reshape(sp + (K,)), pr["xs2"], pr["xt2"]) if xt == 2 else ()))
        return pr["dw"].astype(f64) + fref.conv_filter_grad(a, pr["dy"].reshape(sp + (Nc,)), k)

    prs = [problem(), problem()]
    clean, _, _, _ = o.fused_wgrad(prs)
    bad = dict(prs[0])
    if where == "source":
        bad["x"] = prs[0]["x"].copy()
        bad["x"][((1 * 4 + 2) * 7 + 3) * 7 + 3, 3] = NAN        # (1, 2, 3, 3): an interior cell, read by all nine taps
    else:
        bad["xs1"] = prs[0]["xs1"].copy()
        bad["xs1"][3] = NAN
    got, name, _, _ = o.fused_wgrad([bad, prs[1]])
    with np.errstate(all="ignore"):
        w0 = want(bad)
    fin = check(got[0][0], w0, "fused wgrad xt %d %s %s" % (xt, where, name), TOL, None, clean[0][0])
    assert np.array_equal(~fin, np.broadcast_to((np.arange(K) == 3)[:, None], fin.shape))        # input channel 3, every tap
    nf.clean_bits_equal(got[1][0], clean[1][0], np.ones(clean[1][0].shape, bool), "fused wgrad member 1")


# ---- convolutions -----------------------------------------------------------------------------------------------------------------
def conv_case(kind, xs, k, co, s, names_have=None, f16=False, ld=(None, None), offset=(0, 0), accum=False, seed=0):
    """One NaN and one +inf in the gathered operand, then one NaN in the filter's centre tap; returns the kernel names."""
    o = ops()
    rng = np.random.default_rng([seed, len(xs), xs[4], co, k[1], s[1], kind == "forward", f16, accum])
    draw = (lambda shape, sc=1.0: cref.draw16(rng, shape, sc)) if f16 else (lambda shape, sc=1.0: rnd(rng, shape, sc))
    wshape = k + ((co, xs[4]) if kind == "transpose" else (xs[4], co))
    w = draw(wshape, 0.25 if f16 else 0.1)
    if kind == "forward":
        inp, ishape, ref = draw(xs), None, lambda a, ww: cref.forward(a, ww, s, f16=f16)
    elif kind == "input_grad":
        inp, ishape, ref = draw(out_shape(xs, s, co)), xs, lambda a, ww: cref.input_grad(a, ww, s, xs, f16=f16)
    else:
        inp, ishape, ref = draw(xs), None, lambda a, ww: cref.transpose(a, ww, s)
    oshape = ref(np.zeros(inp.shape), np.zeros(wshape)).shape
    prior = NAN
    if accum:
        prior = rnd(rng, oshape) * 3
        prior.reshape(-1)[rng.choice(prior.size, 5, replace=False)] = NAN       # NaN priors: they stay, wherever they are
    kw = dict(input_sizes=ishape, accum=accum, prior=prior, f16=f16, ld=ld, offset=offset, pad=cref.nan_fill())

    def run(a, ww):
        got, outside, names = o.conv_launch(kind, a, ww, s, **kw)
        assert cref.same_bits(outside, np.full(outside.shape, cref.nan_fill(), f32)), "floats outside the slice changed"
        if names_have:
            assert names_have in names, names
        with np.errstate(all="ignore"):
            want = ref(a, ww)
        return got, (want + prior.astype(f64) if accum else want), names

    clean, _, names = run(inp, w)
    bad = inp.copy()
    flat = rng.choice(bad.size, 2, replace=False)
    bad.reshape(-1)[flat[0]] = NAN
    bad.reshape(-1)[flat[1]] = INF
    got, want, _ = run(bad, w)
    tol = TOL if not f16 else 2 * TOL
    what = "%s %s k %s co %d s %s f16 %d accum %d %s " % (kind, xs, k, co, s, f16, accum, names)
    fin = check(got, want, what + "operand", tol, max(float(np.abs(clean[np.isfinite(clean)]).max()), 1e-30), clean)
    assert not fin.all()
    wbad = w.copy()
    cch = (xs[4] if kind == "input_grad" else co) // 2 + 1      # a channel of the result
    centre = (k[0] // 2, k[1] // 2, k[2] // 2)
    if kind == "transpose":
        wbad[centre + (cch, 0)] = NAN
    elif kind == "forward":
        wbad[centre + (0, cch)] = NAN
    else:
        wbad[centre + (cch, 0)] = NAN       # input gradient: the filter's input channel cch is the result's channel
    got, want, _ = run(inp, wbad)
    fin = check(got, want, what + "filter", tol, max(float(np.abs(clean[np.isfinite(clean)]).max()), 1e-30), clean)
    if kind == "forward" and not accum:     # item 6: the centre tap is inside the tensor at every position
        assert not fin[..., cch].any() and fin[..., cols(co, cch)].all()
    return names


@pytest.mark.parametrize("kind", ["forward", "input_grad"])
@pytest.mark.parametrize("splits", [0, 2, 4])
@pytest.mark.parametrize("tile", [0, 1, 2])
def test_conv_forced_tiles_and_k_slices(tile, splits, kind):
    """(1, 4, 8, 8, 64), 1x3x3 to 128 channels: every forced tile, whole and K-sliced (the K-slice exchange adds partial tiles: a
    NaN partial must reach the output, and only its own elements)."""
    with forced(tile, splits):
        names = conv_case(kind, (1, 4, 8, 8, 64), (1, 3, 3), 128, (1, 1, 1), seed=tile * 8 + splits)
    if tile < 2 or kind == "forward":      # the 128-column tile applies above 64 result channels (the input gradient has 64)
        assert TILE_NAMES[tile] in names, names


def test_conv_stem():
    """The stem has entry points of its own (3 input channels): ops.conv3d and the one-pass filter gradient."""
    o = ops()
    xs, k, co, s = (1, 2, 30, 28, 3), (1, 7, 7), 64, (1, 2, 2)
    rng = np.random.default_rng(21)
    x, w = rnd(rng, xs), rnd(rng, k + (3, co), 0.1)
    dy = rnd(rng, out_shape(xs, s, co))
    clean, cdw = o.conv3d(x, w, s), o.conv3d_backprop_filter(x, k + (3, co), dy, s)
    xb = x.copy()
    xb[0, 1, 14, 13, 2] = NAN
    xb[0, 0, 0, 27, 0] = INF
    with np.errstate(all="ignore"):
        fin = check(o.conv3d(xb, w, s), cref.forward(xb, w, s), "stem forward", TOL, float(np.abs(clean).max()), clean)
        assert not fin.all() and fin.any()
        check(o.conv3d_backprop_filter(xb, k + (3, co), dy, s), cref.filter_grad(xb, dy, k + (3, co), s), "stem filter gradient",
              TOL, float(np.abs(cdw).max()), cdw)
    wb = w.copy()
    wb[0, 3, 3, 1, 40] = NAN
    with np.errstate(all="ignore"):
        fin = check(o.conv3d(x, wb, s), cref.forward(x, wb, s), "stem forward, NaN filter", TOL, float(np.abs(clean).max()), clean)
    assert not fin[..., 40].any() and fin[..., cols(co, 40)].all()


@pytest.mark.parametrize("kind", ["forward", "input_grad"])
def test_conv_strided(kind):
    conv_case(kind, (1, 4, 10, 10, 16), (3, 3, 3), 24, (2, 2, 2))


def test_conv_transpose():
    conv_case("transpose", (1, 4, 8, 8, 32), (3, 3, 3), 16, (2, 2, 2))


@pytest.mark.parametrize("kind", ["forward", "input_grad"])
def test_conv_streaming_pointwise(kind):
    conv_case(kind, (1, 16, 32, 32, 64), (1, 1, 1), 64, (1, 1, 1), names_have="pw_stream_kernel")


@pytest.mark.parametrize("kind", ["forward", "input_grad"])
def test_conv_fp16_pointwise(kind):
    """Item 5: the fp16 option with NaN and +inf among operands of magnitude below 4, against the rounded-operand reference."""
    conv_case(kind, (2, 4, 12, 12, 64), (1, 1, 1), 256, (1, 1, 1), f16=True)


@pytest.mark.parametrize("kind", ["forward", "input_grad"])
def test_conv_slices_and_accumulating_epilogue(kind):
    """Operands as channel slices of wider rows, the result added to a prior that already holds NaN outside the footprint."""
    xs, co = (2, 4, 12, 12, 64), 64
    ld = (xs[4] + 4, 2 * co + 12) if kind == "forward" else (co + 4, 2 * xs[4] + 12)
    conv_case(kind, xs, (1, 3, 3), co, (1, 1, 1), ld=ld, offset=(4, 8), accum=True)


def test_conv_sibling_pair_keeps_a_nan_filter_to_its_member():
    """Two convs of one input sent as one grouped launch (the hook of test_gpu_bn.py): a NaN in member 0's filter poisons member
    0's output channel and its statistics, member 1's output and statistics keep their bits."""
    o = ops()
    xs, k, co = (2, 4, 12, 12, 64), (1, 3, 3), 64
    rng = np.random.default_rng(11)
    x, w, w2 = rnd(rng, xs), rnd(rng, k + (64, co), 0.1), rnd(rng, k + (64, co), 0.1)
    clean = o.conv_bn_stats(x, w, (1, 1, 1), filter2=w2)
    assert clean[5] == "igemm2_group_kernel(siblings)", clean[5]
    wb = w.copy()
    wb[0, 1, 1, 5, 9] = NAN
    ys, mean, invstd, mv, nparts, kernel = o.conv_bn_stats(x, wb, (1, 1, 1), filter2=w2)
    assert kernel == clean[5] and nparts == clean[4]
    with np.errstate(all="ignore"):
        check(ys[0], cref.forward(x, wb, (1, 1, 1)), "sibling 0", TOL, None, clean[0][0])
    assert np.isnan(ys[0][..., 9]).all() and np.isnan(mean[0][9]) and np.isnan(invstd[0][9]) and np.isnan(mv[0][:, 9]).all()
    for got, was in ((ys[1], clean[0][1]), (mean[1], clean[1][1]), (invstd[1], clean[2][1]), (mv[1], clean[3][1])):
        nf.clean_bits_equal(got, was, np.ones(was.shape, bool), "sibling 1")
    nf.clean_bits_equal(mean[0], clean[1][0], cols(co, 9), "sibling 0 mean, other channels")
    nf.clean_bits_equal(mv[0], clean[3][0], cols(co, 9), "sibling 0 moving, other channels")


def test_filter_gradient_group_keeps_a_nan_to_its_member():
    """Two filter gradients in one launch (ops.wgrad_group): the NaN and the +inf in member 0's x reach the taps and input
    channel the float64 reference says, member 1 keeps its bits."""
    o = ops()
    rng = np.random.default_rng(12)
    prs = []
    for xs, k, co in (((2, 4, 12, 12, 64), (1, 3, 3), 64), ((1, 3, 9, 10, 20), (3, 3, 3), 12)):
        prs.append(dict(x=rnd(rng, xs), dy=rnd(rng, xs[:4] + (co,)), filter_sizes=k + (xs[4], co), strides=(1, 1, 1),
                        dw=rnd(rng, k + (xs[4], co)), dbias=rnd(rng, (co,))))
    clean, name, cuts, _ = o.wgrad_group(prs)
    bad = dict(prs[0], x=prs[0]["x"].copy())
    bad["x"][1, 2, 0, 5, 7] = NAN             # a border cell: the taps that would read it from outside the tensor stay finite
    bad["x"][0, 1, 6, 6, 30] = INF
    got, name2, cuts2, _ = o.wgrad_group([bad, prs[1]])
    assert (name2, cuts2) == (name, cuts)
    with np.errstate(all="ignore"):
        want = cref.filter_grad(bad["x"], bad["dy"], bad["filter_sizes"], (1, 1, 1)) + bad["dw"].astype(f64)
    fin = check(got[0][0], want, "wgrad group member 0 " + name, TOL, float(np.abs(clean[0][0]).max()), clean[0][0])
    assert not fin.all() and fin[..., cols(64, 7, 30), :].all()
    nf.clean_bits_equal(got[0][1], clean[0][1], np.ones(64, bool), "member 0 dbias (dy is clean)")
    for q in (0, 1):
        nf.clean_bits_equal(got[1][q], clean[1][q], np.ones(clean[1][q].shape, bool), "wgrad group member 1")


# ---- attention -------------------------------------------------------------------------------------------------------------------
CORE = [(2, 129, 33, 64), (3, 5, 3, 32)]


def masked_rule(got, w64, w32, fin, floor, what):
    z = lambda a: np.where(fin, a, 0)
    if fin.any():
        ar.rule(z(got), z(w64), z(w32), floor=floor, what=what)


@pytest.mark.parametrize("which", ["g", "f", "h"])
@pytest.mark.parametrize("mode", ["stored", "flash"])
@pytest.mark.parametrize("B,ng,nf_,ch", CORE)
def test_attention_core(B, ng, nf_, ch, mode, which):
    """A NaN in one query row of g: that row of o and dg, and (through ds^T g and beta^T d_o) all of that batch's df and dh.  A NaN
    in one key of f or h: every row of that batch.  The other batches keep the clean launch's bits; the masks are the float64
    reference's."""
    o = ops()
    g, f, h, d = ar.core_input("units", B, ng, nf_, ch)
    clean = o.attention_core_launch(mode, g, f, h, d)
    bad = dict(g=g.copy(), f=f.copy(), h=h.copy())
    b0 = B - 1
    bad[which][b0, (ng if which == "g" else nf_) // 2, 1] = NAN
    got = o.attention_core_launch(mode, bad["g"], bad["f"], bad["h"], d)
    with np.errstate(all="ignore"):
        w64, w32 = ar.core(bad["g"], bad["f"], bad["h"], d), ar.core(bad["g"], bad["f"], bad["h"], d, f32)
    others = (np.arange(B) != b0).reshape(B, 1, 1)
    for name, a, w, w3, c, floor in zip(("o", "dg", "df", "dh"), got, w64, w32, clean, (ar.FLOOR, ar.FLOOR_DS, ar.FLOOR_DS, ar.FLOOR)):
        what = "attention %s %s NaN in %s: %s" % (mode, (B, ng, nf_, ch), which, name)
        fin = check(a, w, what, clean=c, region=others)
        assert fin[others[:, 0, 0]].all() and (name == "dh" or not fin[b0].all()), what      # (dh = beta^T d_o reads g and f only)
        masked_rule(a, w, w3, fin, floor, what)
    if which == "g":
        row = np.zeros((B, ng, 1), bool)
        row[b0, ng // 2] = True
        assert np.array_equal(np.isnan(got[0]), np.broadcast_to(row, got[0].shape))


def test_softmax_rows():
    """Rows holding a NaN, a +inf, a -inf, and all three: NaN and +inf make the whole row NaN (inf - inf), a lone -inf is a zero
    weight in an otherwise ordinary row; the other rows keep the clean launch's bits, pad columns stay 0, guard rows stay."""
    o = ops()
    rng = np.random.default_rng(3)
    for rows, cols_, ld in ((9, 33, 36), (6, 300, 300), (5, 4100, 4104)):
        s = rnd(rng, (rows, cols_), 2.0)
        wide = lambda a: np.concatenate([np.pad(a, ((0, 0), (0, ld - cols_)), constant_values=NAN), np.full((2, ld), NAN, f32)])
        clean = o.softmax_rows_launch(wide(s), cols_, guard_rows=2)
        bad = s.copy()
        bad[0, cols_ // 2] = NAN
        bad[1, 1] = INF
        bad[2, cols_ - 1] = -INF
        bad[3, [0, 5, cols_ - 2]] = [NAN, INF, -INF]
        got = o.softmax_rows_launch(wide(bad), cols_, guard_rows=2)
        with np.errstate(all="ignore"):
            want = ar.softmax_rows(bad)
            w32 = ar.softmax_rows(bad, f32)
        fin = check(got[:rows, :cols_], want, "softmax %dx%d" % (rows, cols_), clean=clean[:rows, :cols_],
                    region=(np.arange(rows) > 3)[:, None])
        masked_rule(got[:rows, :cols_], want, w32, fin, ar.FLOOR, "softmax %dx%d" % (rows, cols_))
        assert not fin[[0, 1, 3]].any() and fin[2].all() and got[2, cols_ - 1] == 0
        assert np.all(got[:rows, cols_:] == 0) and np.isnan(got[rows:]).all()


@pytest.mark.parametrize("gamma", [0.0, -0.7])
def test_attn_mix(gamma):
    """z = gamma r + x: a NaN in r is a NaN in z even at gamma = 0 (0 * NaN); dgamma = sum(dz r) is NaN; dr = gamma dz and dx = dz do
    not read the poisoned operands and keep their bits."""
    o = ops()
    M, C = 37, 36
    rng = np.random.default_rng(5)
    r, x, dz = rnd(rng, (M, C)), rnd(rng, (M, C)), rnd(rng, (M, C))
    clean = o.attn_mix(r, x, gamma, C, dz=dz)
    rb, xb = r.copy(), x.copy()
    rb[3, 35] = NAN
    xb[30, 0] = NAN
    rb[7, 7] = INF
    z, dr, dx, dgamma = o.attn_mix(rb, xb, gamma, C, dz=dz)
    with np.errstate(all="ignore"):
        zw = ar.mix(rb, xb, gamma)
        drw, dxw, dgw = ar.mix_bwd(dz, rb, gamma)
    fin = check(z, zw, "mix z", clean=clean[0])
    assert (~fin).sum() == 3 and np.isnan(z[3, 35]) and np.isnan(z[30, 0])
    check(dr, drw, "mix dr", clean=clean[1])
    check(dx, dxw, "mix dx", clean=clean[2])
    assert np.isnan(dgamma) and np.isnan(dgw)


# ---- head, losses, optimisers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transpose,fwd_path", [(True, 1), (True, 2), (False, 0)])      # (the stride-1 head has one kernel per pass)
def test_head(transpose, fwd_path):
    """A NaN and a +inf in interior cells.  Not covered, and written into item 6 of the contract as an implementation detail: the
    head's filter gradients multiply x by the zero gradient of output positions past the border, so a NaN or inf x in the LAST cell
    of an axis (the first too, for the stride-1 head) also reaches the taps of its channel that never read it (measured: 42 NaN
    where the reference has 27 for x[0, D-1, H-1, 0, 9] = +inf).  dk of that channel is non-finite either way.  Masking those taps
    was built and measured: head_bwd_filter_kernel 105 -> 135 us and other zero signs in the stride-1 head's dk, so it was not kept."""
    from test_gpu_head import oracle_head
    o = ops()
    shape = (2, 3, 5, 6, 16)
    rng = np.random.default_rng([transpose, fwd_path])
    x = rng.uniform(-1, 1, shape).astype(f32)
    k = (rng.uniform(-1, 1, (27, 16)) / 4).astype(f32)
    up = 2 if transpose else 1
    dl = rnd(rng, (2, up * 3, up * 5, up * 6))
    clean = o.head(x, k, 0.25, dl, transpose=transpose, fwd_path=fwd_path)
    assert fwd_path == 0 or clean[5][0] == fwd_path
    xb = x.copy()
    xb[1, 1, 2, 3, 5] = NAN
    xb[0, 1, 3, 2, 9] = INF
    logits, pred, dx, dk, db, info = o.head(xb, k, 0.25, dl, transpose=transpose, fwd_path=fwd_path)
    with np.errstate(all="ignore"):
        wl, wdx, wdk, wdb = oracle_head(xb, k, 0.25, dl, transpose)
        wp = 1.0 / (1.0 + np.exp(-wl))
    fin = check(logits, wl, "head logits", clean=clean[0])
    assert not fin.all() and fin.any()
    check(pred, wp, "head pred", clean=clean[1], region=np.isfinite(wl))
    assert set(np.unique(pred[np.isinf(wl)])) <= {0.0, 1.0}            # sigmoid(+-inf)
    check(dx, wdx, "head dx", clean=clean[2])                          # dx does not read x
    check(dk, wdk, "head dk", clean=clean[3])
    assert db == clean[4]


@pytest.mark.parametrize("through_sigmoid", [True, False])
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("n,offset", [(1021, 0), (1021, 1), (4099, 3)])
def test_elementwise_losses(n, offset, kind, through_sigmoid):
    """Smooth-L1, BCE and L1: a NaN logit makes the sum NaN and the gradient NaN at that element alone; the other elements'
    gradients keep their bits (float4 body and scalar head / tail)."""
    o = ops()
    rng = np.random.default_rng([n, offset, kind, through_sigmoid])
    z = rnd(rng, n, 2.0)
    y = rng.uniform(0, 1, n).astype(f32)
    sig = lambda v: (1.0 / (1.0 + np.exp(-v.astype(f64)))).astype(f32)
    run = lambda zz: o.loss(kind, zz, sig(zz) if through_sigmoid else zz, y, through_sigmoid=through_sigmoid, offset=offset)
    l0, d0, _ = run(z)
    assert np.isfinite(l0) and np.isfinite(d0).all()
    pos = [0, n // 2 + 1, n - 1]
    zb = z.copy()
    zb[pos] = NAN
    with np.errstate(all="ignore"):
        l1, d1, _ = run(zb)
    mask = np.zeros(n, bool)
    mask[pos] = True
    assert np.isnan(l1)
    assert np.array_equal(np.isnan(d1), mask)
    nf.clean_bits_equal(d1, d0, ~mask, "loss kind %d gradient" % kind)
    if through_sigmoid:                                     # z = +-inf on a sigmoid head: pred is exactly 1 / 0, nothing is NaN there
        zi = z.copy()
        zi[pos[0]], zi[pos[1]] = INF, -INF
        with np.errstate(all="ignore"):
            l2, d2, _ = run(zi)
        assert not np.isnan(d2[~mask]).any()
        nf.clean_bits_equal(d2, d0, ~mask, "loss kind %d gradient (inf logits)" % kind)
        if kind != 1:                                       # Smooth-L1 and L1 see pred = 1 / 0: finite terms, zero slope
            assert np.isfinite(l2) and d2[pos[0]] == 0 and d2[pos[1]] == 0


@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("ts", [1, 0])
@pytest.mark.parametrize("offset", [0, 3])
def test_map_losses(offset, ts, fix):
    """KLD + CC (and with fixations NSS) per map: a NaN in map 1 makes the sum NaN and that map's terms and whole gradient NaN (the
    map's sums reach every element); maps 0 and 2 keep their terms and their gradient bits."""
    o = ops()
    maps, n = 3, 7 * 9
    rng = np.random.default_rng([offset, ts, fix])
    z = rnd(rng, maps * n)
    y = rng.uniform(0, 1, maps * n).astype(f32)
    s = map_loss_ref.sigmoid32(z)
    fx = (rng.random(maps * n) < 0.1).astype(np.uint8) * 255 if fix else None

    def run(zz):
        p = map_loss_ref.sigmoid32(zz) if ts else None
        if fix:
            return o.saliency_loss(zz, p, y, fx, maps, n, through_sigmoid=bool(ts), offset=offset)
        return o.map_loss(zz, p, y, maps, n, through_sigmoid=bool(ts), offset=offset)

    l0, d0, per0, _ = run(z)
    assert np.isfinite(l0) and np.isfinite(d0).all() and s.size == z.size
    zb = z.copy()
    zb[n + 5] = NAN
    with np.errstate(all="ignore"):
        l1, d1, per1, _ = run(zb)
    inmap = np.zeros(maps * n, bool)
    inmap[n:2 * n] = True
    assert np.isnan(l1)
    assert np.array_equal(np.isnan(d1), inmap), (int(np.isnan(d1).sum()), n)
    nf.clean_bits_equal(d1, d0, ~inmap, "map loss gradient")
    assert np.isnan(per1[1, :2]).all()
    assert np.array_equal(per1[[0, 2]], per0[[0, 2]], equal_nan=True)


OPT_N = [(1023, 0), (1021, 1), (4098, 2), (7, 3)]


def opt_positions(n):
    return sorted({0, 1, n // 2, n - 2, n - 1} & set(range(n)))


def opt_check(outs, cleans, mask, what, poisoned_outputs):
    for q, (a, c) in enumerate(zip(outs, cleans)):
        if q in poisoned_outputs:
            assert np.array_equal(np.isnan(a), mask), (what, q)
        else:
            assert np.isfinite(a).all(), (what, q)
        nf.clean_bits_equal(a, c, ~mask, "%s output %d" % (what, q))


@pytest.mark.parametrize("n,offset", OPT_N)
def test_optimiser_kernels(n, offset):
    """Adam, Adam with decay, Momentum, Nesterov, SGD and their decay forms, plain and with clipping's scale: a NaN gradient
    element poisons that element of p and of its slots and nothing else -- the float4 body, the scalar head / tail (n % 4 != 0)
    and every alignment of the base."""
    o = ops()
    rng = np.random.default_rng([n, offset])
    p, g, m = rnd(rng, n), rnd(rng, n), rnd(rng, n, 0.1)
    v = (rnd(rng, n, 0.1) ** 2).astype(f32)
    pos = opt_positions(n)
    mask = np.zeros(n, bool)
    mask[pos] = True
    gb = g.copy()
    gb[pos] = NAN
    tiles = [(n - n // 3, 0.01), (n // 3, 0.0)] if n // 3 else [(n, 0.01)]
    for gscale in (None, 0.37):
        what = "n %d offset %d gscale %s " % (n, offset, gscale)
        # Adam's launches, the decay forms and the scaled ones want a 16-byte aligned base (test_adam_refuses_a_misaligned_base):
        # offset 0 there, the drawn offset on the plain Momentum / SGD launch
        opt_check(o.adam(p, gb, m, v, 3, gscale=gscale)[:3], o.adam(p, g, m, v, 3, gscale=gscale)[:3], mask, what + "adam", (0, 1, 2))
        opt_check(o.adam_decay(p, gb, m, v, tiles, 3, gscale=gscale)[:4], o.adam_decay(p, g, m, v, tiles, 3, gscale=gscale)[:4], mask,
                  what + "adam_decay", (0, 1, 2, 3))
        for kind, nest in (("momentum", False), ("momentum", True), ("sgd", False)):
            hit = (0, 1) if kind == "momentum" else (0,)
            off = offset if gscale is None else 0
            opt_check(o.optimizer(kind, p, gb, m, use_nesterov=nest, offset=off, gscale=gscale),
                      o.optimizer(kind, p, g, m, use_nesterov=nest, offset=off, gscale=gscale), mask, what + kind, hit)
            opt_check(o.optimizer_decay(kind, p, gb, m, tiles, use_nesterov=nest, gscale=gscale)[:3],
                      o.optimizer_decay(kind, p, g, m, tiles, use_nesterov=nest, gscale=gscale)[:3], mask,
                      what + kind + "_decay", (0, 1, 2) if kind == "momentum" else (0, 1))


@pytest.mark.parametrize("n,offset", OPT_N)
def test_ema_and_grad_accum(n, offset):
    o = ops()
    rng = np.random.default_rng([n, offset, 1])
    s, p = rnd(rng, n), rnd(rng, n)
    pos = opt_positions(n)
    mask = np.zeros(n, bool)
    mask[pos] = True
    pb = p.copy()
    pb[pos] = NAN
    opt_check([o.ema(s, pb, 0.01, offset=offset)], [o.ema(s, p, 0.01, offset=offset)], mask, "ema", (0,))
    for mode in ("store", "add", "finish"):
        opt_check([o.grad_accum(s, pb, mode, offset=offset)], [o.grad_accum(s, p, mode, offset=offset)], mask, "grad_accum " + mode, (0,))


# ---- whole graphs ------------------------------------------------------------------------------------------------------------------
CFG = p3d.NetConfig(base=8, blocks=(1, 1, 1))
CFG16 = p3d.NetConfig(base=16, blocks=(1, 1, 1))      # attention and the decoder-block head need a base that is a multiple of 16
SHAPE = (2, 16, 32, 32)


def poisoned_batch():
    x = p3d.synthetic_clip(0, SHAPE + (3,)).copy()
    y = p3d.synthetic_target(3, SHAPE)
    xb = x.copy()
    xb[0, 3, 5, 7, 1] = NAN
    return x, xb, y


def make(structure, params, attention=None, cfg=CFG):
    from sap3d_tensorflow_amd import P3DSession
    s = P3DSession(structure, batch=SHAPE[0], frames=SHAPE[1], height=SHAPE[2], width=SHAPE[3], base=cfg.base, blocks=cfg.blocks)
    s.load(params)
    if attention:
        s.set_attention_mode(attention)
    return s


@pytest.mark.parametrize("structure,attention", [("unet", None), ("unet++ds", "gemm"), ("unet++ds", "flash")])
def test_graph_batchnorm_networks(structure, attention):
    """One NaN pixel in clip 0 (base 8 for unet; unet++ds at base 16, the smallest its attention blocks take).  The training step's loss is NaN and pred has the oracle's mask (all of it: batch statistics couple
    the clips); the step poisons the weights, so the next step on a CLEAN batch still reports a non-finite loss.  The inference
    forward has the oracle's mask per clip -- all of it here too, because the backbone blocks keep batch statistics whatever
    `training` says (tests/test_nonfinite_ref_cpu.py) -- also with BatchNorm fused into the convs forward and backward and with
    the fp16 pointwise mode."""
    from test_gpu_net import randomise_norm_params
    x, xb, y = poisoned_batch()
    cfg = CFG if structure == "unet" else CFG16
    params = randomise_norm_params(p3d.init_params(1, structure, cfg))
    with np.errstate(all="ignore"):
        wl, wp, wg, _ = p3d.loss_and_grads(dict(params), xb, y, 0.0, True, structure, cfg)
        wi, _ = p3d.forward(dict(params), xb, 0.0, False, structure, cfg)
    assert np.isnan(wl) and np.isnan(wp).all() and np.isnan(np.asarray(wi)).all()
    s = make(structure, params, attention, cfg)
    pred = s.forward(xb, 0.0, False)
    nf.footprint_equal(pred.reshape(wi.shape), wi, structure + " inference pred")
    for fusion, fp16 in ((2, False), (0, True), (2, True)):
        s.set_bn_fusion(fusion)
        s.set_pointwise_fp16(fp16)
        nf.footprint_equal(s.forward(xb, 0.0, False).reshape(wi.shape), wi, "%s inference fusion %d fp16 %d" % (structure, fusion, fp16))
        loss, pred = s.backward(xb, y, 0.0)
        assert np.isnan(loss), (fusion, fp16, loss)
    s.close()
    s = make(structure, params, attention, cfg)
    assert np.isfinite(s.backward(x, y, 0.0)[0])                       # the clean batch, same session setup
    loss, pred = s.backward(xb, y, 0.0)
    assert np.isnan(loss), loss
    nf.footprint_equal(pred.reshape(wp.shape), wp, structure + " training pred")
    bad = [n for n in wg if not np.isfinite(s.get_grad(n)).all()]
    assert "firstconv1" in bad and len(bad) >= len(wg) // 2, (len(bad), len(wg))
    assert np.isnan(s.train_step(xb, y, dropout=0.0)), "train_step on the poisoned batch"
    assert not np.isfinite(s.train_step(x, y, dropout=0.0)), "the step after: the weights are poisoned, and the loss says so"
    s.close()


def test_graph_groupnorm_decoder():
    """GroupNorm does not couple the clips: clip 0's pred has the oracle's NaN mask, clip 1's pred stays within the forward
    tolerance of the clean pred, in training and in inference; the loss is NaN and the following clean step reports it."""
    from oracle import p3d_gn
    from test_gpu_net import _gn_params
    x, xb, y = poisoned_batch()
    params = _gn_params(CFG16, np.float32, "decoder")
    with np.errstate(all="ignore"):
        wl, wp, wg, _ = p3d_gn.loss_and_grads(dict(params), xb, y, 0.0, True, CFG16, np.float32, head="decoder")
        wi, _ = p3d_gn.forward(dict(params), xb, 0.0, False, CFG16, np.float32, head="decoder")
        ci, _ = p3d_gn.forward(dict(params), x.astype(f64), 0.0, False, CFG16, np.float64, head="decoder")
    wp, wi, ci = (np.asarray(a).reshape(2, -1) for a in (wp, wi, ci))
    assert np.isnan(wl) and np.isnan(wp[0]).any() and np.isfinite(wp[1]).all()
    s = make("gn_p3d_decoder", params, cfg=CFG16)
    for training, want in ((False, wi), (True, wp)):
        pred = s.forward(xb, 0.0, training).reshape(2, -1)
        nf.footprint_equal(pred, want, "gn decoder pred, training %s" % training)
        assert np.abs(pred[1] - ci[1]).max() <= 1e-4 * max(np.abs(ci).max(), 1.0)
    loss, pred = s.backward(xb, y, 0.0)
    assert np.isnan(loss)
    nf.footprint_equal(pred.reshape(2, -1), wp, "gn decoder backward pred")
    assert np.isnan(s.train_step(xb, y, dropout=0.0))
    assert not np.isfinite(s.train_step(x, y, dropout=0.0))
    s.close()
