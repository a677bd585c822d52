"""The fused-BatchNorm launches (p3d_set_bn_fusion: csrc/conv_igemm2.hip AT = RELU1 / RELU2 / GRAD, the ngate branch of
igemm_epilogue.h, xt / dyt of conv_wgrad2.hip, bn_finalize_kernel / bn_grad_finalize_kernel) op by op against the float64 laws
of tests/fused_bn_ref.py, through the hooks p3d_debug_fused_conv / p3d_debug_fused_wgrad / p3d_debug_fused_reject, which build
their launches with the builders conv() uses (net.hip, fused_*).

  a. folded coefficients: 1, 7, 32 partials in the consumer's prologue, 33 through the finalize launch (asserted by name), from
     float32 partials the test supplies; an offset of 16 sigma, a constant channel that hits the variance clamp; publish = 0 and
     update_moving = 0 leave their arrays bit for bit.
  b. RELU1 / RELU2 forward with shifts of O(1) (a padded tap that read relu(shift) would be far out), slices, forced tiles and
     K-slices, two sources in one buffer, the fp16 option (rounds the TRANSFORMED operand: FusedLoop reads the transformed tile).
  c. GRAD input gradient with k3 of O(1); coefficients from partials with / without publish, and published.
  d. gates on supplied scale / shift / mean / invstd with every decision at least 1e-4 from 0 (none excluded): exact zeros, one
     value for both gates, raw_store, untouched raw buffer, partial rows and their sums.
  e. filter gradients with xt = 1 / 2, dyt, both, on forced tiles, alone and in a mixed group of three, onto a random prior.
  f. one chain on the device against the composition of the laws.
  g. malformed launches are refused by the launchers / the validator / the builder.

Tolerances.  TOL = 2e-5 of the expected result's max magnitude (max |prior + result| where a launch accumulates): the project's
conv tolerance (tests/test_gpu_ops.py).  Coefficients: 16 * eps32 * (sum of the magnitudes of the terms of the expression): the
folds run in double and at most about six float32 roundings follow.  Gate partials: (rows of the tile) * eps32 * sum |term|, the
worst-case bound of a float32 summation of that many terms, against float64 sums of the hook's OWN gated output.  Moving
statistics: 4 float32 ulps of the moving values (tests/test_gpu_bn.py).  Every path-specific case asserts the kernel name."""
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fused_bn_ref as ref              # noqa: E402
from conv_launch_ref import nan_fill, same_bits              # noqa: E402
from test_gpu_conv_launch import TOL, forced, slice_forms              # noqa: E402

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
NANP = nan_fill()
BIG, SMALL = (2, 4, 7, 7), (1, 2, 5, 6)        # M = 392 (ragged for 64- and 128-row tiles), M = 60 (less than one tile)
KERNELS = [(1, 1, 1), (1, 3, 3), (3, 1, 1)]
TILE_NAMES = {0: "<64,64", 1: "<128,64", 2: "<128,128"}
AT_NAMES = {1: ",relu1", 2: ",relu2", 3: ",bngrad"}      # launch_igemm's name table (net.hip)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def rnd(rng, shape, scale=1.0, mean=0.0):
    return f32(rng.standard_normal(shape) * scale + mean)


def embed(a, ld, off, fill=NANP):
    a = f32(a).reshape(-1, a.shape[-1])
    out = np.full((a.shape[0], ld), fill, np.float32)
    out[:, off:off + a.shape[1]] = a
    return out


def inside(buf, C, off, shape=None):
    v = buf[:, off:off + C]
    return v if shape is None else v.reshape(shape)


def outside_untouched(buf, C, off, what=""):
    o = np.concatenate([buf[:, :off], buf[:, off + C:]], axis=1)
    assert same_bits(o, np.full(o.shape, NANP, np.float32)), (what, "floats outside the slice changed")


def close(got, want, tol=TOL, what="", scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(got).any(), (what, "NaN left", int(np.isnan(got).sum()))
    scale = max(np.abs(want).max(), 1e-30) if scale is None else scale
    err = np.abs(got - want).max() / scale
    print("%s err %.3g (tol %.3g)" % (what, err, tol))
    assert err < tol, (what, err)
    return err


def coef_close(got, want, terms, what):
    """16 * eps32 * sum |term| per channel (module docstring)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    bound = 16 * EPS32 * np.maximum(terms, 1e-30)
    print("%s worst err / bound %.3g" % (what, (err / bound).max()))
    assert (err <= bound).all(), (what, (err / bound).max())


def fma32(s, y, t):
    """float32 fma(s, y, t) of float32 inputs: the product is exact in float64, the sum is rounded once more (to float32)."""
    return (np.asarray(s, np.float64) * np.asarray(y, np.float64) + np.asarray(t, np.float64)).astype(np.float32)


def relu_operand32(x, s, t, x2=None, s2=None, t2=None):
    """The transformed operand as the kernel holds it in float32 (transform_store)."""
    a = np.maximum(fma32(s, x, t), np.float32(0))
    if x2 is not None:
        a = (a + np.maximum(fma32(s2, x2, t2), np.float32(0))).astype(np.float32)
    return a


def check_name(names, at, tile, Nc, gate=False, f16=False):
    last = names.split(";")[-1]
    if f16:
        assert last.endswith(",f16>"), names
    else:
        assert last.endswith(AT_NAMES.get(at, "") + (",gate" if gate else "") + ">"), names
        assert (",gate" in last) == gate, names
    if tile in (0, 1) or (tile == 2 and Nc > 64):
        assert TILE_NAMES[tile] + "," in last, (names, tile)
    return 128 if "<128," in last else 64


def check_splits(res, splits, K, taps):
    steps = taps * -(-K // 32)
    if splits and steps >= splits:
        assert res["splits"][1] == splits, (res["splits"], splits, steps)


def fused():
    from sap3d_tensorflow_amd import ops
    return ops


def split_bounds(rng, M, n):
    """An arbitrary split of M rows into n non-empty ranges."""
    cuts = np.sort(rng.choice(np.arange(1, M), n - 1, replace=False)) if n > 1 else np.array([], int)
    return [0] + [int(c) for c in cuts] + [M]


def taps_of(k):
    return k[0] * k[1] * k[2]


# ---- a. folded coefficients ---------------------------------------------------------------------------------------------------
def clamp_constant(bounds, M):
    """A constant whose float32 partials over `bounds` give sum(x^2) / M - mean^2 < 0 (probed on the CPU)."""
    for c in np.linspace(1.0, 40.0, 800):
        y = np.full((M, 1), np.float32(c), np.float32)
        if ref.fold(ref.partials_of(y, bounds), M, np.ones(1), np.zeros(1))["raw_var"][0] < 0:
            return np.float32(c)
    raise AssertionError("no constant with a negative raw variance for this split")


@pytest.mark.parametrize("K", [64, 40])
@pytest.mark.parametrize("nparts", [1, 7, 32, 33])
def test_forward_fold_publishes_the_law(nparts, K):
    rng = np.random.default_rng(100 + nparts + K)
    M, Nc = 392, 36
    bounds = split_bounds(rng, M, nparts)
    y = rnd(rng, (M, K))
    y[:, 1] += 16.0                                    # mean 16 sigma
    y[:, 0] = clamp_constant(bounds, M)                # hits the clamp
    y[:, K - 1] = rnd(rng, M, 0.05, -3.0)              # the last channel of the tail
    parts = ref.partials_of(y, bounds)
    gamma, beta = f32(rng.uniform(0.5, 1.5, K)), rnd(rng, K)
    mm0, mv0 = rnd(rng, K), f32(rng.uniform(0.5, 2.0, K))
    w = rnd(rng, (1, 1, 1, K, Nc), 0.2)
    law = ref.fold(parts, M, gamma, beta)
    assert law["raw_var"][0] < 0 and law["var"][0] == 0
    pre = {k: np.full(K, NANP, np.float32) for k in ("scale", "shift", "mean", "invstd")}
    src = dict(y=embed(y, K, 0), off=0, gamma=gamma, beta=beta, partials=parts, rows=M, publish=1, update_moving=1,
               moving_mean=mm0, moving_var=mv0, **pre)
    res = fused().fused_conv("forward", BIG + (K,), w, (1, 1, 1), np.full((M, Nc), NANP, np.float32), src=[src])
    names = res["kernels"].split(";")
    if nparts > ref.FOLD_MAX:
        assert names[0] == "bn_finalize_kernel" and len(names) == 2, names       # the rule: beyond 32, the finalize launch ...
    else:
        assert len(names) == 1, names
    assert names[-1].endswith(",relu1>"), names
    pub = res["src"][0]
    for k in ("mean", "invstd", "scale", "shift"):
        coef_close(pub[k], law[k], law["terms"][k], k)
    mm_want, mv_want = ref.moving_update(mm0, law["mean"]), ref.moving_update(mv0, law["var"])
    ulps = 4 * EPS32 * (np.abs(mm_want).max() + np.abs(mv_want).max())
    assert np.abs(pub["moving_mean"] - mm_want).max() <= ulps and np.abs(pub["moving_var"] - mv_want).max() <= ulps
    # ... and the consumer reads the published values: the output is the law on them
    want = ref.conv(ref.relu_operand(y.reshape(BIG + (K,)), pub["scale"], pub["shift"]), w)
    close(res["out"].reshape(want.shape), want, what="output on the published coefficients")
    # publish = 0: the same output, the published arrays and the moving statistics bit for bit as they were
    if nparts <= ref.FOLD_MAX:
        src2 = dict(src, publish=0)
        res2 = fused().fused_conv("forward", BIG + (K,), w, (1, 1, 1), np.full((M, Nc), NANP, np.float32), src=[src2])
        for k in pre:
            assert same_bits(res2["src"][0][k], pre[k]), k
        assert same_bits(res2["src"][0]["moving_mean"], mm0) and same_bits(res2["src"][0]["moving_var"], mv0)
        assert same_bits(res2["out"], res["out"])
    # update_moving off: published, moving statistics untouched
    res3 = fused().fused_conv("forward", BIG + (K,), w, (1, 1, 1), np.full((M, Nc), NANP, np.float32), src=[dict(src, update_moving=0)])
    assert same_bits(res3["src"][0]["moving_mean"], mm0) and same_bits(res3["src"][0]["moving_var"], mv0)
    assert same_bits(res3["src"][0]["scale"], pub["scale"]) and same_bits(res3["src"][0]["shift"], pub["shift"])


def test_forward_fold_publishes_once_under_k_slices_and_many_tiles():
    """The publisher is block 0 of slice 0 alone: with K-slices and several tiles the moving statistics move ONCE."""
    rng = np.random.default_rng(7)
    M, K, Nc = 392, 64, 132
    y = rnd(rng, (M, K), 1.0, 0.5)
    parts = ref.partials_of(y, split_bounds(rng, M, 7))
    gamma, beta = f32(rng.uniform(0.5, 1.5, K)), rnd(rng, K)
    mm0, mv0 = rnd(rng, K), f32(rng.uniform(0.5, 2.0, K))
    w = rnd(rng, (1, 3, 3, K, Nc), 0.1)
    law = ref.fold(parts, M, gamma, beta)
    z = np.zeros(K, np.float32)
    src = dict(y=y, off=0, gamma=gamma, beta=beta, partials=parts, rows=M, publish=1, update_moving=1, moving_mean=mm0,
               moving_var=mv0, scale=z, shift=z, mean=z, invstd=z)
    with forced(0, 3):
        res = fused().fused_conv("forward", BIG + (K,), w, (1, 1, 1), np.full((M, Nc), NANP, np.float32), src=[src])
    assert res["splits"][1] == 3
    mm_want, mv_want = ref.moving_update(mm0, law["mean"]), ref.moving_update(mv0, law["var"])
    ulps = 4 * EPS32 * (np.abs(mm_want).max() + np.abs(mv_want).max())
    assert np.abs(res["src"][0]["moving_mean"] - mm_want).max() <= ulps and np.abs(res["src"][0]["moving_var"] - mv_want).max() <= ulps
    want = ref.conv(ref.relu_operand(y.reshape(BIG + (K,)), res["src"][0]["scale"], res["src"][0]["shift"]), w)
    close(res["out"].reshape(want.shape), want, what="K-sliced output")


# ---- b. RELU1 / RELU2 forward -------------------------------------------------------------------------------------------------
def fwd_cases():
    out = []
    for i, (k, K, Nc) in enumerate(itertools.product(KERNELS, [64, 40], [64, 36, 132])):
        out.append((k, K, Nc, 1 + i % 2, i % 3, (1, 3)[(i // 2) % 2], SMALL if i % 4 == 3 else BIG, i))
    return out


def published(rng, K):
    """scale of either sign and O(1), shift of O(1): relu(shift) is far from 0 on about half the channels."""
    s = f32(rng.uniform(0.5, 1.5, K) * rng.choice([-1.0, 1.0], K))
    t = rnd(rng, K, 1.0)
    return s, t


@pytest.mark.parametrize("k,K,Nc,at,tile,splits,sp,i", fwd_cases())
def test_relu_forward(k, K, Nc, at, tile, splits, sp, i):
    rng = np.random.default_rng(200 + i)
    forms_in, forms_out = slice_forms(K), slice_forms(Nc)
    (ld0, off0), (ld1, off1) = forms_in[i % len(forms_in)], forms_in[(i + 3) % len(forms_in)]
    ldo, offo = forms_out[(2 * i + 1) % len(forms_out)]
    xs = sp + (K,)
    M = int(np.prod(sp))
    x = [rnd(rng, xs) for _ in range(at)]
    st = [published(rng, K) for _ in range(at)]
    w, bias = rnd(rng, k + (K, Nc), 0.2), (rnd(rng, Nc) if i % 3 == 0 else None)
    z = np.zeros(K, np.float32)
    src = [dict(y=embed(x[q], (ld0, ld1)[q], (off0, off1)[q]), off=(off0, off1)[q], scale=st[q][0], shift=st[q][1], mean=z, invstd=z)
           for q in range(at)]
    with forced(tile, splits):
        res = fused().fused_conv("forward", xs, w, (1, 1, 1), np.full((M, ldo), NANP, np.float32), off_out=offo, bias=bias, src=src)
    check_name(res["kernels"], at, tile, Nc)
    check_splits(res, splits, K, taps_of(k))
    a = ref.relu_operand(x[0], *st[0], *((x[1],) + st[1] if at == 2 else ()))
    want = ref.conv(a, w) + (0 if bias is None else bias.astype(np.float64))
    close(inside(res["out"], Nc, offo, want.shape), want, what="relu%d %s" % (at, res["kernels"]))
    outside_untouched(res["out"], Nc, offo)
    for q in range(at):      # published coefficients are read, never written
        assert same_bits(res["src"][q]["scale"], st[q][0]) and same_bits(res["src"][q]["mean"], z)


@pytest.mark.parametrize("tile", [0, 1])
def test_relu2_sources_in_two_slices_of_one_buffer(tile):
    rng = np.random.default_rng(31 + tile)
    K, Nc, k = 40, 36, (1, 3, 3)
    xs = BIG + (K,)
    x = [rnd(rng, xs) for _ in range(2)]
    st = [published(rng, K) for _ in range(2)]
    w = rnd(rng, k + (K, Nc), 0.2)
    ld, offs = 2 * K + 12, (4, K + 12)
    buf = embed(x[0], ld, offs[0])
    buf[:, offs[1]:offs[1] + K] = x[1].reshape(-1, K)
    z = np.zeros(K, np.float32)
    src = [dict(y=buf, off=offs[q], scale=st[q][0], shift=st[q][1], mean=z, invstd=z) for q in range(2)]
    with forced(tile, 0):
        res = fused().fused_conv("forward", xs, w, (1, 1, 1), np.full((392, Nc), NANP, np.float32), src=src)
    check_name(res["kernels"], 2, tile, Nc)
    want = ref.conv(ref.relu_operand(x[0], *st[0], x[1], *st[1]), w)
    close(res["out"].reshape(want.shape), want, what="relu2, one buffer")


@pytest.mark.parametrize("at,K,Nc", [(1, 64, 64), (2, 40, 132)])
def test_relu_forward_fp16_rounds_the_transformed_operand(at, K, Nc):
    rng = np.random.default_rng(41 + at)
    xs = BIG + (K,)
    x = [rnd(rng, xs) for _ in range(at)]
    st = [published(rng, K) for _ in range(at)]
    w = rnd(rng, (1, 1, 1, K, Nc), 0.2)
    z = np.zeros(K, np.float32)
    src = [dict(y=embed(x[q], K, 0), off=0, scale=st[q][0], shift=st[q][1], mean=z, invstd=z) for q in range(at)]
    res = fused().fused_conv("forward", xs, w, (1, 1, 1), np.full((392, Nc), NANP, np.float32), src=src, f16=True)
    check_name(res["kernels"], at, -1, Nc, f16=True)
    a32 = relu_operand32(x[0], *st[0], *((x[1],) + st[1] if at == 2 else ()))
    rounded = ref.conv(ref.half(a32), ref.half(w))
    plain = ref.conv(a32, w)
    got = res["out"].reshape(rounded.shape)
    close(got, rounded, what="fp16, rounded reference")
    assert np.abs(got - plain).max() / np.abs(plain).max() > TOL, "fp16 path indistinguishable from float32"


# ---- c. GRAD input gradient ---------------------------------------------------------------------------------------------------
def grad_problem(rng, sp, Cin, Cout, k, nparts):
    """A conv Cin -> Cout whose output feeds a fused BatchNorm: gated gradient g with mean of O(1) (so k3 is O(1)), the
    BatchNorm's input y, its saved statistics, and float32 partials of (sum g, sum g*xhat) over an arbitrary row split."""
    M = int(np.prod(sp))
    g = rnd(rng, sp + (Cout,), 1.0, 1.5)
    y = rnd(rng, sp + (Cout,), 1.0, 0.7)
    gamma = f32(rng.uniform(0.5, 1.5, Cout))
    mean, invstd = rnd(rng, Cout, 0.3, 0.7), f32(rng.uniform(0.7, 1.4, Cout))
    bounds = split_bounds(rng, M, nparts)
    g2, gx = g.reshape(M, Cout).astype(np.float64), None
    gx = g2 * (y.reshape(M, Cout).astype(np.float64) - mean) * invstd
    parts = np.stack([np.stack([g2[a:b].sum(0), gx[a:b].sum(0)], -1) for a, b in zip(bounds[:-1], bounds[1:])]).astype(np.float32)
    w = rnd(rng, k + (Cin, Cout), 0.2)
    return dict(M=M, g=g, y=y, gamma=gamma, mean=mean, invstd=invstd, parts=parts, w=w, law=ref.grad_fold(parts, M, gamma, mean, invstd))


def check_published_grad(got, law):
    C = law["k1"].shape[0]
    coef = got["coef"].reshape(3, C)
    for j, kname in enumerate(("k1", "k2", "k3")):
        coef_close(coef[j], law[kname], law["terms"][kname], kname)
    coef_close(got["dgamma"], law["dgamma"], law["terms"]["dgamma"], "dgamma")
    coef_close(got["dbeta"], law["dbeta"], law["terms"]["dbeta"], "dbeta")


def grad_cases():
    out = []
    for i, (k, Cout, Cin) in enumerate(itertools.product(KERNELS, [64, 40], [64, 36, 132])):
        out.append((k, Cout, Cin, i % 3, (1, 3)[(i // 3) % 2], ("publish", "fold", "published")[(i // 2) % 3], (1, 7, 32, 33)[i % 4],
                    SMALL if i % 5 == 4 else BIG, i % 2, i))
    return out


@pytest.mark.parametrize("k,Cout,Cin,tile,splits,mode,nparts,sp,accum,i", grad_cases())
def test_grad_input_gradient(k, Cout, Cin, tile, splits, mode, nparts, sp, accum, i):
    rng = np.random.default_rng(300 + i)
    if mode == "fold" and nparts > ref.FOLD_MAX:
        nparts = 32                                   # beyond 32 the finalize launch publishes: no fold-only form exists
    nparts = min(nparts, int(np.prod(sp)) - 1)
    pr = grad_problem(rng, sp, Cin, Cout, k, nparts)
    M, law = pr["M"], pr["law"]
    fg, fy, fo = slice_forms(Cout)[i % 3], slice_forms(Cout)[(i + 2) % 3], slice_forms(Cin)[(i + 1) % 3]
    prior = rnd(rng, (M, Cin)) if accum else np.full((M, Cin), NANP, np.float32)
    pre = dict(coef=np.full((3, Cout), NANP, np.float32), dgamma=np.full(Cout, NANP, np.float32), dbeta=np.full(Cout, NANP, np.float32))
    grad = dict(y=embed(pr["y"], *fy), off=fy[1], **pre)
    if mode == "published":
        given = np.stack([law["k1"], law["k2"], law["k3"]]).astype(np.float32)
        grad["coef"] = given
    else:
        grad.update(gamma=pr["gamma"], mean=pr["mean"], invstd=pr["invstd"], partials=pr["parts"], rows=M, publish=int(mode == "publish"))
    with forced(tile, splits):
        res = fused().fused_conv("input_grad", sp + (Cin,), pr["w"], (1, 1, 1), embed(prior, *fo), off_out=fo[1],
                                 g=embed(pr["g"], *fg), off_g=fg[1], grad=grad, accum=bool(accum))
    names = res["kernels"].split(";")
    if mode == "publish" and nparts > ref.FOLD_MAX:
        assert names[0] == "bn_grad_finalize_kernel" and len(names) == 2, names
    else:
        assert len(names) == 1, names
    check_name(res["kernels"], 3, tile, Cin)
    check_splits(res, splits, Cout, taps_of(k))
    got = res["grad"]
    if mode == "publish":
        check_published_grad(got, law)
        k1, k2, k3 = got["coef"].reshape(3, Cout)
    else:
        for kk in ("dgamma", "dbeta"):
            assert same_bits(got[kk], pre[kk]), kk
        assert same_bits(got["coef"], grad["coef"])
        k1, k2, k3 = grad["coef"] if mode == "published" else (law["k1"], law["k2"], law["k3"])
    want = ref.conv_input_grad(ref.grad_operand(pr["g"], pr["y"], k1, k2, k3), pr["w"])
    if accum:
        want = want + prior.reshape(want.shape)
    close(inside(res["out"], Cin, fo[1], want.shape), want, what="grad %s %s" % (mode, res["kernels"]))
    outside_untouched(res["out"], Cin, fo[1])


# ---- d. gates -----------------------------------------------------------------------------------------------------------------
def gate_inputs(rng, M, C):
    """scale, shift, mean, invstd and a y whose float32 fma(scale, y, shift) is at least 1e-4 from 0 everywhere."""
    scale, shift = published(rng, C)
    mean, invstd = rnd(rng, C, 0.3), f32(rng.uniform(0.7, 1.4, C))
    y = rnd(rng, (M, C))
    for _ in range(50):
        bad = np.abs(fma32(scale, y, shift)) < 1e-4
        if not bad.any():
            break
        y[bad] = rnd(rng, int(bad.sum()))
    assert not (np.abs(fma32(scale, y, shift)) < 1e-4).any()
    return dict(scale=scale, shift=shift, mean=mean, invstd=invstd, y=y)


def gate_cases():
    out = []
    for i, (k, Cout, Cin) in enumerate(itertools.product(KERNELS, [64, 40], [64, 36, 132])):
        out.append((k, Cout, Cin, i % 3, (1, 3)[(i // 3) % 2], 1 + i % 2, (i // 2) % 2, (i // 4) % 2, i % 3 != 1,
                    SMALL if i % 6 == 5 else BIG, i))
    return out


@pytest.mark.parametrize("k,Cout,Cin,tile,splits,ngate,raw_store,accum,with_grad,sp,i", gate_cases())
def test_gated_epilogue(k, Cout, Cin, tile, splits, ngate, raw_store, accum, with_grad, sp, i):
    rng = np.random.default_rng(400 + i)
    pr = grad_problem(rng, sp, Cin, Cout, k, 5)
    M, law = pr["M"], pr["law"]
    fg, fo = slice_forms(Cout)[i % 3], slice_forms(Cin)[(i + 1) % 3]
    fq = [slice_forms(Cin)[(i + q) % 3] for q in range(2)]
    gi = [gate_inputs(rng, M, Cin) for _ in range(ngate)]
    prior = rnd(rng, (M, Cin)) if accum else np.full((M, Cin), NANP, np.float32)
    raw0 = embed(prior, *fo)
    cap = -(-M // 64) + 2
    gates = [dict(y=embed(gi[q]["y"], *fq[q]), off_y=fq[q][1], out=np.full((M, fq[1 - q][0]), NANP, np.float32), off_out=fq[1 - q][1],
                  part=np.full((cap, Cin, 2), NANP, np.float32), **{kk: gi[q][kk] for kk in ("scale", "shift", "mean", "invstd")})
             for q in range(ngate)]
    grad = None
    if with_grad:
        grad = dict(y=embed(pr["y"], Cout, 0), off=0, coef=np.stack([law["k1"], law["k2"], law["k3"]]).astype(np.float32))
    with forced(tile, splits):
        res = fused().fused_conv("input_grad", sp + (Cin,), pr["w"], (1, 1, 1), raw0, off_out=fo[1], g=embed(pr["g"], *fg), off_g=fg[1],
                                 grad=grad, gates=gates, raw_store=bool(raw_store), accum=bool(accum))
    bm = check_name(res["kernels"], 3 if with_grad else 0, tile, Cin, gate=True)
    check_splits(res, splits, Cout, taps_of(k))       # (K-sliced: the folding block runs this epilogue)
    operand = ref.grad_operand(pr["g"], pr["y"], *grad["coef"]) if with_grad else pr["g"]
    v = ref.conv_input_grad(operand, pr["w"]).reshape(M, Cin)
    if accum:
        v = v + prior
    vscale = np.abs(v).max()
    rows = -(-M // bm)
    assert res["gpart_rows"] == rows, (res["gpart_rows"], rows, bm)
    gq = []
    for q in range(ngate):
        ldq, offq = fq[1 - q]
        out = res["gates"][q]["out"]
        outside_untouched(out, Cin, offq)
        g = inside(out, Cin, offq)
        mask = ref.gate_mask(gi[q]["y"], gi[q]["scale"], gi[q]["shift"])
        assert (g[~mask] == 0).all() and not np.signbit(g[~mask]).any(), "masked elements are exactly +0"
        close(g[mask], v[mask], what="gate %d passed" % q, scale=vscale)
        gq.append((g, mask))
        part = res["gates"][q]["part"]
        assert same_bits(part[rows:], np.full(part[rows:].shape, NANP, np.float32)), "partial rows beyond the launch's tiles changed"
        sums, mags = ref.gate_partials(g, gi[q]["y"], gi[q]["mean"], gi[q]["invstd"], bm)
        err = np.abs(part[:rows].astype(np.float64) - sums)
        bound = bm * EPS32 * np.maximum(mags, 1e-30)
        print("gate %d partials worst err / bound %.3g" % (q, (err / bound).max()))
        assert (err <= bound).all(), (q, (err / bound).max())
    if ngate == 2:
        both = gq[0][1] & gq[1][1]
        assert both.any() and same_bits(gq[0][0][both], gq[1][0][both]), "the two gates saw different values"
    if raw_store:
        outside_untouched(res["out"], Cin, fo[1])
        raw = inside(res["out"], Cin, fo[1])
        close(raw, v, what="raw", scale=vscale)
        for g, mask in gq:
            assert same_bits(raw[mask], g[mask]), "raw and gated results differ where the gate passes"
    else:
        assert same_bits(res["out"], raw0), "the raw buffer changed without raw_store"


# ---- e. filter gradients --------------------------------------------------------------------------------------------------------
def wgrad_problem(rng, sp, K, Nc, k, xt, dyt, i=0):
    """One filter-gradient problem with a K tail / an Nc tail, its float64 expectation included."""
    M = int(np.prod(sp))
    fx, fx2, fdy, fdy2 = slice_forms(K)[i % 3], slice_forms(K)[(i + 1) % 3], slice_forms(Nc)[(i + 2) % 3], slice_forms(Nc)[i % 3]
    x, dy = rnd(rng, sp + (K,)), rnd(rng, sp + (Nc,), 1.0, 0.5)
    pr = dict(x=embed(x, *fx), offx=fx[1], dy=embed(dy, *fdy), offdy=fdy[1], input_sizes=sp + (K,), filter_sizes=k + (K, Nc),
              strides=(1, 1, 1), dw=rnd(rng, k + (K, Nc)), xt=xt, dyt=dyt)
    a, b = x.astype(np.float64), dy.astype(np.float64)
    if xt:
        s1, t1 = published(rng, K)
        pr.update(xs1=s1, xt1=t1)
        if xt == 2:
            x2 = rnd(rng, sp + (K,))
            s2, t2 = published(rng, K)
            pr.update(x2=embed(x2, *fx2), offx2=fx2[1], xs2=s2, xt2=t2)
            a = ref.relu_operand(x, s1, t1, x2, s2, t2)
        else:
            a = ref.relu_operand(x, s1, t1)
    if dyt:
        y2 = rnd(rng, sp + (Nc,), 1.0, 0.7)
        coef = f32(np.stack([rng.uniform(0.5, 1.5, Nc), rng.standard_normal(Nc) * 0.3, rng.standard_normal(Nc) + 1.0]))
        pr.update(dy2=embed(y2, *fdy2), offdy2=fdy2[1], dcoef=coef)
        b = ref.grad_operand(dy, y2, *coef)
    pr["want"] = pr["dw"].astype(np.float64) + ref.conv_filter_grad(a, b, k)
    return pr


@pytest.mark.parametrize("tm,tn", [(64, 64), (128, 64), (64, 128), (128, 128)])
@pytest.mark.parametrize("xt,dyt", [(1, 0), (2, 0), (0, 1), (1, 1), (2, 1)])
def test_fused_filter_gradient(xt, dyt, tm, tn):
    i = xt * 2 + dyt + tm // 64 + tn // 32
    rng = np.random.default_rng(500 + i)
    k = KERNELS[i % 3]
    # a forced 128-row / 128-column tile applies from 128 reduction / output channels on (conv_wgrad2.hip plan()): 136 and 132
    # keep the K tail and the Nc tail there, 40 and 36 on the 64-wide tiles
    pr = wgrad_problem(rng, BIG if i % 4 else SMALL, 136 if tm == 128 else 40, 132 if tn == 128 else 36, k, xt, dyt, i)
    with forced(-1, 0, tm, tn):
        (got,), name, cuts, info = fused().fused_wgrad([pr])
    assert name == "wgrad2_kernel<%d,%d>" % (tm, tn) and info[1:] == (tm, tn), (name, info)
    close(got[0], pr["want"], what="xt %d dyt %d %s" % (xt, dyt, name))


def test_fused_filter_gradient_mixed_group():
    """One plain member, one xt = 2 member and one xt = 1 + dyt member in ONE launch."""
    rng = np.random.default_rng(77)
    prs = [wgrad_problem(rng, BIG, 64, 36, (1, 3, 3), 0, 0, 0), wgrad_problem(rng, BIG, 40, 64, (3, 1, 1), 2, 0, 1),
           wgrad_problem(rng, SMALL, 40, 132, (1, 1, 1), 1, 1, 2)]
    got, name, cuts, info = fused().fused_wgrad(prs)
    assert name == "wgrad2_kernel<64,64,fused>(grouped)" and all(c >= 1 for c in cuts), (name, cuts)
    for q, pr in enumerate(prs):
        close(got[q][0], pr["want"], what="group member %d" % q)


# ---- f. one chain on the device -------------------------------------------------------------------------------------------------
def test_chain_on_the_device():
    """conv_a -> (fold, RELU1) conv_b, then the gated input gradient of conv_b, the GRAD input gradient of conv_a and the dyt /
    xt filter gradients, every step fed with the hooks' own float32 outputs; against tests/fused_bn_ref.py composed on the same
    float32 y and gate inputs (the composition is tied to the oracle in tests/test_fused_bn_ref_cpu.py).  Outputs at TOL.
    dgamma / dbeta at 1e-4: they are sums over M = 392 rows of gated values held to TOL = 2e-5 of max |v|, so their error is at
    most M * 2e-5 * max |v| * max(1, max |xhat|) in the worst case and about sqrt(M) of that for independent errors, while the
    sums themselves are of the order sqrt(M) * rms(v) or more: 1e-4 of max |sum| leaves a factor of a few over the independent
    case and is what the issue sets."""
    ops = fused()
    rng = np.random.default_rng(5)
    C, ka, kb = 64, (1, 3, 3), (1, 1, 1)
    xs = BIG + (C,)
    M = 392
    x, wa, wb = rnd(rng, xs), rnd(rng, ka + (C, C), 0.1), rnd(rng, kb + (C, C), 0.2)
    gamma, beta = f32(rng.uniform(0.5, 1.5, C)), rnd(rng, C, 0.5)
    dz = rnd(rng, xs)
    y, _, _ = ops.conv_launch("forward", x, wa, (1, 1, 1), prior=NANP)
    close(y, ref.conv(x, wa), what="conv_a")
    parts = ref.partials_of(y.reshape(M, C), list(range(0, M, 64)) + [M])
    z0 = np.zeros(C, np.float32)
    fwd = ops.fused_conv("forward", xs, wb, (1, 1, 1), np.full((M, C), NANP, np.float32),
                         src=[dict(y=y.reshape(M, C), off=0, gamma=gamma, beta=beta, partials=parts, rows=M, publish=1, update_moving=0,
                                   scale=z0, shift=z0, mean=z0, invstd=z0, moving_mean=z0, moving_var=z0)])
    pub = fwd["src"][0]
    law = ref.fold(parts, M, gamma, beta)
    for kk in ("mean", "invstd", "scale", "shift"):
        coef_close(pub[kk], law[kk], law["terms"][kk], kk)
    close(fwd["out"].reshape(xs), ref.conv(ref.relu_operand(y, pub["scale"], pub["shift"]), wb), what="output")
    # backward of conv_b: gated by the BatchNorm's published values
    gate = dict(y=y.reshape(M, C), off_y=0, out=np.full((M, C), NANP, np.float32), off_out=0, part=np.full((9, C, 2), NANP, np.float32),
                **{kk: pub[kk] for kk in ("scale", "shift", "mean", "invstd")})
    bwd = ops.fused_conv("input_grad", xs, wb, (1, 1, 1), np.full((M, C), NANP, np.float32), g=dz.reshape(M, C), gates=[gate])
    bm = check_name(bwd["kernels"], 0, -1, C, gate=True)
    g, nrows = bwd["gates"][0]["out"], bwd["gpart_rows"]
    mask = fma32(pub["scale"], y.reshape(M, C), pub["shift"]) > 0             # the decisions on the hook's own float32 inputs
    v = ref.conv_input_grad(dz, wb).reshape(M, C)
    g_want = np.where(mask, v, 0.0)
    close(g, g_want, what="gated gradient")
    gparts = bwd["gates"][0]["part"][:nrows]
    # backward of conv_a: GRAD operand from those partials
    pre = dict(coef=np.zeros((3, C), np.float32), dgamma=z0, dbeta=z0)
    dxr = ops.fused_conv("input_grad", xs, wa, (1, 1, 1), np.full((M, C), NANP, np.float32), g=g,
                         grad=dict(y=y.reshape(M, C), off=0, gamma=gamma, mean=pub["mean"], invstd=pub["invstd"], partials=gparts, rows=M,
                                   publish=1, **pre))
    check_name(dxr["kernels"], 3, -1, C)
    sums, _ = ref.gate_partials(g_want, y.reshape(M, C), pub["mean"], pub["invstd"], bm)
    gl = ref.grad_fold(sums, M, gamma, pub["mean"], pub["invstd"])
    close(dxr["grad"]["dgamma"], gl["dgamma"], 1e-4, "dgamma")
    close(dxr["grad"]["dbeta"], gl["dbeta"], 1e-4, "dbeta")
    dy = ref.grad_operand(g_want.reshape(xs), y, gl["k1"], gl["k2"], gl["k3"])
    close(inside(dxr["out"], C, 0, xs), ref.conv_input_grad(dy, wa), what="dx")
    # filter gradients: dW_a through dyt (the coefficients the input gradient published), dW_b through xt = 1
    pa = dict(x=x.reshape(M, C), dy=g, input_sizes=xs, filter_sizes=ka + (C, C), strides=(1, 1, 1), dw=np.zeros(ka + (C, C), np.float32),
              dyt=1, dy2=y.reshape(M, C), dcoef=dxr["grad"]["coef"])
    pb = dict(x=y.reshape(M, C), dy=dz.reshape(M, C), input_sizes=xs, filter_sizes=kb + (C, C), strides=(1, 1, 1),
              dw=np.zeros(kb + (C, C), np.float32), xt=1, xs1=pub["scale"], xt1=pub["shift"])
    got, name, _, _ = ops.fused_wgrad([pa, pb])
    assert "fused" in name, name
    close(got[0][0], ref.conv_filter_grad(x, dy, ka), what="dW_a (dyt)")
    close(got[1][0], ref.conv_filter_grad(ref.relu_operand(y, pub["scale"], pub["shift"]), dz, kb), what="dW_b (xt)")


# ---- g. rejected launches ---------------------------------------------------------------------------------------------------------
HIP_ERROR_INVALID_VALUE = 1


@pytest.mark.parametrize("which", range(10))
def test_malformed_fused_launches_are_refused(which):
    """0 / 33 partials straight to a launcher (RELU1, GRAD), a gate beside a statistics sink, RELU1 with transposed weights,
    second row lengths that are no multiple of 4, xt / dyt with pair: hipErrorInvalidValue, and `false` from the validator."""
    err, ok = fused().fused_reject(which)
    assert err == HIP_ERROR_INVALID_VALUE, (which, err)
    assert ok == (which < 7), which


def test_gated_launch_on_a_strided_conv_is_the_builders_error():
    from sap3d_tensorflow_amd import P3dError
    rng = np.random.default_rng(3)
    C = 8
    gi = gate_inputs(rng, 8, C)
    gate = dict(y=gi["y"], off_y=0, out=np.zeros((8, C), np.float32), off_out=0, part=np.zeros((4, C, 2), np.float32),
                **{kk: gi[kk] for kk in ("scale", "shift", "mean", "invstd")})
    with pytest.raises(P3dError, match="stride-1"):
        fused().fused_conv("input_grad", (1, 1, 2, 4, C), rnd(rng, (1, 1, 1, C, C)), (1, 1, 2), np.zeros((8, C), np.float32),
                           g=rnd(rng, (4, C)), gates=[gate])
