"""The conv kernels (conv_igemm2.hip, conv_pointwise.hip, conv_wgrad2.hip) in the launch forms of the TRAIN STEP, op by op against
the float64 oracle (tests/conv_launch_ref.py).  tests/test_gpu_ops.py runs them dense, into zero-filled outputs, one filter
gradient per launch; the step does none of that (net_ops.inc conv() / deconv(), net.hip queue_wgrad / flush_wgrads):

  a. operands are channel slices of wider rows (the concat heads are written in place): results at TOL, and every float outside
     the slice BIT-identical to what the test put there -- a NaN with a payload, then a finite value (a neighbour that is read and
     folded in changes the result);
  b. outputs hold stale values: every non-accumulating case starts from NaN, none may remain, and the residue classes of a strided
     conv that no tap reaches hold exactly 0 (input gradient) / exactly the bias (transposed conv);
  c. gradients accumulate (accum = 1) through the tile epilogue, the folding block of a K-sliced launch, the K-sliced tail class
     and the streaming kernel; empty residue classes are then skipped (prior bit for bit); filter and bias gradients add to what
     they hold; max-pool backward accumulates;
  d. filter gradients go out in groups of up to 6 problems: cuts per problem, the shared slab stride, the 64x128 tile;
  e. the fp16 option of the 1x1x1 convs, against the rounded-operand reference at TOL (and NOT equal to the un-rounded one).

Tolerance: TOL = 2e-5 of the expected result's max magnitude (tests/test_gpu_ops.py), for accumulating cases of max |prior +
result|.  Every case that is about a path asserts the kernel name the hook reports.

The BatchNorm-fusion operand transforms and gated epilogues (at_mode, ngate, xt / dyt; off by default) have a file of their own:
  * tests/test_gpu_fused_ops.py, through the hooks p3d_debug_fused_conv / p3d_debug_fused_wgrad, against tests/fused_bn_ref.py:
    results at TOL, folded coefficients at 16 eps32 of their terms' magnitudes, gate partials at the float32 summation bound.
Not covered here: the attention GEMMs (tests/test_gpu_attention.py), RCCL."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conv_launch_ref as ref              # noqa: E402

from test_gpu_ops import CONV_CASES, DECONV_CASES, POOL_CASES              # noqa: E402,F401

pytestmark = pytest.mark.gpu

TOL = 2e-5
FILLS = [ref.nan_fill(), np.float32(3.25)]      # what lies outside a slice: a NaN with a payload, then a finite value


def close(got, want, tol=TOL, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(got).any(), (what, "NaN left", int(np.isnan(got).sum()))
    scale = max(np.abs(want).max(), 1e-30)
    err = np.abs(got.astype(np.float64) - want).max() / scale
    print("%s err %.3g (tol %.3g)" % (what, err, tol))
    assert err < tol, (what, err)


def untouched(outside, fill, what=""):
    assert ref.same_bits(outside, np.full(outside.shape, fill, np.float32)), (what, "floats outside the slice changed")


def rnd(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


def seed(*key):
    return abs(hash(key)) % (2 ** 31)


def slice_forms(C):
    """(ld, offset) of a C-channel slice: ld in {C, C + 4, 2C + 12}, offset in {0, 4, ld - C} where it fits."""
    out = []
    for ld in (C, C + 4, 2 * C + 12):
        for off in sorted({0, 4, ld - C}):
            if off + C <= ld:
                out.append((ld, off))
    return out


def slice_pairs(ci, co):
    """Gathered side and output side varied independently: every form of each side at least once, against several of the other."""
    a, b = slice_forms(ci), slice_forms(co)
    n = max(len(a), len(b))
    pairs = [(a[i % len(a)], b[(2 * i + 1) % len(b)]) for i in range(n)]
    pairs += [(a[0], b[-1]), (a[-1], b[0]), (a[-1], b[-1])]
    return list(dict.fromkeys(pairs))


def out_shape(xs, s, co):
    return (xs[0],) + tuple(-(-xs[1 + i] // s[i]) for i in range(3)) + (co,)


class forced:
    """p3d_debug_force_plan for the duration of a with block."""
    def __init__(self, tile=-1, splits=0, tm=0, tn=0):
        self.args = (tile, splits, tm, tn)

    def __enter__(self):
        from sap3d_tensorflow_amd import lib
        lib().p3d_debug_force_plan(*self.args)

    def __exit__(self, *exc):
        from sap3d_tensorflow_amd import lib
        lib().p3d_debug_force_plan(-1, 0, 0, 0)


def _launch(*args, **kw):
    """ops.conv_launch with the payload NaN outside the slices unless the case says otherwise."""
    from sap3d_tensorflow_amd import ops
    kw.setdefault("pad", FILLS[0])
    out = ops.conv_launch(*args, **kw)
    _launch.splits = ops.conv_launch.last_splits          # (smallest, largest) K-slice count of the launches' plans
    return out


def k_sliced(forced_splits, K, taps=1):
    """The kernel names do not carry the K-slice count; the hook reports it.  A forced count applies where the launch has that
    many K steps (32 channels each per tap; p3d_igemm2_plan ignores a larger one): then every launch with taps must have it."""
    steps = taps * -(-K // 32)
    if forced_splits and steps >= forced_splits:
        assert _launch.splits[1] == forced_splits, (_launch.splits, forced_splits, steps)
        return True
    return False


TILE_NAMES = {0: "<64,64", 1: "<128,64", 2: "<128,128"}

# ---- a. + b.: slices, into outputs that hold NaN ----------------------------------------------------------------------------------
# from CONV_CASES and test_filter_gradient_tile_shapes (no stem: it has its own entry points); Nc = 256 / 64 (tile multiples),
# 48, 12, 132, 24 (ragged multiples of 4)
SLICE_CASES = [
    ((2, 4, 12, 12, 64), (1, 1, 1), 256, (1, 1, 1)),
    ((1, 4, 13, 11, 32), (1, 1, 1), 48, (1, 2, 2)),
    ((2, 4, 12, 12, 64), (1, 3, 3), 64, (1, 1, 1)),
    ((1, 3, 9, 10, 20), (3, 3, 3), 12, (1, 1, 1)),
    ((3, 2, 9, 7, 136), (1, 1, 1), 132, (1, 1, 1)),
    ((1, 4, 10, 10, 16), (3, 3, 3), 24, (2, 2, 2)),
]


@pytest.mark.parametrize("xs,k,co,s", SLICE_CASES)
def test_conv_forward_on_channel_slices(xs, k, co, s):
    rng = np.random.default_rng(seed(xs, k, co, s))
    x, w, b = rnd(rng, xs), rnd(rng, k + (xs[4], co)) * 0.1, rnd(rng, (co,))
    want = ref.forward(x, w, s, b)
    for (fi, fo) in slice_pairs(xs[4], co):
        for fill in FILLS:
            what = "fwd in %s out %s fill %s" % (fi, fo, fill)
            got, outside, names = _launch("forward", x, w, s, bias=b, ld=(fi[0], fo[0]), offset=(fi[1], fo[1]), pad=fill)
            close(got, want, what=what)
            untouched(outside, fill, what)


@pytest.mark.parametrize("xs,k,co,s", SLICE_CASES)
def test_conv_input_gradient_on_channel_slices(xs, k, co, s):
    """dx written (accum = 0) into NaN: the residue classes of a strided conv that no tap reaches must be written too, with 0."""
    rng = np.random.default_rng(seed(xs, k, co, s, 1))
    w = rnd(rng, k + (xs[4], co)) * 0.1
    dy = rnd(rng, out_shape(xs, s, co))
    want = ref.input_grad(dy, w, s, xs)
    empty = ref.empty_mask(xs, k, s)
    assert empty.any() == any(kk < ss for kk, ss in zip(k, s))
    for (fo, fi) in slice_pairs(xs[4], co):          # the gathered side is dy (co channels), the output dx (Cin)
        for fill in FILLS:
            what = "dgrad in %s out %s fill %s" % (fi, fo, fill)
            got, outside, names = _launch("input_grad", dy, w, s, input_sizes=xs, ld=(fi[0], fo[0]), offset=(fi[1], fo[1]), pad=fill)
            close(got, want, what=what)
            untouched(outside, fill, what)
            assert ref.same_bits(got[:, empty], np.zeros_like(got[:, empty])), what


@pytest.mark.parametrize("xs,k,co,s", DECONV_CASES)
def test_conv_transpose_on_channel_slices(xs, k, co, s):
    """The transposed conv's forward; where k < s the positions no tap reaches hold exactly the bias."""
    rng = np.random.default_rng(seed(xs, k, co, s, 2))
    x, kern, b = rnd(rng, xs), rnd(rng, k + (co, xs[4])) * 0.1, rnd(rng, (co,))
    want = ref.transpose(x, kern, s, b)
    empty = ref.empty_mask(want.shape, k, s)
    assert empty.any() == any(kk < ss for kk, ss in zip(k, s))
    for (fi, fo) in slice_pairs(xs[4], co):
        for fill in FILLS:
            what = "deconv in %s out %s fill %s" % (fi, fo, fill)
            got, outside, names = _launch("transpose", x, kern, s, bias=b, ld=(fi[0], fo[0]), offset=(fi[1], fo[1]), pad=fill)
            close(got, want, what=what)
            untouched(outside, fill, what)
            assert ref.same_bits(got[:, empty], np.broadcast_to(b, got[:, empty].shape)), what
    got, _, _ = _launch("transpose", x, kern, s, bias=None)
    close(got, want - b.astype(np.float64), what="no bias")
    assert ref.same_bits(got[:, empty], np.zeros_like(got[:, empty]))


def _wgrad_want(pr):
    """float64 (dw, dbias or None) of a wgrad_group problem, priors included."""
    if pr.get("transpose"):
        dw = ref.transpose_filter_grad(pr["x"], pr["dy"], pr["filter_sizes"], pr["strides"])
    else:
        dw = ref.filter_grad(pr["x"], pr["dy"], pr["filter_sizes"], pr["strides"])
    if pr.get("dw") is not None:
        dw = dw + np.asarray(pr["dw"], np.float64)
    db = None
    if pr.get("dbias") is not None:
        db = np.asarray(pr["dy"], np.float64).reshape(-1, pr["dy"].shape[-1]).sum(0) + np.asarray(pr["dbias"], np.float64)
    return dw, db


def _wgrad_check(got, want, what):
    (dw, db), (wdw, wdb) = got, want
    if wdw.size:
        close(dw, wdw, what=what + " dw")
    if wdb is not None:
        close(db, wdb, what=what + " dbias")
    else:
        assert db is None


@pytest.mark.parametrize("xs,k,co,s", SLICE_CASES)
def test_filter_gradient_on_channel_slices(xs, k, co, s):
    """One problem per launch, x and dy as slices, dw and dbias ADDED to a random prior."""
    from sap3d_tensorflow_amd import ops
    rng = np.random.default_rng(seed(xs, k, co, s, 3))
    x, dy = rnd(rng, xs), rnd(rng, out_shape(xs, s, co))
    fs = k + (xs[4], co)
    base = dict(x=x, dy=dy, filter_sizes=fs, strides=s, dw=rnd(rng, fs) * 10, dbias=rnd(rng, (co,)) * 10)
    want = _wgrad_want(base)
    for (fi, fo) in slice_pairs(xs[4], co):
        for fill in FILLS:
            pr = dict(base, ld=(fi[0], fo[0]), offset=(fi[1], fo[1]))
            res, name, cuts, info = ops.wgrad_group([pr], pad=fill)
            _wgrad_check(res[0], want, "wgrad x %s dy %s fill %s %s cuts %s" % (fi, fo, fill, name, cuts))
            assert cuts[0] >= 1 and info[0] == cuts[0]


# ---- b.: the ragged last tile, K-sliced tiles, the tail class -- into NaN ------------------------------------------------------------
@pytest.mark.parametrize("tile", [0, 1, 2])
@pytest.mark.parametrize("splits", [0, 2, 4])
def test_forced_tiles_and_k_slices_leave_no_element_unwritten(tile, splits):
    """1183 output rows (a ragged last M tile for 64 and 128) x 132 channels on every forced tile, whole and K-sliced, forward and
    input gradient, written into NaN; the strided 1x1x1 input gradient (ids 3, 11 of the network) with its three empty classes."""
    xs, k, co, s = (1, 7, 13, 13, 72), (1, 3, 3), 132, (1, 1, 1)
    rng = np.random.default_rng(seed(tile, splits))
    x, w, b = rnd(rng, xs), rnd(rng, k + (xs[4], co)) * 0.1, rnd(rng, (co,))
    dy = rnd(rng, out_shape(xs, s, co))
    with forced(tile, splits):
        got, outside, names = _launch("forward", x, w, s, bias=b, ld=(None, 2 * co + 12), offset=(0, 4))
        assert k_sliced(splits, xs[4], 9) == (splits > 0) and (splits == 0 or _launch.splits[0] == splits)
        gdx, odx, ndx = _launch("input_grad", dy, w, s, input_sizes=xs, ld=(None, xs[4] + 4), offset=(0, 4))
        assert k_sliced(splits, co, 9) == (splits > 0) and (splits == 0 or _launch.splits[0] == splits)
    assert TILE_NAMES[tile] in names and TILE_NAMES[tile] in ndx, (names, ndx)
    close(got, ref.forward(x, w, s, b), what="fwd " + names)
    untouched(outside, FILLS[0])
    close(gdx, ref.input_grad(dy, w, s, xs), what="dgrad " + ndx)
    untouched(odx, FILLS[0])
    xs2, co2, s2 = (2, 4, 14, 14, 256), 128, (1, 2, 2)
    w2 = rnd(rng, (1, 1, 1, xs2[4], co2)) * 0.1
    dy2 = rnd(rng, out_shape(xs2, s2, co2))
    with forced(tile, splits):
        g2, _, n2 = _launch("input_grad", dy2, w2, s2, input_sizes=xs2)
        assert k_sliced(splits, co2) == (splits > 0)          # the class with a tap: 128 channels = 4 steps (the empty ones have none)
    close(g2, ref.input_grad(dy2, w2, s2, xs2), what="strided dgrad " + n2)
    empty = ref.empty_mask(xs2, (1, 1, 1), s2)
    assert empty.sum() * 4 == empty.size * 3
    assert ref.same_bits(g2[:, empty], np.zeros_like(g2[:, empty]))


# ---- c.: accumulation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [0, 1, 2])
@pytest.mark.parametrize("splits", [0, 2, 4])
def test_accumulating_epilogues_of_every_tile_and_of_k_sliced_launches(tile, splits):
    """accum = 1 onto a random prior: the tile epilogue (splits 0: the plan's choice for the forced tile) and the folding block of
    a K-sliced launch (2, 4), as conv()'s input gradient and as deconv()'s (the forward builder with accum)."""
    xs, k, co, s = (2, 4, 14, 14, 256), (1, 3, 3), 128, (1, 1, 1)
    rng = np.random.default_rng(seed(tile, splits, 7))
    x, w = rnd(rng, xs), rnd(rng, k + (xs[4], co)) * 0.1
    dy = rnd(rng, out_shape(xs, s, co))
    pf, pg = rnd(rng, dy.shape) * 3, rnd(rng, xs) * 3
    with forced(tile, splits):
        got, outside, names = _launch("forward", x, w, s, accum=True, prior=pf, ld=(None, co + 4), offset=(0, 4))
        assert k_sliced(splits, xs[4], 9) == (splits > 0) and (splits == 0 or _launch.splits[0] == splits)
        gdx, odx, ndx = _launch("input_grad", dy, w, s, input_sizes=xs, accum=True, prior=pg, ld=(None, 2 * xs[4] + 12), offset=(0, xs[4] + 12))
        assert k_sliced(splits, co, 9) == (splits > 0) and (splits == 0 or _launch.splits[0] == splits)
    assert TILE_NAMES[tile] in names and TILE_NAMES[tile] in ndx, (names, ndx)
    close(got, ref.accumulated(pf, ref.forward(x, w, s)), what="fwd+= " + names)
    untouched(outside, FILLS[0])
    close(gdx, ref.accumulated(pg, ref.input_grad(dy, w, s, xs)), what="dgrad+= " + ndx)
    untouched(odx, FILLS[0])


def test_accumulating_tail_split_class():
    """(1, 8, 66, 64, 32) -> 128: 33792 rows, a few tiles over a multiple of the 256 CUs, whose last round goes out K-sliced
    (test_conv_last_round_is_k_sliced); the deconv()-style accumulating forward, and the same launch into NaN."""
    xs, k, co, s = (1, 8, 66, 64, 32), (3, 3, 3), 128, (1, 1, 1)
    rng = np.random.default_rng(17)
    x, w, b = rnd(rng, xs), rnd(rng, k + (xs[4], co)) * 0.1, rnd(rng, (co,))
    want = ref.forward(x, w, s, b)
    prior = rnd(rng, want.shape) * 3
    with forced(1):
        got, outside, names = _launch("forward", x, w, s, bias=b, accum=True, prior=prior, ld=(None, co + 4), offset=(0, 0))
    assert names.endswith("(tail)"), names
    close(got, ref.accumulated(prior, want), what="tail += " + names)
    untouched(outside, FILLS[0])
    with forced(1):
        got, outside, names = _launch("forward", x, w, s, bias=b, ld=(None, co + 4), offset=(0, 4))
    assert names.endswith("(tail)"), names
    close(got, want, what="tail = " + names)
    untouched(outside, FILLS[0])


@pytest.mark.parametrize("xs,ci,co", [((2, 8, 32, 33), 256, 64), ((2, 16, 32, 32), 64, 64)])
def test_streaming_kernel_accumulates_and_keeps_to_its_slice(xs, ci, co):
    """>= 16384 rows, 64 gathered channels (pw_shape, conv_pointwise.hip): the input gradient of a conv to 64 channels runs on
    pw_stream_kernel and stores straight from the accumulators (pw_store_slab): accum = 1 onto a random prior and accum = 0
    into NaN, the output a slice of a wider row (16896 rows = 528 slabs of 32 on 512 blocks; 32768 rows)."""
    xs = xs + (ci,)
    rng = np.random.default_rng(3)
    w = rnd(rng, (1, 1, 1, ci, co)) * 0.2
    dy = rnd(rng, xs[:4] + (co,))
    want = ref.input_grad(dy, w, (1, 1, 1), xs)
    prior = rnd(rng, xs) * 3
    for fill in FILLS:
        got, outside, names = _launch("input_grad", dy, w, (1, 1, 1), input_sizes=xs, accum=True, prior=prior, ld=(None, ci + 4), offset=(0, 4), pad=fill)
        assert names == "pw_stream_kernel", names
        close(got, ref.accumulated(prior, want), what="stream += ")
        untouched(outside, fill)
        got, outside, names = _launch("input_grad", dy, w, (1, 1, 1), input_sizes=xs, ld=(None, 2 * ci + 12), offset=(0, ci + 12), pad=fill)
        assert names == "pw_stream_kernel", names
        close(got, want, what="stream = ")
        untouched(outside, fill)
    if ci == 64:        # the forward of a 64 -> 64 conv streams as well (weights in registers)
        x, b = rnd(rng, xs), rnd(rng, (co,))
        pf = rnd(rng, xs[:4] + (co,)) * 3
        got, outside, names = _launch("forward", x, w, (1, 1, 1), bias=b, accum=True, prior=pf, ld=(ci + 4, co + 4), offset=(4, 0))
        assert names == "pw_stream_kernel", names
        close(got, ref.accumulated(pf, ref.forward(x, w, (1, 1, 1), b)), what="stream fwd += ")
        untouched(outside, FILLS[0])


STRIDED = [c for c in CONV_CASES if max(c[3]) > 1 and c[0][4] % 4 == 0]


@pytest.mark.parametrize("xs,k,co,s", STRIDED)
def test_accumulating_residue_classes_skip_the_empty_ones(xs, k, co, s):
    """The input gradient of every strided conv of CONV_CASES with accum = 1: classes with taps add to the prior, classes
    without (1x1x1 at stride 2: three of four) are not launched -- those positions keep the prior bit for bit."""
    rng = np.random.default_rng(seed(xs, k, co, s, 4))
    w = rnd(rng, k + (xs[4], co)) * 0.1
    dy = rnd(rng, out_shape(xs, s, co))
    prior = rnd(rng, xs) * 3
    want = ref.accumulated(prior, ref.input_grad(dy, w, s, xs))
    empty = ref.empty_mask(xs, k, s)
    cls = ((np.arange(xs[1]) % s[0])[:, None, None] * 64 + (np.arange(xs[2]) % s[1])[None, :, None] * 8
           + (np.arange(xs[3]) % s[2])[None, None, :])
    live = len(np.unique(cls[~empty]))          # residue classes that some tap reaches
    for fill in FILLS:
        got, outside, names = _launch("input_grad", dy, w, s, input_sizes=xs, accum=True, prior=prior, ld=(co + 4, xs[4] + 4), offset=(4, 0), pad=fill)
        assert len(names.split(";")) in (1, live), (names, live)          # one grouped launch, or one per class with taps
        close(got, want, what="classes += " + names)
        untouched(outside, fill)
        assert ref.same_bits(got[:, empty], prior[:, empty])


@pytest.mark.parametrize("tile", ["64x64", "64x128", "128x64", "128x128"])
@pytest.mark.parametrize("xs,k,co", [((2, 4, 14, 14, 256), (1, 3, 3), 128), ((3, 2, 9, 7, 136), (1, 1, 1), 132)])
def test_filter_and_bias_gradient_add_to_what_they_hold(tile, xs, k, co):
    """p3d_kernels.h: 'the launch ADDS the gradient' -- a random prior in dw and dbias, one problem on each forced tile (the
    problems of test_filter_gradient_tile_shapes), bit-identical run to run."""
    from sap3d_tensorflow_amd import ops
    tm, tn = (int(v) for v in tile.split("x"))
    rng = np.random.default_rng(5)
    x, dy = rnd(rng, xs), rnd(rng, xs[:4] + (co,))
    fs = k + (xs[4], co)
    pr = dict(x=x, dy=dy, filter_sizes=fs, strides=(1, 1, 1), dw=rnd(rng, fs) * 20, dbias=rnd(rng, (co,)) * 20)
    with forced(-1, 0, tm, tn):
        res, name, cuts, info = ops.wgrad_group([pr])
        again, _, _, _ = ops.wgrad_group([pr])
    assert name == "wgrad2_kernel<%d,%d>" % (tm, tn) and info[1:] == (tm, tn), (name, info)
    _wgrad_check(res[0], _wgrad_want(pr), "wgrad += %s cuts %s" % (name, cuts))
    assert ref.same_bits(res[0][0], again[0][0]) and ref.same_bits(res[0][1], again[0][1])


@pytest.mark.parametrize("xs,k,s", POOL_CASES)
def test_max_pool_on_slices_and_accumulating_backward(xs, k, s):
    from sap3d_tensorflow_amd import ops
    from oracle import nn
    rng = np.random.default_rng(7)
    x = np.maximum(rnd(rng, xs), 0)
    C_ = xs[4]
    t = nn.Tape()
    X = nn.Var(x.astype(np.float64))
    Y = nn.max_pool3d(t, X, k, s)
    dy = rnd(rng, Y.data.shape)
    Y.grad = dy.astype(np.float64)
    t.ops[-1]()
    disjoint = tuple(k) == tuple(s) and all(i % ss == 0 for i, ss in zip(xs[1:4], s))
    prior = rnd(rng, xs) * 3
    for (fx, fy) in slice_pairs(C_, C_):
        for fill in FILLS:
            ld, off = (fx[0], fy[0]), (fx[1], fy[1])
            y, outside = ops.max_pool3d_launch(x, k, s, ld=ld, offset=off, pad=fill)
            assert np.array_equal(y, Y.data.astype(np.float32))
            untouched(outside, fill)
            dx, outside, kern = ops.max_pool3d_grad_launch(x, k, s, dy, ld=ld, offset=off, pad=fill)
            assert kern == ("maxpool_bwd_disjoint_kernel" if disjoint else "maxpool_bwd_gather_kernel")
            close(dx, X.grad, what="pool grad = " + kern)
            untouched(outside, fill)
            dx, outside, kern = ops.max_pool3d_grad_launch(x, k, s, dy, accumulate=True, prior=prior, ld=ld, offset=off, pad=fill)
            close(dx, ref.accumulated(prior, X.grad), what="pool grad += " + kern)
            untouched(outside, fill)


@pytest.mark.parametrize("rows,c", [(17, 64), (5000, 64), (3001, 1024), (777, 6), (50, 2048)])
def test_bias_gradient_on_a_slice_adds_to_its_prior(rows, c):
    """deconv()'s bias gradient: p3d_colsum(y->g, y->ld, ...) adds the column sums of a slice to what dbias holds."""
    from sap3d_tensorflow_amd import ops
    rng = np.random.default_rng(rows * 131 + c)
    dy = rnd(rng, (rows, c))
    prior = rnd(rng, (c,)) * 10
    want = dy.astype(np.float64).sum(0) + prior
    scale = np.abs(dy.astype(np.float64)).sum(0).max()
    step = 4 if c % 4 == 0 else 2
    for ld, off in [(c, 0), (c + step, step), (2 * c + 3 * step, c + 3 * step)]:
        for fill in FILLS:
            got = ops.bias_add_grad_launch(dy, ld=ld, offset=off, pad=fill, prior=prior)
            assert np.abs(got - want).max() <= 2e-6 * max(scale, 1.0), (ld, off)        # the bound of test_bias_add_grad


# ---- d.: grouped filter gradients ---------------------------------------------------------------------------------------------------
def _problem(rng, xs, k, co, s=(1, 1, 1), ld=(None, None), offset=(0, 0), bias=False, prior=True, transpose=False):
    x = rnd(rng, xs)
    if transpose:
        dy = rnd(rng, (xs[0], xs[1] * s[0], xs[2] * s[1], xs[3] * s[2], co))
        fs = tuple(k) + (co, xs[4])
    else:
        dy = rnd(rng, out_shape(xs, s, co))
        fs = tuple(k) + (xs[4], co)
    return dict(x=x, dy=dy, filter_sizes=fs, strides=s, ld=ld, offset=offset, transpose=transpose,
                dw=rnd(rng, fs) * 5 if prior else None, dbias=rnd(rng, (co,)) * 5 if bias else None)


def _group_check(probs, expect_name=None, **flags):
    """One grouped launch: each member against float64, the launch repeated bit for bit, and each member launched alone as the
    second witness (grouped and single differ in the order of the cuts only)."""
    from sap3d_tensorflow_amd import ops
    res, name, cuts, info = ops.wgrad_group(probs, **flags)
    print("group %s cuts %s info %s" % (name, cuts, info))
    if expect_name is not None:
        assert name == expect_name, name
    again, name2, cuts2, info2 = ops.wgrad_group(probs, **flags)
    assert (name2, cuts2, info2) == (name, cuts, info)
    live = [c for c in cuts if c > 0]
    assert info[0] == (max(live) if live else 1)
    for i, pr in enumerate(probs):
        rows = int(np.prod(pr["x"].shape[:4])) if not pr.get("transpose") else int(np.prod(pr["dy"].shape[:4]))
        dead = rows == 0 or int(np.prod(pr["filter_sizes"][:3])) == 0
        assert (cuts[i] == 0) == dead, (i, cuts)
        assert ref.same_bits(res[i][0], again[i][0]), i
        if res[i][1] is not None:
            assert ref.same_bits(res[i][1], again[i][1]), i
        if dead:        # dropped from the launch: the gradients keep what they held
            assert ref.same_bits(res[i][0], np.zeros(pr["filter_sizes"], np.float32) if pr["dw"] is None else pr["dw"])
            assert res[i][1] is None or ref.same_bits(res[i][1], pr["dbias"])
            continue
        want = _wgrad_want(pr)
        _wgrad_check(res[i], want, "member %d" % i)
        single, _, _, _ = ops.wgrad_group([pr], **flags)
        _wgrad_check(single[0], want, "member %d alone" % i)
        close(res[i][0], single[0][0].astype(np.float64), what="member %d grouped vs alone" % i)
    return name, cuts, info


def _bottleneck(rng, n, d, h, w, cin, planes, project=True):
    """The filter gradients one bottleneck queues (conv() backward, last conv first): 1x1x1 expand, 3x1x1, 1x3x3, 1x1x1 reduce,
    and the strided 1x1x1 projection of a stage's first block (from the tensor of the stage before)."""
    lat = (n, d, h, w)
    out = [_problem(rng, lat + (planes,), (1, 1, 1), 4 * planes),
           _problem(rng, lat + (planes,), (3, 1, 1), planes),
           _problem(rng, lat + (planes,), (1, 3, 3), planes),
           _problem(rng, lat + (cin,), (1, 1, 1), planes)]
    if project:
        out.append(_problem(rng, (n, d, 2 * h, 2 * w, cin), (1, 1, 1), 4 * planes, s=(1, 2, 2)))
    return out


# stages 1-3 at 2 clips of 16x112x112 (28x28, 14x14, 7x7 lattices), a quarter of the width
@pytest.mark.parametrize("stage,lat,cin,planes", [(1, (2, 8, 28, 28), 16, 16), (2, (2, 4, 14, 14), 64, 32), (3, (2, 2, 7, 7), 128, 64)])
def test_grouped_filter_gradients_of_one_bottleneck(stage, lat, cin, planes):
    rng = np.random.default_rng(100 + stage)
    probs = _bottleneck(rng, *lat, cin, planes)
    name, cuts, info = _group_check(probs, expect_name="wgrad2_kernel<64,64>(grouped)")
    assert info[1:] == (64, 64)


@pytest.mark.parametrize("long_first", [False, True])
def test_grouped_filter_gradients_across_a_stage_boundary_share_a_slab_stride(long_first):
    """The queue packs across stage boundaries: stage 2's first bottleneck (1568 positions, with its projection) and stage 1's
    last expand conv (12544 positions).  The balancing rule cuts the long member further, so the members differ in cuts and
    the slab of (slot, cut) is slot * kstride + cut with kstride the LARGEST cut count.  An index by the member's own cut
    count puts the slabs of a member with few cuts onto those of a member with many cuts that sits BEFORE it in the group
    (slot * 10 + cut < 64 * slots before it), so the long member comes first as well as last."""
    rng = np.random.default_rng(200)
    long_one = [_problem(rng, (2, 8, 28, 28, 16), (1, 1, 1), 64)]
    rest = _bottleneck(rng, 2, 4, 14, 14, 64, 32)
    probs = long_one + rest if long_first else rest + long_one
    name, cuts, info = _group_check(probs)
    assert len(probs) == 6 and len(set(cuts)) >= 2 and info[0] > 1, (cuts, info)
    longest = cuts[0] if long_first else cuts[5]
    assert longest == max(cuts) and longest > min(cuts), cuts          # the balancing rule cut the long member further


def test_grouped_filter_gradients_on_the_64x128_tile():
    """Every member over >= 2048 positions, to a multiple of 128 channels, with >= 9 taps: the group takes the 64x128 tile
    (group_takes_rect, the unet++ head's nodes); one 1x1x1 member and it stays on 64x64."""
    rng = np.random.default_rng(300)
    lat = (1, 4, 24, 24)          # 2304 positions
    probs = [_problem(rng, lat + (32,), (1, 3, 3), 128, bias=True), _problem(rng, lat + (16,), (3, 3, 3), 128),
             _problem(rng, lat + (24,), (1, 3, 3), 256, ld=(28, 268), offset=(4, 12))]
    name, cuts, info = _group_check(probs, expect_name="wgrad2_kernel<64,128>(grouped)")
    assert info[1:] == (64, 128)
    probs.append(_problem(rng, lat + (32,), (1, 1, 1), 128))
    name, cuts, info = _group_check(probs, expect_name="wgrad2_kernel<64,64>(grouped)")
    assert info[1:] == (64, 64)


@pytest.mark.parametrize("polite,greedy", [(False, False), (True, False), (False, True)])
def test_grouped_filter_gradients_members_slices_and_flags(polite, greedy):
    """6 members (the maximum) on slices of different row lengths, bias gradients on some only, a transposed conv's problem
    (deconv()), under each residency flag; 2 members; members without rows / without taps are dropped and keep their priors."""
    from sap3d_tensorflow_amd import ops
    rng = np.random.default_rng(400)
    lat = (2, 2, 7, 7)
    six = [_problem(rng, lat + (64,), (1, 1, 1), 132, ld=(68, 144), offset=(4, 12), bias=True),
           _problem(rng, lat + (48,), (1, 3, 3), 64, ld=(108, 64), offset=(60, 0)),
           _problem(rng, lat + (64,), (3, 1, 1), 48, ld=(64, 52), offset=(0, 4), bias=True, prior=False),
           _problem(rng, (1, 2, 6, 5, 32), (3, 3, 3), 16, s=(2, 2, 2), transpose=True, ld=(36, 44), offset=(0, 28)),
           _problem(rng, (2, 2, 14, 14, 24), (1, 1, 1), 64, s=(1, 2, 2), ld=(60, 68), offset=(36, 4), bias=True),
           _problem(rng, (1, 4, 10, 10, 16), (3, 3, 3), 24, s=(2, 2, 2))]
    _group_check(six, expect_name="wgrad2_kernel<64,64>(grouped)", polite=polite, greedy=greedy)
    _group_check(six[:2], expect_name="wgrad2_kernel<64,64>(grouped)", polite=polite, greedy=greedy)
    dead = [_problem(rng, (0, 2, 7, 7, 16), (1, 3, 3), 16, bias=True), six[1], _problem(rng, (1, 2, 4, 4, 8), (0, 3, 3), 8), six[0]]
    _group_check(dead, polite=polite, greedy=greedy)
    with pytest.raises(Exception):
        ops.wgrad_group(six + six[:1])


# ---- e.: the fp16 option of the 1x1x1 convs ---------------------------------------------------------------------------------------------
def _f16_names_ok(names):
    """No streaming kernel, and the f16 marker on every single launch (a grouped launch's name carries none: there only the
    numbers tell)."""
    for n in names.split(";"):
        assert n != "pw_stream_kernel" and (",f16>" in n or n.startswith("igemm2_group_kernel")), names


def _f16_check(got, rounded, exact, what):
    """At TOL of the rounded-operand reference, and more than 10 x TOL from the un-rounded one (the references themselves differ
    by more than 10 x TOL: asserted before the GPU is asked)."""
    scale = np.abs(rounded).max()
    close(got, rounded, what=what)
    far = np.abs(got.astype(np.float64) - exact).max() / scale
    print("%s distance from the un-rounded reference %.3g" % (what, far))
    assert far > 10 * TOL, (what, far)


@pytest.mark.parametrize("K,N", [(64, 256), (256, 64), (32, 48), (256, 128)])
@pytest.mark.parametrize("s", [(1, 1, 1), (1, 2, 2)])
def test_fp16_pointwise_against_rounded_operands(K, N, s):
    """4096 rows (1024 output rows when strided), operand magnitudes in [2^-6, 4] (weights x 0.1): no fp16 subnormals."""
    rng = np.random.default_rng(K * 1000 + N + s[1])
    xs = (1, 4, 32, 32, K)
    x, w, b = ref.draw16(rng, xs), ref.draw16(rng, (1, 1, 1, K, N), 0.1), rnd(rng, (N,))
    dy = ref.draw16(rng, out_shape(xs, s, N))
    fwd16, fwd = ref.forward(x, w, s, b, f16=True), ref.forward(x, w, s, b)
    dx16, dx = ref.input_grad(dy, w, s, xs, f16=True), ref.input_grad(dy, w, s, xs)
    assert np.abs(fwd16 - fwd).max() > 10 * TOL * np.abs(fwd16).max()          # from the references alone
    assert np.abs(dx16 - dx).max() > 10 * TOL * np.abs(dx16).max()
    empty = ref.empty_mask(xs, (1, 1, 1), s)
    for (fi, fo) in [((K, 0), (N, 0)), ((K + 4, 4), (2 * N + 12, N + 12))]:
        got, outside, names = _launch("forward", x, w, s, bias=b, f16=True, ld=(fi[0], fo[0]), offset=(fi[1], fo[1]))
        _f16_names_ok(names)
        _f16_check(got, fwd16, fwd, "f16 fwd %s %s %s" % (fi, fo, names))
        untouched(outside, FILLS[0])
        g, outside, names = _launch("input_grad", dy, w, s, input_sizes=xs, f16=True, ld=(fo[0], fi[0]), offset=(fo[1], fi[1]))
        _f16_names_ok(names)
        _f16_check(g, dx16, dx, "f16 dgrad %s %s %s" % (fi, fo, names))
        untouched(outside, FILLS[0])
        assert ref.same_bits(g[:, empty], np.zeros_like(g[:, empty]))
    # accumulation, and K-sliced (forced splits 2: the folding block's epilogue) where the reduction has two steps of 32 channels
    # -- every launch here but the forward of the K = 32 case, which stays whole
    prior = ref.draw16(rng, xs)
    for splits in (0, 2):
        with forced(-1 if splits == 0 else 0, splits):
            g, _, names = _launch("input_grad", dy, w, s, input_sizes=xs, f16=True, accum=True, prior=prior)
            assert k_sliced(splits, N) == (splits > 0)
            got, _, n2 = _launch("forward", x, w, s, bias=b, f16=True)
            assert k_sliced(splits, K) == (splits > 0 and K >= 64)
        _f16_names_ok(names)
        _f16_names_ok(n2)
        close(g, ref.accumulated(prior, dx16), what="f16 dgrad += splits %d %s" % (splits, names))
        assert ref.same_bits(g[:, empty], prior[:, empty])
        _f16_check(got, fwd16, fwd, "f16 fwd splits %d %s" % (splits, n2))
    with pytest.raises(Exception):
        _launch("forward", x[..., :16], rnd(rng, (1, 3, 3, 16, 8)), (1, 1, 1), f16=True)


def test_fp16_pointwise_over_many_rows_stays_on_the_tiled_kernel():
    """>= 16384 rows, 64 -> 64: without f16 this launch streams (pw_stream_kernel has no fp16 form, conv_pointwise.hip); with it
    the tiled fp16 kernel must take it."""
    rng = np.random.default_rng(9)
    xs = (1, 16, 32, 32, 64)
    x, w = ref.draw16(rng, xs), ref.draw16(rng, (1, 1, 1, 64, 64), 0.1)
    f16, f = ref.forward(x, w, (1, 1, 1), f16=True), ref.forward(x, w, (1, 1, 1))
    assert np.abs(f16 - f).max() > 10 * TOL * np.abs(f16).max()
    got, _, names = _launch("forward", x, w, (1, 1, 1))
    assert names == "pw_stream_kernel", names
    close(got, f, what="fp32 " + names)
    got, _, names = _launch("forward", x, w, (1, 1, 1), f16=True)
    _f16_names_ok(names)
    _f16_check(got, f16, f, "f16 " + names)
    g, _, names = _launch("input_grad", x, w, (1, 1, 1), input_sizes=xs, f16=True)
    _f16_names_ok(names)
    _f16_check(g, ref.input_grad(x, w, (1, 1, 1), xs, f16=True), ref.input_grad(x, w, (1, 1, 1), xs), "f16 dgrad " + names)
