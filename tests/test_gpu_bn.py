"""Op-level parity of BatchNorm's statistics behind every producer the network uses (through p3d_debug_conv_bn_stats) against
the float64 oracle: the conv's statistics epilogue writes per-tile (sum, sum of squares) partials, bn_finalize_kernel folds
them into the batch mean / variance and updates the moving statistics (tf.layers.batch_normalization in training: eps 1e-3,
momentum 0.99, biased variance, oracle/nn.py).  The cases sit on the producers' dispatch boundaries: each forced tile of the
tiled kernel with and without K-slices, the K-sliced tail, the stem, ragged row counts, the streaming 1x1x1 kernel (including
the 16384 <= M < 27648 window where its 512 partials outgrew the reserved slot), sibling pairs, transposed convs, and the
small-tensor threshold.  Below that threshold (M <= 1024, C % 8 == 0) the network's producers write no partials; the hook
then takes its statistics from p3d_bn_stats, so those cases pin the partial count (0) only -- the small-tensor kernels'
own statistics are tested through p3d_debug_bn_pass in the second half of this file.

Tolerances.
  y: bit-equal to ops.conv3d / ops.conv3d_transpose (the epilogue must not change what the conv writes).
  mean / variance against the oracle's statistics of the float64 conv: 2e-5 of the variance's scale (the test_gpu_ops.py
    conv tolerance; the statistics average the per-element conv error, so they inherit at most that).
  normalised output z = scale * y + shift (gamma 1, beta 0) against the oracle's training-mode output: 1e-4 of its scale.
  moving statistics after one update: the oracle's float64 update, within 1e-2 of the mean's / the variance's tolerance
    (the batch statistic enters with weight 0.01) plus 4 float32 ulps of the moving values (the kernel updates in float32).
  offset inputs (per-channel mean mu = 0, 4 sigma, 16 sigma through the conv's bias): the finalize forms
    var = sum(y^2) / M - mean^2 from float32 partials of at most a few hundred rows each.  A float32 partial sum of n squares
    carries a rounding error of at most about sqrt(n) * eps32 * n * (sigma^2 + mu^2) (random-walk rounding; n - 1 in the worst
    case), and the double-precision fold over partials adds nothing comparable.  Dividing by M gives
    |d var| <~ K * eps32 * (sigma^2 + mu^2), i.e. a relative error of K * eps32 * (1 + mu^2 / sigma^2).  The assertion uses
    K = 64 (sqrt of a 4096-row partial -- larger than any producer's, so a pass is not luck) against the statistics of the
    kernel's own y in float64, which isolates the statistics from the conv's error."""
import numpy as np
import pytest

from oracle import nn

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)


def rnd(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


def ref_conv(x, w, s, transpose, bias):
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    if transpose:
        oshape = (x.shape[0], x.shape[1] * s[0], x.shape[2] * s[1], x.shape[3] * s[2], w.shape[3])
        y = nn.conv3d_backward_input(x64, w64, s, oshape)
    else:
        y = nn.conv3d_forward(x64, w64, s)
    return y + bias.astype(np.float64) if bias is not None else y


def run_hook(x, w, s, bias, transpose, w2, moving):
    from sap3d_tensorflow_amd import ops
    return ops.conv_bn_stats(x, w, s, bias=bias, transpose=transpose, filter2=w2, moving=moving)


def check_one(y_got, mean, invstd, mv_after, mv_before, y_ref, x, w, s, bias, transpose, offset):
    from sap3d_tensorflow_amd import ops
    C = y_got.shape[-1]
    # the epilogue must not change y
    y_op = ops.conv3d_transpose(x, w, s, bias=bias) if transpose else ops.conv3d(x, w, s, bias=bias)
    assert np.array_equal(y_got, y_op)

    var_got = 1.0 / invstd.astype(np.float64) ** 2 - nn.BN_EPS      # invstd = 1 / sqrt(var + eps), rounded once to float32
    # statistics of the kernel's own y: the cancellation bound of the docstring
    yf = y_got.reshape(-1, C).astype(np.float64)
    m_own = yf.mean(0)
    v_own = ((yf - m_own) ** 2).mean(0)
    sig2 = v_own.max()
    mu2 = (m_own ** 2).max()
    bound = 64 * EPS32 * (sig2 + mu2) + 4 * EPS32 * (sig2 + nn.BN_EPS)      # (+ the float32 rounding of invstd itself)
    assert np.abs(var_got - v_own).max() <= bound, (np.abs(var_got - v_own).max(), bound, offset)
    assert np.abs(mean.astype(np.float64) - m_own).max() <= 64 * EPS32 * np.sqrt(sig2 + mu2), offset

    # against the oracle on the float64 conv (tf.layers.batch_normalization in training)
    tape = nn.Tape()
    mm0, mv0 = mv_before[0].astype(np.float32).copy(), mv_before[1].astype(np.float32).copy()
    gamma, beta = nn.Var(np.ones(C)), nn.Var(np.zeros(C))
    z_ref = nn.batch_normalization(tape, nn.Var(y_ref), gamma, beta, mm0.astype(np.float64), mv0.astype(np.float64), True).data
    yr = y_ref.reshape(-1, C)
    m_ref = yr.mean(0)
    v_ref = ((yr - m_ref) ** 2).mean(0)
    tol = 2e-5 * v_ref.max() + bound
    assert np.abs(var_got - v_ref).max() <= tol
    mean_tol = 2e-5 * np.sqrt(v_ref.max()) + 64 * EPS32 * np.sqrt(sig2 + mu2)
    assert np.abs(mean.astype(np.float64) - m_ref).max() <= mean_tol
    if offset == 0:
        z_got = (y_got.astype(np.float64) - mean.astype(np.float64)) * invstd.astype(np.float64)
        assert np.abs(z_got - z_ref).max() <= 1e-4 * max(np.abs(z_ref).max(), 1.0)
    (_, mm_want), (_, mv_want) = tape.updates
    ulps = 4 * EPS32 * (np.abs(mv_want).max() + np.abs(mm_want).max())
    assert np.abs(mv_after[0].astype(np.float64) - mm_want).max() <= 1e-2 * mean_tol + ulps
    assert np.abs(mv_after[1].astype(np.float64) - mv_want).max() <= 1e-2 * tol + ulps


def conv_case(xs, k, co, s, transpose=False, sibling=False, offset=0.0, seed=0):
    """Returns (nparts, kernel) after checking every tolerance of the docstring for one producer."""
    rng = np.random.default_rng(seed + 7919 * len(xs) + xs[4] * 31 + co)
    x = rnd(rng, xs)
    cin = xs[4]
    wshape = k + ((co, cin) if transpose else (cin, co))
    fan = np.prod(k) * cin
    w = (rnd(rng, wshape) / np.sqrt(fan)).astype(np.float32)
    w2 = (rnd(rng, wshape) / np.sqrt(fan)).astype(np.float32) if sibling else None
    bias = None
    if offset or rng.random() < 0.5 and xs[4] != 3:
        bias = (offset * (1.0 + 0.1 * rng.random(co)) + 0.1 * rng.standard_normal(co)).astype(np.float32)
    pairs = 2 if sibling else 1
    moving = np.stack([np.stack([rng.standard_normal(co), rng.uniform(0.5, 2.0, co)])] * pairs)
    out1 = run_hook(x, w, s, bias, transpose, w2, moving)
    out2 = run_hook(x, w, s, bias, transpose, w2, moving)
    for a, b in zip(out1[:4], out2[:4]):                      # bit-reproducible run to run
        if isinstance(a, list):
            for p, q in zip(a, b):
                assert np.array_equal(p, q)
        else:
            assert np.array_equal(a, b)
    assert out1[4:] == out2[4:]
    ys, mean, invstd, mv, nparts, kernel = out1
    for q, wq in enumerate([w] + ([w2] if sibling else [])):
        check_one(ys[q], mean[q], invstd[q], mv[q], moving[q], ref_conv(x, wq, s, transpose, bias), x, wq, s, bias, transpose,
                  offset)
    return nparts, kernel


def expect_parts(xs, k, co, s, transpose=False):
    from sap3d_tensorflow_amd import ops
    wshape = k + ((co, xs[4]) if transpose else (xs[4], co))
    written, cap = ops.stat_parts(xs, wshape, s, transpose=transpose)
    assert written <= cap
    return written


def rows_of(xs, s):
    return xs[0] * -(-xs[1] // s[0]) * -(-xs[2] // s[1]) * -(-xs[3] // s[2])


@pytest.fixture
def forced_plan():
    from sap3d_tensorflow_amd._lib import check, lib
    yield lambda tile, splits: check(lib().p3d_debug_force_plan(tile, splits, 0, 0))
    check(lib().p3d_debug_force_plan(-1, 0, 0, 0))


@pytest.mark.parametrize("tile,bm", [(0, 64), (1, 128), (2, 128)])
@pytest.mark.parametrize("splits", [0, 2, 4])
def test_tiled_plans(forced_plan, tile, bm, splits):
    xs, k, co, s = (2, 4, 16, 17, 64), (1, 3, 3), 128, (1, 1, 1)       # M = 2176: 34 / 17 row tiles
    forced_plan(tile, splits)
    nparts, kernel = conv_case(xs, k, co, s)
    assert nparts == [-(-rows_of(xs, s) // bm)] == [expect_parts(xs, k, co, s)], kernel
    assert kernel != "pw_stream_kernel"


def test_tail_split():
    xs, k, co, s = (1, 4, 74, 128, 64), (3, 3, 3), 64, (1, 1, 1)       # 296 tiles of 128x64: 40 in the K-sliced tail class
    nparts, kernel = conv_case(xs, k, co, s)
    assert kernel == "igemm2_group_kernel(tail)"
    assert nparts == [-(-rows_of(xs, s) // 128)] == [expect_parts(xs, k, co, s)]


@pytest.mark.parametrize("xs,co", [((1, 3, 37, 41, 3), 64), ((2, 4, 32, 32, 3), 16)])
def test_stem(xs, co):
    nparts, _ = conv_case(xs, (1, 7, 7), co, (1, 2, 2))
    assert nparts == [expect_parts(xs, (1, 7, 7), co, (1, 2, 2))] and nparts[0] > 0


@pytest.mark.parametrize("xs,k,co,s", [((1, 5, 13, 17, 32), (1, 3, 3), 48, (1, 1, 1)),       # M = 1105
                                       ((1, 4, 13, 11, 64), (3, 1, 1), 12, (1, 1, 1)),       # M = 572, C % 8 != 0: tiled
                                       ((2, 8, 29, 27, 64), (1, 1, 1), 128, (1, 2, 2))])     # strided 1x1x1, M = 3360
def test_ragged_rows(xs, k, co, s):
    nparts, _ = conv_case(xs, k, co, s)
    assert nparts == [expect_parts(xs, k, co, s)] and nparts[0] > 0


@pytest.mark.parametrize("xs,co", [
    ((1, 4, 64, 64, 64), 128),      # 16384: the first row count of the overflow window
    ((1, 5, 64, 64, 64), 128),      # 20480
    ((1, 1, 863, 32, 64), 128),     # 27616: the last multiple of 32 below the window's edge
    ((1, 27, 32, 32, 64), 128),     # 27648: the edge (M / 64 + 80 = 512)
    ((1, 4, 112, 112, 64), 128),    # 50176
    ((1, 4, 112, 112, 64), 64),     # 50176 at 64 channels: 784 slabs of 64 rows
    ((1, 4, 112, 112, 64), 256),    # 50176 at 256 channels
    ((1, 4, 64, 64, 64), 256),      # 16384 at 256 channels
])
def test_streaming_kernel(xs, co):
    k, s = (1, 1, 1), (1, 1, 1)
    M = rows_of(xs, s)
    nparts, kernel = conv_case(xs, k, co, s)
    assert kernel == "pw_stream_kernel"
    assert nparts == [min(M // (32 if co >= 128 else 64), 512)] == [expect_parts(xs, k, co, s)]


@pytest.mark.parametrize("offset", [4.0, 16.0])
@pytest.mark.parametrize("xs,k,co", [((1, 4, 64, 64, 64), (1, 1, 1), 128), ((2, 4, 16, 17, 64), (1, 3, 3), 64)])
def test_offset_inputs(xs, k, co, offset):
    """Per-channel mean at 4 sigma and 16 sigma (the conv's output has unit-order sigma): the docstring's cancellation bound."""
    conv_case(xs, k, co, (1, 1, 1), offset=offset)


@pytest.mark.parametrize("xs,k,co,grouped", [((1, 4, 64, 64, 64), (1, 1, 1), 128, False),    # streaming: two launches
                                              ((2, 4, 12, 12, 64), (1, 3, 3), 64, True)])    # tiled: one grouped launch
def test_sibling_pair(xs, k, co, grouped):
    nparts, kernel = conv_case(xs, k, co, (1, 1, 1), sibling=True)
    e = expect_parts(xs, k, co, (1, 1, 1))
    assert nparts == [e, e]
    assert (kernel == "igemm2_group_kernel(siblings)") == grouped, kernel


@pytest.mark.parametrize("xs,co", [((1, 4, 8, 8, 32), 16), ((2, 4, 14, 14, 64), 64), ((1, 2, 9, 9, 128), 256)])
def test_transposed(xs, co):
    k, s = (3, 3, 3), (2, 2, 2)
    nparts, _ = conv_case(xs, k, co, s, transpose=True)
    assert nparts == [expect_parts(xs, k, co, s, transpose=True)] and nparts[0] > 0


@pytest.mark.parametrize("xs,small", [((1, 4, 16, 16, 64), True),       # M = 1024: the small-tensor BatchNorm, no partials
                                      ((1, 1, 25, 41, 64), False)])    # M = 1025
def test_small_tensor_threshold(xs, small):
    nparts, _ = conv_case(xs, (1, 3, 3), 64, (1, 1, 1))
    assert (nparts == [0]) == small
    assert nparts == [expect_parts(xs, (1, 3, 3), 64, (1, 1, 1))]


# ---- one normalise / ReLU / add pass, forward and backward (p3d_debug_bn_pass) ---------------------------------------------
#
# Inputs are built so that no ReLU argument comes near zero: each BN input is mu +- (0.5 + u) per element (u uniform in
# [0, 1), signs balanced, so the batch mean is mu), |beta| <= 0.1 and gamma in [0.5, 1.5], so |gamma * xhat + beta| >= ~0.13;
# a residual that meets a ReLU (mode 1) and the second BN input of mode 2 share the element's sign.  A ReLU decision that
# flipped between float32 and float64 would otherwise move a whole element of the gradient.
#
# Tolerances: z within 1e-4 of its scale.  The backward of a batch-statistics BN is gamma * invstd * (g - mean(g) -
# xhat * mean(g * xhat)): it cancels (as attention's softmax backward does), so float32 errors are relative to the terms, not
# to the difference, and every gradient is compared within 1e-4 of the scale of its terms -- max|dz| * max(gamma * invstd)
# for the input gradients, max|want| + sqrt(M) * max|dz| * max(1, max|xhat|) for dgamma / dbeta (sums of M terms).
# With a per-channel offset mu, the non-small paths' statistics carry the cancellation error of the docstring at the top,
# K * eps32 * (1 + mu^2 / sigma^2) relative on the variance (K = 64), which is added to every tolerance (z moves by half
# the variance's relative error times |xhat|).  The small-tensor kernels are held to the same bound.

def stats_parts(M, C):
    rpi = 256 // (C // 4)
    return min(max(-(-M // (rpi * 8)), 1), 512)


def bn_inputs(rng, M, C, mode, mu=0.0):
    s = np.where(np.arange(M) % 2 == 0, 1.0, -1.0)[:, None] * np.ones((1, C))
    s = s[rng.permutation(M)]
    y1 = mu + s * (0.5 + rng.random((M, C)))
    if mode == 1:
        y2 = s * (0.2 + rng.random((M, C)))                    # residual, same sign as bn1(y1)
    elif mode == 2:
        y2 = 2.0 * mu + s * (0.5 + rng.random((M, C)))         # second BN input, same sign
    elif mode == 3:
        t = np.where(np.arange(M) % 2 == 0, 1.0, -1.0)[rng.permutation(M)][:, None]
        y2 = -mu + t * (0.5 + rng.random((M, C)))
    elif mode == 4:
        y2 = rng.standard_normal((M, C))
    else:
        y2 = None
    return y1.astype(np.float32), (y2.astype(np.float32) if y2 is not None else None)


def bn_oracle(mode, y1, y2, params, moving, dz, batch):
    """float64 tape: tf.layers.batch_normalization + tf.nn.relu + add, then the backward from dz."""
    tape = nn.Tape()
    two = mode in (2, 3)
    mv = [(moving[q][0].astype(np.float64), moving[q][1].astype(np.float64)) for q in range(2 if two else 1)]
    v1 = nn.Var(y1.astype(np.float64))
    g = [nn.Var(params[q][0].astype(np.float64)) for q in range(len(mv))]
    b = [nn.Var(params[q][1].astype(np.float64)) for q in range(len(mv))]
    n1 = nn.batch_normalization(tape, v1, g[0], b[0], mv[0][0], mv[0][1], bool(batch[0]))
    v2 = nn.Var(y2.astype(np.float64)) if y2 is not None else None
    if mode == 0:
        out = nn.relu(tape, n1)
    elif mode == 1:
        out = nn.relu(tape, nn.add(tape, n1, v2))
    elif mode == 2:
        out = nn.relu(tape, nn.add(tape, n1, nn.batch_normalization(tape, v2, g[1], b[1], mv[1][0], mv[1][1], bool(batch[1]))))
    elif mode == 3:
        out = nn.add(tape, nn.relu(tape, n1), nn.relu(tape, nn.batch_normalization(tape, v2, g[1], b[1], mv[1][0], mv[1][1],
                                                                                       bool(batch[1]))))
    else:
        out = nn.add(tape, v2, nn.relu(tape, n1))
    out.grad = dz.astype(np.float64)
    for fn in reversed(tape.ops):
        fn()
    moving_after = [list(m) for m in mv]
    k = 0
    for q in range(len(mv)):
        if batch[q]:
            moving_after[q] = [tape.updates[k][1], tape.updates[k + 1][1]]
            k += 2
    grads = np.stack([np.stack([g[q].grad, b[q].grad]) for q in range(len(mv))])
    zero = np.zeros_like(v1.data)
    return out.data, v1.grad, (v2.grad if v2 is not None and v2.grad is not None else zero), grads, np.array(moving_after)


def bn_pass_case(mode, M, C, path, batch=(1, 1), acc2=False, mu=0.0, seed=0):
    from sap3d_tensorflow_amd import ops
    rng = np.random.default_rng(seed + 1009 * mode + 17 * M + C + 7 * path + 3 * int(acc2) + 2 * batch[0])
    y1, y2 = bn_inputs(rng, M, C, mode, mu)
    bns = 2 if mode in (2, 3) else 1
    params = np.stack([np.stack([rng.uniform(0.5, 1.5, C), rng.uniform(-0.1, 0.1, C)]) for _ in range(bns)]).astype(np.float32)
    moving = []
    for q, y in enumerate([y1, y2][:bns]):
        yd = y.astype(np.float64)
        if batch[q]:
            moving.append([rng.standard_normal(C), rng.uniform(0.5, 2.0, C)])
        else:      # inference: moving statistics equal to the data's own, so the ReLU margins above hold
            moving.append([yd.mean(0), yd.var(0)])
    moving = np.array(moving, dtype=np.float32)
    dz = rng.standard_normal((M, C)).astype(np.float32)
    pre = rng.standard_normal((M, C)).astype(np.float32) if (acc2 and mode != 0) else None
    z, dy1, dy2, grads, mv, info = ops.bn_pass(mode, y1, y2, params, moving, dz, batch=batch, acc2=pre, path=path)
    again = ops.bn_pass(mode, y1, y2, params, moving, dz, batch=batch, acc2=pre, path=path)
    for a, b in zip((z, dy1, dy2, grads, mv), again[:5]):            # bit-reproducible run to run
        assert (a is None and b is None) or np.array_equal(a, b)
    zw, g1w, g2w, gw, mvw = bn_oracle(mode, y1, y2, params, moving, dz, batch)

    sig2 = min(float(np.var(y.astype(np.float64), 0).min()) for y in [y1, y2][:bns])
    off = 64 * EPS32 * (1.0 + 4.0 * mu * mu / sig2)                  # (mode 2's second input sits at 2 mu)
    tol = 1e-4 + off
    gis = np.abs(params[:, 0]).max() / np.sqrt(sig2 + nn.BN_EPS)
    assert np.abs(z - zw).max() <= tol * max(np.abs(zw).max(), 1.0), (np.abs(z - zw).max(), info)
    gscale = np.abs(dz).max() * max(gis, 1.0)
    assert np.abs(dy1 - g1w).max() <= tol * gscale, (np.abs(dy1 - g1w).max() / gscale, info)
    if mode != 0:
        want2 = g2w + (pre.astype(np.float64) if pre is not None else 0.0)
        assert np.abs(dy2 - want2).max() <= tol * (gscale + (np.abs(pre).max() if pre is not None else 0.0)), info
    pscale = np.abs(gw).max() + np.sqrt(M) * np.abs(dz).max() * 2.0
    assert np.abs(grads - gw).max() <= tol * pscale, (np.abs(grads - gw).max() / pscale, info)
    # one momentum update: 0.01 of the batch statistics' error (the cancellation bound, absolute) + float32 rounding
    mtol = 12 * EPS32 * np.abs(mvw).max() + 1e-2 * 64 * EPS32 * (sig2 + 4 * mu * mu)
    assert np.abs(mv - mvw).max() <= mtol, (np.abs(mv - mvw).max(), mtol, info)
    for q in range(bns):
        if not batch[q]:
            assert np.array_equal(mv[q], moving[q])                  # inference: the moving statistics stay
    return info


@pytest.mark.parametrize("mode,acc2", [(0, False)] + [(m, a) for m in (1, 2, 3, 4) for a in (False, True)])
@pytest.mark.parametrize("batch", [1, 0])
@pytest.mark.parametrize("M", [1024, 1025])
def test_bn_pass_modes(mode, batch, acc2, M):
    """Every mode with batch and moving statistics, the second gradient overwritten and accumulated (acc2), on both sides of
    the small-tensor threshold (M = 1024: bn_small.hip; 1025: fold-apply and the three-launch backward)."""
    info = bn_pass_case(mode, M, 64, 0, batch=(batch, batch), acc2=acc2)
    assert info[0] == (1 if M <= 1024 else 2)


PATH_CASES = [      # (M, C, path, taken or None for "must be refused")
    (1024, 64, 1, 1), (1024, 64, 2, 2), (1024, 64, 3, 3), (1025, 64, 1, None), (1025, 64, 2, 2), (1025, 64, 3, 3),
    (1024, 8, 1, 1), (1024, 8, 2, None), (1024, 8, 3, 3), (2048, 8, 0, 3), (2048, 8, 1, None),
    (1024, 504, 1, 1), (1024, 504, 3, 3), (2048, 504, 0, 3), (2048, 504, 2, None),
    (1024, 512, 1, 1), (1024, 512, 2, 2), (1024, 512, 3, 3), (2048, 512, 0, 2), (2048, 512, 3, 3),
    (1024, 1024, 1, 1), (1024, 1024, 2, 2), (1024, 1024, 3, 3), (2048, 1024, 0, 3), (2048, 1024, 2, None),   # 128 / 256 partials
    (1024, 520, 1, 1), (1024, 520, 2, None), (1024, 520, 3, 3), (2048, 520, 0, 3),
    (16384, 64, 0, 2), (16384, 64, 3, 3),          # 128 statistics partials: fold-apply takes them
    (16512, 64, 0, 3), (16512, 64, 2, None),       # 129: it does not
    (65408, 64, 0, 3), (65536, 64, 3, 3), (98304, 64, 3, 3),     # 511, 512 and capped 512 (of 768) partials
]


@pytest.mark.parametrize("mode", [0, 2, 4])
@pytest.mark.parametrize("M,C,path,taken", PATH_CASES)
def test_bn_pass_paths(mode, M, C, path, taken):
    from sap3d_tensorflow_amd import P3dError
    if taken is None:
        with pytest.raises(P3dError, match="does not take"):
            bn_pass_case(mode, M, C, path)
        return
    info = bn_pass_case(mode, M, C, path)
    assert info[0] == taken
    if taken != 1:
        assert info[1] == stats_parts(M, C)


@pytest.mark.parametrize("mu", [0.0, 4.0, 16.0])
@pytest.mark.parametrize("M,path", [(1024, 1), (1024, 3), (65536, 3), (16384, 2)])
@pytest.mark.parametrize("mode", [0, 2])
def test_bn_pass_offset_inputs(mu, M, path, mode):
    """Per-channel means at 0, 4 sigma and 16 sigma (sigma ~ 1): within the cancellation bound above, on the small-tensor
    kernels, the finalize + apply path (bn_finalize over p3d_bn_stats partials) and fold-apply."""
    bn_pass_case(mode, M, 64, path, mu=mu)
