"""Op-level parity of the kernels at the end of every train step against the float64 oracle, element by element: the output
head (head.hip, through p3d_debug_head), the Smooth-L1 loss (smooth_l1_kernel, through p3d_debug_smooth_l1) and Adam
(adam_kernel, through p3d_debug_adam, and inside the train step).  Every hook case runs twice and must be bit-equal run to run.

The head has two forward kernels (L = C/4 lanes per position when L is a power of two in [2, 64], else one thread per
position) and two filter-gradient kernels (four channels per thread whose per-block partials are folded HEAD_FOLD = 32
blocks per group and then the groups, else one channel per thread and one fold), chosen by the launchers' rule; the hook
forces each where it can run and reports the kernel and grid that ran.  The stride-1 head of the GN decoder-block network
has one kernel per pass.

Head tolerances.  A float32 sum of n terms accumulated serially is within gamma_n * sum|terms| of the exact sum, gamma_n =
n u / (1 - n u), u = eps32 / 2 (Higham, Accuracy and Stability, 3.1); every output is held to n * eps32 * sum|terms| with n
the longest serial chain that forms it and sum|terms| the same operation on |x|, |k|, |dlogits| in float64:
  - forward, lanes kernel: 8 taps x 4 channels per lane, log2(L) shuffle levels, then the bias: 32 + log2(L) + 1;
  - forward, one thread per position: the bias, then 8 taps x C channels (stride 1: 27 x C);
  - input gradient: 27 taps;
  - filter gradient: the positions one thread visits (8 terms each for dbias), then the R (or 256 / C) position rows of a
    block, then the blocks of a group (at most 32) and the groups -- or all the blocks, on the one-level fold -- then the
    add into the prefilled dk / dbias (whose magnitude joins sum|terms|).
pred = sigmoid(logits): sigmoid' <= 1/4 carries the logit bound over; expf and the division add a few ulps of pred; below
the smallest normal float32 expf(-v) overflows and pred is exactly 0 (the oracle's 3.7e-44 at v = -100).

Smooth-L1.  d = pred - target rounds once; 0.5 d^2 or |d| - 0.5 rounds at most three times more, so each float32 term is
within 2 eps32 of its value, and the double sums over at most n terms add n * eps64 of their magnitude.  The gradient d,
sign(d) or (with the sigmoid) d * p * (1 - p) is within 3 eps32 of its value.  Values whose difference is exact in float32
(|d| = 1, 1 +- 1 ulp, 0) must take the reference's branch, tf.less(|d|, 1): their gradient is compared exactly.

Adam (epsilon-hat form, m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2; p -= lr_t m / (sqrt(v) + eps)).  m is a
difference when m and g have opposite signs, so its error is bounded by the magnitudes of its two terms, not by |m|:
|dm| <= 4 eps32 (b1 |m0| + (1 - b1) |g|).  v sums non-negative terms: |dv| <= 4 eps32 v.  The step size lr_t (rounded to
float32), the division and sqrt(v) + eps add at most 6 eps32 relative, so |dp| <= lr_t / (sqrt(v) + eps) * (|dm| + 6 eps32
|m|) + eps32 |p|.  Over k steps the error of m and v compounds to k times those bounds, with the magnitude sum
b1 M + (1 - b1) |g| carried along."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import nn                                   # noqa: E402
import reg_ref                                          # noqa: E402
from sap3d_tensorflow_amd import P3dError, ops          # noqa: E402

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)
TINY32 = float(np.finfo(np.float32).tiny)
F32 = lambda v: float(np.float32(v))          # noqa: E731  hyper-parameters as the kernels hold them


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the head ----------------------------------------------------------------------------------------------------------
def head_twice(*args, **kw):
    a = ops.head(*args, **kw)
    b = ops.head(*args, **kw)
    for q in range(5):
        assert bits_equal(a[q], b[q]), "run-to-run difference in output %d" % q
    assert a[5] == b[5]
    return a


def oracle_head(x, k, bias, dl, transpose):
    """float64 (logits, dx, dk [27, C], dbias) from nn's conv ops: the head is conv3d_transpose(x, 1, 3, 2) with kernel
    [3, 3, 3, 1, C] (nn.conv3d_transpose), or conv3d(x, 1, 3, 1) with kernel [3, 3, 3, C, 1] (nn.conv3d)."""
    x = np.asarray(x, np.float64)
    N, D, H, W, C = x.shape
    dl = np.asarray(dl, np.float64)[..., None]
    if transpose:
        K = np.asarray(k, np.float64).reshape(3, 3, 3, 1, C)
        s = (2, 2, 2)
        logits = nn.conv3d_backward_input(x, K, s, (N, 2 * D, 2 * H, 2 * W, 1))[..., 0] + bias
        dx = nn.conv3d_forward(dl, K, s)
        dk = nn.conv3d_backward_filter(dl, x, K.shape, s)
    else:
        K = np.asarray(k, np.float64).reshape(3, 3, 3, C, 1)
        s = (1, 1, 1)
        logits = nn.conv3d_forward(x, K, s)[..., 0] + bias
        dx = nn.conv3d_backward_input(dl, K, s, x.shape)
        dk = nn.conv3d_backward_filter(x, dl, K.shape, s)
    return logits, dx, dk.reshape(27, C), float(dl.sum())


def filter_chain(info, shape, transpose):
    """Longest serial chain of the filter gradient (and of dbias) for the kernel and grid the hook reports."""
    N, D, H, W, C = shape
    total = N * D * H * W
    kern, blocks = info[2], info[3]
    if kern == 1:                                      # four channels per thread, R = 256 / (C / 4) rows, two-level fold
        rows = 256 // (C // 4)
        fold = min(32, blocks) + -(-blocks // 32)
    else:                                              # one channel per thread, 256 / C rows, one-level fold
        rows = 256 // C
        fold = blocks
    per_thread = -(-total // (blocks * rows))
    return per_thread + rows + fold + 1, 8 * per_thread + rows + fold + 1


def check_head(shape, transpose=True, sigmoid=True, fwd_path=0, filter_path=0, seed=0, bias=0.25, xscale=1.0, dk0=None,
               db0=None):
    rng = np.random.default_rng(seed)
    N, D, H, W, C = shape
    up = 2 if transpose else 1
    x = (xscale * rng.uniform(-1, 1, shape)).astype(np.float32)
    k = rng.uniform(-1, 1, (27, C)).astype(np.float32) / np.float32(math.sqrt(C))
    dl = rng.standard_normal((N, up * D, up * H, up * W)).astype(np.float32)
    dk0 = rng.uniform(-1, 1, (27, C)).astype(np.float32) if dk0 is None else dk0
    db0 = np.float32(0.75) if db0 is None else np.float32(db0)
    bias = np.float32(bias)
    logits, pred, dx, dk, db, info = head_twice(x, k, bias, dl, transpose=transpose, sigmoid=sigmoid, dk=dk0, dbias=db0,
                                                fwd_path=fwd_path, filter_path=filter_path)
    w_logits, w_dx, w_dk, w_db = oracle_head(x, k, float(bias), dl, transpose)
    a_logits, a_dx, a_dk, a_db = oracle_head(np.abs(x), np.abs(k), abs(float(bias)), np.abs(dl), transpose)
    # forward
    if info[0] == 1:
        n_fwd = 32 + int(math.log2(C // 4)) + 1
    else:
        n_fwd = (8 if transpose else 27) * C + 1
    tol = n_fwd * EPS32 * a_logits
    err = np.abs(logits - w_logits)
    assert np.all(err <= tol), ("logits", shape, info, float((err - tol).max()))
    w_pred = 1.0 / (1.0 + np.exp(-w_logits)) if sigmoid else w_logits
    ptol = (0.25 * tol + 4 * EPS32 * np.abs(w_pred) + TINY32) if sigmoid else tol
    assert np.all(np.abs(pred - w_pred) <= ptol), ("pred", shape, info)
    if not sigmoid:
        assert bits_equal(pred, logits)
    # input gradient
    tol = 27 * EPS32 * a_dx
    err = np.abs(dx - w_dx)
    assert np.all(err <= tol), ("dx", shape, info, float((err - tol).max()))
    # filter gradient, added to dk0 / db0
    n_k, n_b = filter_chain(info, shape, transpose)
    tol = n_k * EPS32 * (a_dk + np.abs(dk0))
    err = np.abs(dk - (dk0.astype(np.float64) + w_dk))
    assert np.all(err <= tol), ("dk", shape, info, float((err - tol).max()))
    assert abs(db - (float(db0) + w_db)) <= n_b * EPS32 * (a_db + abs(float(db0))), ("dbias", shape, info, db, float(db0) + w_db)
    return info, (logits, pred, dx, dk, db)


def lanes_ok(C):
    L = C // 4
    return C % 4 == 0 and 2 <= L <= 64 and (L & (L - 1)) == 0


WIDTHS = [4, 8, 12, 16, 24, 32, 64, 96, 128, 256]


@pytest.mark.parametrize("C", WIDTHS)
def test_head_widths_every_path(C):
    shape = (2, 3, 5, 6, C)
    info, _ = check_head(shape)                                    # the network's rule
    assert info[0] == (1 if lanes_ok(C) else 2) and info[2] == 1, info
    fwd = [1, 2] if lanes_ok(C) else [2]
    for f in fwd:
        for w in (1, 2):
            got, _ = check_head(shape, fwd_path=f, filter_path=w, seed=C + 10 * f + w)
            assert got[0] == f and got[2] == w, got


@pytest.mark.parametrize("C", WIDTHS)
def test_head_stride1_widths(C):
    # C not dividing 256 (12, 24, 96): the filter gradient leaves 256 % C threads of its blocks idle
    info, _ = check_head((2, 3, 5, 6, C), transpose=False, sigmoid=False)
    assert info[0] == 3 and info[2] == 3, info


def test_head_refusals():
    x = lambda C: np.zeros((1, 2, 2, 2, C), np.float32)          # noqa: E731
    dl = np.zeros((1, 4, 4, 4), np.float32)
    for C in (6, 260):
        with pytest.raises(P3dError):
            ops.head(x(C), np.zeros((27, C)), 0.0, dl)
        with pytest.raises(P3dError):
            ops.head(x(C), np.zeros((27, C)), 0.0, np.zeros((1, 2, 2, 2)), transpose=False)
    with pytest.raises(P3dError):
        ops.head(x(12), np.zeros((27, 12)), 0.0, dl, fwd_path=1)   # L = 3: no lanes kernel
    with pytest.raises(P3dError):
        ops.head(x(4), np.zeros((27, 4)), 0.0, dl, fwd_path=1)     # L = 1
    with pytest.raises(P3dError):
        ops.head(x(8), np.zeros((27, 8)), 0.0, dl, fwd_path=3)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 8), (3, 1, 1, 1, 32), (1, 1, 1, 7, 4), (2, 1, 9, 2, 16), (1, 3, 5, 7, 12),
                                   (3, 2, 3, 5, 64)])
@pytest.mark.parametrize("transpose", [True, False])
def test_head_extents(shape, transpose):
    # D = H = W = 1: every neighbour and every tap but the centre (stride 1) or the first parity (stride 2) is out of range
    check_head(shape, transpose=transpose)
    if transpose and lanes_ok(shape[4]):
        check_head(shape, transpose=transpose, fwd_path=2, filter_path=2, seed=3)


@pytest.mark.parametrize("shape,transpose,sigmoid", [((2, 8, 56, 56, 32), True, True),      # unet
                                                     ((2, 8, 56, 56, 128), True, False),    # concat, unet++ (no sigmoid: concat)
                                                     ((2, 8, 56, 56, 256), True, False),    # gn_p3d
                                                     ((2, 16, 112, 112, 16), False, False)])  # GN decoder block
def test_head_reference_sizes(shape, transpose, sigmoid):
    info, _ = check_head(shape, transpose=transpose, sigmoid=sigmoid)
    if transpose:
        total = int(np.prod(shape[:4]))
        want = min(1024, -(-total * shape[4] // 4096))
        assert info[:3] == (1, info[1], 1) and info[3] == want, info
        if shape[4] == 32:
            assert want % 32 != 0 and want > 32                    # 392 blocks: 12 full groups and a ragged one of 8


@pytest.mark.parametrize("dims,blocks", [((1, 4, 8, 8), 4),           # one group
                                         ((1, 3, 23, 30), 33),        # a second group of one block
                                         ((2, 5, 16, 20), 50),        # a ragged second group of 18
                                         ((1, 8, 96, 96), 1024)])     # the cap: 32 full groups
def test_head_filter_fold_shapes(dims, blocks):
    # C = 64: 16 position rows per block, ceil(positions / 64) blocks
    info, _ = check_head(dims + (64,), filter_path=1, seed=blocks)
    assert info[2] == 1 and info[3] == blocks, info
    info, _ = check_head(dims + (64,), filter_path=2, seed=blocks + 1)
    assert info[2] == 2 and info[3] == min(256, -(-int(np.prod(dims)) // 128)), info


def test_head_forward_past_grid_cap():
    # lanes kernel at C = 256 (64 lanes): 73728 positions need 18432 blocks of 4 positions, the grid stops at 16384
    info, _ = check_head((1, 8, 96, 96, 256), sigmoid=True)
    assert info[0] == 1 and info[1] == 16384 and info[3] == 1024, info
    # one thread per position at C = 4: 2.1 M positions need 8320 blocks, the grid stops at 8192
    info, _ = check_head((1, 8, 512, 520, 4), sigmoid=False)
    assert info[0] == 2 and info[1] == 8192, info


def test_head_gradients_add_to_what_they_hold():
    shape = (2, 3, 6, 5, 32)
    for w in (1, 2):
        zero = np.zeros((27, 32), np.float32)
        _, got0 = check_head(shape, filter_path=w, dk0=zero, db0=0.0, seed=5)
        dk0 = np.random.default_rng(9).uniform(-2, 2, (27, 32)).astype(np.float32)
        _, got1 = check_head(shape, filter_path=w, dk0=dk0, db0=-1.5, seed=5)
        assert bits_equal(got1[3], (dk0 + got0[3]).astype(np.float32))
        assert got1[4] == np.float32(np.float32(-1.5) + got0[4])
        for q in range(3):
            assert bits_equal(got0[q], got1[q])


@pytest.mark.parametrize("bias", [100.0, -100.0])
def test_head_sigmoid_saturates(bias):
    _, (logits, pred, _, _, _) = check_head((1, 2, 3, 4, 16), bias=bias, xscale=0.01)
    assert np.all(pred == (1.0 if bias > 0 else 0.0)), np.unique(pred)


# ---- Smooth-L1 -----------------------------------------------------------------------------------------------------------
def oracle_smooth_l1(pred, target, through_sigmoid):
    tape = nn.Tape()
    p = nn.Var(np.asarray(pred, np.float64))
    out = nn.smooth_l1_loss(tape, p, np.asarray(target, np.float64))
    tape.backward(out)
    g = p.grad
    if through_sigmoid:
        g = g * p.data * (1 - p.data)
    d = p.data - np.asarray(target, np.float64)
    terms = np.where(np.abs(d) < 1, 0.5 * d * d, np.abs(d) - 0.5)
    return float(out.data), g, float(np.abs(terms).sum())


def smooth_l1_twice(*args, **kw):
    a = ops.smooth_l1(*args, **kw)
    b = ops.smooth_l1(*args, **kw)
    assert a[0] == b[0] and bits_equal(a[1], b[1]) and a[2] == b[2]
    return a


def check_smooth_l1(pred, target, through_sigmoid, offset, loss0=0.0):
    pred, target = np.asarray(pred, np.float32), np.asarray(target, np.float32)
    n = pred.size
    loss, dl, info = smooth_l1_twice(pred, target, through_sigmoid, offset, loss0)
    assert info[0] == (1 if offset == 0 and n % 4 == 0 else 2), (n, offset, info)
    assert info[1] == min(1024, -(-n // 256)), info
    w_loss, w_g, mag = oracle_smooth_l1(pred, target, through_sigmoid)
    assert abs(loss - (loss0 + w_loss)) <= 2 * EPS32 * mag + n * EPS64 * (mag + abs(loss0)), (n, offset, loss, loss0 + w_loss)
    assert np.all(np.abs(dl - w_g) <= 3 * EPS32 * np.abs(w_g)), (n, offset)
    return loss, dl


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1021, 4096, 1024 * 256 * 4 + 12])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("through_sigmoid", [True, False])
def test_smooth_l1_lengths(n, offset, through_sigmoid):
    rng = np.random.default_rng(n + offset)
    target = rng.random(n)
    if through_sigmoid:
        pred = 1 / (1 + np.exp(-rng.normal(0, 3, n)))
    else:
        pred = target + rng.normal(0, 1.5, n)                     # both branches
    check_smooth_l1(pred, target, through_sigmoid, offset)


def test_smooth_l1_branch_edges():
    one = np.float32(1)
    up, down = np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0))
    # differences exact in float32: |d| = 1 (linear branch), 1 -+ 1 ulp, 0, and large |d|
    pred = np.array([1, -1, up, -up, down, -down, 0, 0.3, 2.25, 1.25, 1e6, -1e6, 0.5, 3.0], np.float32)
    target = np.array([0, 0, 0, 0, 0, 0, 0, 0.3, 1.25, 2.25, 0, 0, 0.5, 2.0], np.float32)
    for offset in (0, 1, 2, 3):
        loss, dl = check_smooth_l1(pred, target, False, offset)
        d = pred.astype(np.float64) - target
        want = np.where(np.abs(d) < 1, d, np.sign(d)).astype(np.float32)
        assert bits_equal(dl, want)                                # tf.less(|d|, 1): |d| = 1 is linear, d = 0 gives 0
        assert dl[0] == 1 and dl[1] == -1 and dl[4] == down and dl[6] == 0 and dl[7] == 0 and dl[8] == 1
    # with the sigmoid: pred exactly 0 or 1 gives a zero gradient whatever d is
    pred = np.array([0, 1, 0, 1, 0.5, 0.25, 1, 0], np.float32)
    target = np.array([1, 0, 0, 1, 0.5, 1.25, 0.5, 0.5], np.float32)
    _, dl = check_smooth_l1(pred, target, True, 0)
    assert np.all(dl[[0, 1, 2, 3, 4, 6, 7]] == 0) and dl[5] == np.float32(-1 * 0.25 * 0.75)


def test_smooth_l1_adds_to_the_loss():
    rng = np.random.default_rng(4)
    pred, target = rng.random(5000).astype(np.float32), rng.random(5000).astype(np.float32)
    l0, d0 = check_smooth_l1(pred, target, True, 0)
    l1, d1 = check_smooth_l1(pred, target, True, 0, loss0=123.25)
    assert l1 == 123.25 + l0 and bits_equal(d0, d1)


# ---- Adam ----------------------------------------------------------------------------------------------------------------
B1, B2, EPS = F32(0.9), F32(0.999), F32(1e-8)


def adam_bounds(m0_mag, g, m1, v1, p1, lr_t, k=1):
    """Per-element bounds on p, m, v after an update (module docstring); m0_mag = b1 * (magnitude sum of m before) + ...,
    k = the number of steps whose rounding m and v carry."""
    em = 4 * EPS32 * k * (B1 * m0_mag + (1 - B1) * np.abs(g))
    ev = 4 * EPS32 * k * v1
    den = np.sqrt(v1) + EPS
    ep = lr_t / den * (em + (6 + 2 * k) * EPS32 * np.abs(m1)) + EPS32 * np.abs(p1)
    return ep, em, ev


def adam_inputs(rng, n):
    mag = 10.0 ** rng.uniform(-12, 6, n)
    g = mag * rng.choice([-1.0, 1.0], n)
    g[rng.random(n) < 0.05] = 0.0
    p = rng.uniform(-1, 1, n)
    gp = 10.0 ** rng.uniform(-12, 6, n) * rng.choice([-1.0, 1.0], n)         # an earlier step's gradient
    m = (1 - B1) * gp
    v = (1 - B2) * gp * gp
    # cancellation in b1 m + (1 - b1) g: an earlier gradient of the opposite sign
    c = rng.random(n) < 0.1
    m[c] = -(1 - B1) / B1 * g[c] * (1 + 1e-3 * rng.standard_normal(c.sum()))
    f = lambda a: a.astype(np.float32)           # noqa: E731
    return f(p), f(g), f(m), f(v)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1021, 2 ** 20 + 3])
@pytest.mark.parametrize("t", [1, 2, 10, 1000])
@pytest.mark.parametrize("lr_on_device", [False, True])
def test_adam_elementwise(n, t, lr_on_device):
    rng = np.random.default_rng(n * 7 + t)
    p, g, m, v = adam_inputs(rng, n)
    lr = F32(1e-3)
    a = ops.adam(p, g, m, v, t, lr, B1, B2, EPS, lr_on_device=lr_on_device)
    b = ops.adam(p, g, m, v, t, lr, B1, B2, EPS, lr_on_device=lr_on_device)
    for q in range(3):
        assert bits_equal(a[q], b[q])
    p1, m1, v1, lr_t = a
    want_lr_t = lr * math.sqrt(1 - B2 ** t) / (1 - B1 ** t)
    assert abs(lr_t - want_lr_t) <= EPS32 * want_lr_t            # one float32 rounding
    wp, wm, wv = (x.astype(np.float64) for x in (p, m, v))
    nn.adam_step(wp, g.astype(np.float64), wm, wv, t, lr, B1, B2, EPS)
    ep, em, ev = adam_bounds(np.abs(m.astype(np.float64)), g.astype(np.float64), wm, wv, wp, want_lr_t)
    for name, got, want, tol in (("m", m1, wm, em), ("v", v1, wv, ev), ("p", p1, wp, ep)):
        err = np.abs(got - want)
        bad = np.flatnonzero(err > tol)
        assert bad.size == 0, (name, n, t, bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("n", [1, 3, 4, 5, 7, 1021, 2 ** 20 + 3])
@pytest.mark.parametrize("lr_on_device", [False, True])
@pytest.mark.parametrize("s", [1.0, 0.37])
def test_adam_bits_are_the_float32_replay(n, lr_on_device, s):
    """adam_kernel and adam_scaled_kernel against reg_ref.adam32, bit for bit on p, m and v: tail only, one group, group plus
    tail, and more groups than one grid pass.  Elements whose 4-group lies whole in [0, n) take the fma form, the tail the
    unfused one; the scaled kernel runs on float32(g * s), rounded once."""
    rng = np.random.default_rng(n * 11 + 5)
    p, g, m, v = adam_inputs(rng, n)
    whole = (np.arange(n) & ~3) + 3 < n
    for gscale, gs in ((None, g), (s, (g * np.float32(s)).astype(np.float32))):
        p1, m1, v1, lr_t = ops.adam(p, g, m, v, 3, F32(1e-3), B1, B2, EPS, lr_on_device=lr_on_device, gscale=gscale)
        wp, wm, wv = reg_ref.adam32(p, m, v, gs, lr_t, B1, B2, EPS, whole)
        for name, got, want in (("p", p1, wp), ("m", m1, wm), ("v", v1, wv)):
            bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (name, n, gscale, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


def test_adam_refuses_a_misaligned_base():
    p = np.zeros(8, np.float32)
    for off in (1, 2, 3):
        with pytest.raises(P3dError):
            ops.adam(p, p, p, p, 1, offset=off)
    ops.adam(p, p, p, p, 1, offset=0)


@pytest.mark.parametrize("structure,cfg,shape", [("unet", (16, (1, 1, 2)), (2, 16, 32, 32)),
                                                 ("gn_p3d", (16, (1, 2, 2)), (2, 16, 32, 32))])
def test_adam_inside_the_train_step(structure, cfg, shape):
    """p1 = adam_step(p0, g) for every trainable variable over three steps of the two-part optimiser step: the first part
    (launched beside the stem's filter gradient) and the second must cover the whole buffer with neither a gap nor an
    overlap, and the first must read final gradients only."""
    from oracle import p3d
    from sap3d_tensorflow_amd import P3DSession
    base, blocks = cfg
    s = P3DSession(structure, batch=shape[0], frames=shape[1], height=shape[2], width=shape[3], base=base, blocks=blocks, seed=1)
    try:
        lr = F32(1e-3)
        s.set_adam(lr, B1, B2, EPS)
        x, y = p3d.synthetic_clip(0, shape + (3,)), p3d.synthetic_target(3, shape)
        names = [n for n, _, tr in s.variables() if tr]
        state = {n: [np.zeros(1), np.zeros(1), np.zeros(1)] for n in names}        # m, v, magnitude sum of m (float64)
        for step in range(1, 4):
            p0 = {n: s.get_param(n).astype(np.float64) for n in names}
            if step == 1:
                s.upload(x, y)
                launches = [ln for ln in s.schedule(0.0, seed=1) if ln.startswith("L ")]
                assert sum(" adam_kernel" in ln for ln in launches) == 2, "the optimiser step is not split"
            else:
                s.train_step(x, y, dropout=0.0, seed=step)
            lr_t = lr * math.sqrt(1 - B2 ** step) / (1 - B1 ** step)
            for n in names:
                g = s.get_grad(n).astype(np.float64)
                p1 = s.get_param(n)
                m, v, mag = state[n]
                mag1 = B1 * mag + (1 - B1) * np.abs(g)
                wp, wm, wv = p0[n].copy(), m * np.ones_like(g), v * np.ones_like(g)
                nn.adam_step(wp, g, wm, wv, step, lr, B1, B2, EPS)
                ep, _, _ = adam_bounds(mag, g, wm, wv, wp, lr_t, k=step)
                err = np.abs(p1 - wp)
                bad = np.flatnonzero(err > ep)
                assert bad.size == 0, (structure, step, n, bad.size, bad[:5])
                assert np.any(p1 != p0[n]) or not np.any(g), (structure, step, n, "not updated")
                state[n] = [wm, wv, mag1]
    finally:
        s.close()
