"""CPU pins of the two oracle ops tests/test_gpu_head.py holds the loss and optimiser kernels to: nn.smooth_l1_loss
(utils/network.py:49-62 with sigma 1: the quadratic branch only where tf.less(|d|, 1)) and nn.adam_step
(tf.train.AdamOptimizer's epsilon-hat form, Appendix A.6)."""
import math

import numpy as np

from oracle import nn


def test_smooth_l1_branch_at_one_and_zero():
    d = np.array([1.0, -1.0, 1.0 - 2 ** -30, -(1.0 - 2 ** -30), 0.0, 0.5, -2.0, 1.0 + 2 ** -30])
    target = np.full(d.size, 0.25)
    tape = nn.Tape()
    pred = nn.Var(target + d)
    out = nn.smooth_l1_loss(tape, pred, target)
    tape.backward(out)
    dd = pred.data - target
    # |d| = 1 is on the linear branch (|d| - 0.5, gradient sign(d)); just below it the quadratic one (d^2 / 2, gradient d)
    want_terms = [0.5, 0.5, 0.5 * dd[2] ** 2, 0.5 * dd[3] ** 2, 0.0, 0.125, 1.5, dd[7] - 0.5]
    want_grad = [1.0, -1.0, dd[2], dd[3], 0.0, 0.5, -1.0, 1.0]
    assert math.isclose(float(out.data), sum(want_terms), rel_tol=1e-15)      # a SUM, not a mean
    assert np.array_equal(pred.grad, np.array(want_grad))
    assert pred.grad[4] == 0.0 and not np.signbit(pred.grad[4])


def test_adam_step_closed_form():
    rng = np.random.default_rng(0)
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    p = rng.standard_normal(64)
    p0 = p.copy()
    m, v = np.zeros(64), np.zeros(64)
    gs = [rng.standard_normal(64) for _ in range(3)]
    for t, g in enumerate(gs, 1):
        nn.adam_step(p, g, m, v, t, lr, b1, b2, eps)
    # m_t = (1 - b1) sum_i b1^(t - i) g_i, v_t likewise, and p moves by lr_t m_t / (sqrt(v_t) + eps) at every step
    want_p = p0.copy()
    for t in range(1, 4):
        mt = (1 - b1) * sum(b1 ** (t - i) * gs[i - 1] for i in range(1, t + 1))
        vt = (1 - b2) * sum(b2 ** (t - i) * gs[i - 1] ** 2 for i in range(1, t + 1))
        lr_t = lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
        want_p -= lr_t * mt / (np.sqrt(vt) + eps)
    assert np.allclose(m, mt, rtol=1e-14, atol=1e-16) and np.allclose(v, vt, rtol=1e-14, atol=1e-18)
    assert np.allclose(p, want_p, rtol=1e-13, atol=1e-16)
    # the first step moves every element by lr (sign of g) up to eps: m / sqrt(v) = g / |g| at t = 1
    q = p0.copy()
    nn.adam_step(q, gs[0], np.zeros(64), np.zeros(64), 1, lr, b1, b2, eps)
    assert np.allclose(p0 - q, lr * np.sign(gs[0]), rtol=1e-6)
    # epsilon outside the square root: a zero second moment gives a step of lr_t * m / eps, not lr_t * m / sqrt(eps)
    q, mm, vv = np.zeros(1), np.array([1e-12 / (1 - b1)]), np.zeros(1)
    nn.adam_step(q, np.zeros(1), mm, vv, 1, lr, b1, b2, eps)
    assert math.isclose(-q[0], lr * math.sqrt(1 - b2) / (1 - b1) * b1 * 1e-12 / (1 - b1) / eps, rel_tol=1e-12)
