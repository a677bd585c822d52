"""No-GPU pins of the yardsticks tests/test_gpu_gn.py measures GroupNorm and CBAM with: reduce_max's tie rule and group_norm
with groups of three channels, each against a hand computation."""
import numpy as np

from oracle import nn


def test_reduce_max_splits_the_gradient_equally_among_exact_ties():
    x = np.array([[1.0, 3.0, 3.0, 0.0],
                  [2.0, 2.0, 2.0, 2.0],
                  [5.0, 1.0, 4.0, 4.0]])
    t = nn.Tape()
    v = nn.Var(x.copy())
    m = nn.reduce_max(t, v, (1,))
    assert np.array_equal(m.data[:, 0], [3.0, 2.0, 5.0])
    m.grad = np.array([[6.0], [8.0], [1.0]])
    for fn in reversed(t.ops):
        fn()
    assert np.array_equal(v.grad, [[0.0, 3.0, 3.0, 0.0],
                                   [2.0, 2.0, 2.0, 2.0],
                                   [1.0, 0.0, 0.0, 0.0]])
    # along axis 0: whole-zero columns (post-ReLU data) tie every row
    t = nn.Tape()
    v = nn.Var(np.array([[0.0, 0.0], [0.0, 0.0], [0.0, -1.0]]))
    m = nn.reduce_max(t, v, (0,))
    m.grad = np.array([[3.0, 4.0]])
    for fn in reversed(t.ops):
        fn()
    assert np.array_equal(v.grad, [[1.0, 2.0], [1.0, 2.0], [1.0, 0.0]])       # three tied zeros; two tied zeros


def test_group_norm_with_three_channels_per_group():
    rng = np.random.default_rng(3)
    N, D, H, W, C, G = 2, 2, 3, 1, 96, 32          # C / G = 3
    x = rng.standard_normal((N, D, H, W, C)) + np.linspace(-2, 2, C)
    gamma, beta = rng.uniform(0.5, 1.5, C), rng.uniform(-0.5, 0.5, C)
    dz = rng.standard_normal(x.shape)
    t = nn.Tape()
    xv, gv, bv = nn.Var(x.copy()), nn.Var(gamma.copy()), nn.Var(beta.copy())
    out = nn.group_norm(t, xv, gv, bv, G, 1e-5)
    out.grad = dz
    for fn in reversed(t.ops):
        fn()

    # restatement: loops over (sample, group), the group's channels c = 3g, 3g + 1, 3g + 2
    want = np.empty_like(x)
    dx = np.empty_like(x)
    dgamma, dbeta = np.zeros(C), np.zeros(C)
    for n in range(N):
        for g in range(G):
            cs = slice(3 * g, 3 * g + 3)
            v = x[n, ..., cs]
            mean = v.sum() / v.size
            var = ((v - mean) ** 2).sum() / v.size
            inv = 1.0 / np.sqrt(var + 1e-5)
            xhat = (v - mean) * inv
            want[n, ..., cs] = xhat * gamma[cs] + beta[cs]
            gh = dz[n, ..., cs] * gamma[cs]
            dx[n, ..., cs] = inv * (gh - gh.mean() - xhat * (gh * xhat).mean())
            dgamma[cs] += (dz[n, ..., cs] * xhat).reshape(-1, 3).sum(0)
            dbeta[cs] += dz[n, ..., cs].reshape(-1, 3).sum(0)
    assert np.allclose(out.data, want, rtol=0, atol=1e-12)
    assert np.allclose(xv.grad, dx, rtol=0, atol=1e-12)
    assert np.allclose(gv.grad, dgamma, rtol=0, atol=1e-12)
    assert np.allclose(bv.grad, dbeta, rtol=0, atol=1e-12)
