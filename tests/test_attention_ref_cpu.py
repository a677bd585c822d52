"""No-GPU checks of tests/attention_ref.py, the float64 expected results of tests/test_gpu_attention.py: the gradients are the
gradients of the forward formulas (central differences in float64), the restatement agrees with the oracle's ops, and every
input builder lands in the score regime it is named after -- so the GPU tests' conditions hold by the reference alone."""
import numpy as np
import pytest

import attention_ref as ar
from oracle import nn

f64 = np.float64


def central(fn, x, dy, eps=1e-6):
    """d <fn(x), dy> / dx by central differences."""
    g = np.zeros_like(x)
    it = np.nditer(x, flags=["multi_index"])
    for _ in it:
        i = it.multi_index
        old = x[i]
        x[i] = old + eps
        hi = (fn(x) * dy).sum()
        x[i] = old - eps
        lo = (fn(x) * dy).sum()
        x[i] = old
        g[i] = (hi - lo) / (2 * eps)
    return g


def close(a, b, tol):
    assert np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-30), np.abs(a - b).max()


def test_softmax_gradient_is_the_gradient_of_the_forward():
    rng = np.random.default_rng(0)
    s = rng.standard_normal((3, 7))
    d = rng.standard_normal((3, 7))
    close(ar.softmax_rows_bwd(ar.softmax_rows(s), d), central(ar.softmax_rows, s.copy(), d), 1e-7)


def test_core_gradients_are_the_gradients_of_the_forward():
    rng = np.random.default_rng(1)
    g, f, h, d = (rng.standard_normal(s) for s in ((2, 5, 4), (2, 6, 4), (2, 6, 32), (2, 5, 32)))
    o, dg, df, dh = ar.core(g, f, h, d)
    assert np.array_equal(o, ar.core(g, f, h))
    close(dg, central(lambda v: ar.core(v, f, h), g.copy(), d), 1e-6)
    close(df, central(lambda v: ar.core(g, v, h), f.copy(), d), 1e-6)
    close(dh, central(lambda v: ar.core(g, f, v), h.copy(), d), 1e-6)


def test_mix_gradients_are_the_gradients_of_the_forward():
    rng = np.random.default_rng(2)
    r, x, dz, prior = (rng.standard_normal((6, 8)) for _ in range(4))
    keep = rng.random((6, 8)) >= 0.5
    for gamma in (0.0, 1.0, -0.7):
        dr, dx, dgm = ar.mix_bwd(dz, r, gamma, keep, 0.5, dx_prior=prior, dgamma_prior=0.25)
        close(dr, central(lambda v: ar.mix(v, x, gamma, keep, 0.5), r.copy(), dz), 1e-7)
        close(dx - prior, central(lambda v: ar.mix(r, v, gamma, keep, 0.5), x.copy(), dz), 1e-7)
        gm = np.array([gamma])
        close(dgm - 0.25, central(lambda v: ar.mix(r, x, v[0], keep, 0.5), gm, dz), 1e-7)
    # without dropout the mask and the scale drop out
    assert np.array_equal(ar.mix(r, x, 0.3), r * 0.3 + x)
    assert np.array_equal(ar.mix_bwd(dz, r, 0.3)[1], dz)


def test_restatement_matches_the_oracle_ops():
    """oracle/nn.py's matmul and softmax, chained as oracle/p3d.py's attention() chains them (utils/network.py:183-185)."""
    rng = np.random.default_rng(3)
    g, f, h, d = (rng.standard_normal(s) for s in ((2, 9, 4), (2, 7, 4), (2, 7, 32), (2, 9, 32)))
    t = nn.Tape()
    vg, vf, vh = nn.Var(g), nn.Var(f), nn.Var(h)
    beta = nn.softmax(t, nn.matmul(t, vg, vf, transpose_b=True))
    out = nn.matmul(t, beta, vh)
    out.grad = d
    for fn in reversed(t.ops):
        fn()
    o, dg, df, dh = ar.core(g, f, h, d)
    for a, b in ((o, out.data), (dg, vg.grad), (df, vf.grad), (dh, vh.grad)):
        close(a, b, 1e-12)


def test_float32_restatement_is_the_same_formula():
    g, f, h, d = ar.core_input("units", 2, 40, 50, 64)
    for a, b in zip(ar.core(g, f, h, d, np.float32), ar.core(g, f, h, d)):
        assert a.dtype == np.float32 and b.dtype == f64
        assert 0 < ar.rel_err(a, b) < 1e-5
    s, _ = ar.softmax_input(np.random.default_rng(4), 18, 300)
    assert ar.softmax_rows(s, np.float32).dtype == np.float32
    assert 0 < ar.rel_err(ar.softmax_rows(s, np.float32), ar.softmax_rows(s)) < 1e-5
    r = np.random.default_rng(5).standard_normal((4, 8)).astype(np.float32)
    assert ar.mix(r, r, -0.7, r > 0, 0.5, np.float32).dtype == np.float32


@pytest.mark.parametrize("B,ng,nf,ch", ar.CORE_CASES + ar.STORED_ONLY_CASES)
def test_core_builders_land_in_their_regimes(B, ng, nf, ch):
    g, f, h, d = ar.core_input("units", B, ng, nf, ch)
    if nf >= 3:                     # (one key: the map is 1 whatever the scores)
        assert 0.02 < ar.mean_peak(g, f) < 0.9
    assert 0.5 < ar.scores(g, f).std() < 5                            # scores of a few units

    g, f, h, d = ar.core_input("flat", B, ng, nf, ch)
    p = ar.softmax_rows(ar.scores(g, f))
    assert np.array_equal(p, np.full_like(p, 1.0 / nf))
    close(ar.core(g, f, h), np.broadcast_to(h.astype(f64).mean(1, keepdims=True), (B, ng, ch)), 1e-12)

    g, f, h, d = ar.core_input("rising", B, ng, nf, ch)
    s = ar.scores(g, f)
    assert ar.rises_in_every_tile(s)                                  # the running maximum rises in every 32-key tile
    if nf > ar.TILE:
        assert not ar.first_tile_holds_the_maximum(s)
        assert ar.mean_peak(g, f) > 0.2                               # steep: a handful of keys carry the map
    g2, f2, _, _ = ar.core_input("falling", B, ng, nf, ch)
    s2 = ar.scores(g2, f2)
    assert ar.first_tile_holds_the_maximum(s2)                        # the first tile holds the maximum of every row
    if nf > ar.TILE:
        assert np.all(np.diff(ar.tile_maxima(s2), axis=-1) < 0)

    g, f, h, d = ar.core_input("offset", B, ng, nf, ch)
    s = ar.scores(g, f)
    assert np.all(g[..., 0] == 10) and np.all(f[..., 0] == 10)
    assert 70 < s.min() and s.max() < 130 and abs(s.mean() - 100) < 3
    if nf >= 3:
        assert 0.02 < ar.mean_peak(g, f) < 0.9


def test_core_scales_are_the_results_magnitudes_except_on_zero_results():
    g, f, h, d = ar.core_input("units", 2, 40, 50, 64)
    assert ar.core_scales(g, f, h, d) == [np.abs(w).max() for w in ar.core(g, f, h, d)]
    g, f, h, d = ar.core_input("units", 2, 37, 1, 64)              # one key: dg = df = 0
    o, dg, df, dh = ar.core(g, f, h, d)
    assert not dg.any() and not df.any()
    sc = ar.core_scales(g, f, h, d)
    assert sc[0] == np.abs(o).max() and sc[3] == np.abs(dh).max() and sc[1] > 1 and sc[2] > 1
    g, f, h, d = ar.core_input("flat", 2, 40, 50, 64)              # g = 0: df = 0 and so is the product without the cancellation
    assert ar.core_scales(g, f, h, d)[2] == 1e-30


def test_softmax_builder_rows():
    rng = np.random.default_rng(6)
    for rotate in range(9):
        s, which = ar.softmax_input(rng, 11, 65, rotate)
        assert s.dtype == np.float32 and which[0] == rotate
        for i in range(11):
            kind, off = ar.SOFTMAX_REGIMES[which[i]]
            row = s[i].astype(f64)
            assert abs(np.median(row) - off) < 2
            p = ar.softmax_rows(row)
            if kind == "flat":
                assert np.all(row == row[0]) and np.array_equal(p, np.full(65, 1 / 65))
            elif kind == "onehot":
                assert 190 < row.max() - np.median(row) < 210 and p.max() > 1 - 1e-12
            else:
                assert 0.02 < p.max() < 0.9
            assert abs(p.sum() - 1) < 1e-12
            d = rng.standard_normal(65)
            assert abs(ar.softmax_rows_bwd(p, d).sum()) < 1e-12
