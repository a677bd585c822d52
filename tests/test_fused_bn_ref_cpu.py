"""tests/fused_bn_ref.py (the laws the fused-BatchNorm kernels are held to, tests/test_gpu_fused_ops.py) against the oracle's
tape (oracle/nn.py: conv3d, batch_normalization in training mode, relu), composed the way the fused step composes them:

    fold -> RELU1 / RELU2 conv;   gate -> gradient fold -> GRAD input gradient, dyt / xt filter gradients

on  conv_a -> BatchNorm -> ReLU -> conv_b  and on the ST_B / ST_C two-source sum.  Everything is float64; the tolerance is the
1e-11 (relative to the largest expected magnitude) that tests/test_oracle_vs_torch.py holds in float64."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import fused_bn_ref as ref              # noqa: E402
from oracle import nn                   # noqa: E402

TOL = 1e-11


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
    assert err < TOL, (what, err)


def fold_of(y, gamma, beta, bounds):
    """The fold on float64 partials of an arbitrary row split (ref.partials_of rounds to float32: not here)."""
    y2 = y.reshape(-1, y.shape[-1])
    parts = np.stack([np.stack([y2[a:b].sum(0), (y2[a:b] ** 2).sum(0)], -1) for a, b in zip(bounds[:-1], bounds[1:])])
    return ref.fold(parts, y2.shape[0], gamma, beta)


def backward_through(v, y, f, gamma, bm):
    """gate -> gate partials per bm-row tile -> gradient fold -> the GRAD operand dy."""
    C = y.shape[-1]
    g = ref.gate(v, y, f["scale"], f["shift"])
    parts, _ = ref.gate_partials(g.reshape(-1, C), y.reshape(-1, C), f["mean"], f["invstd"], bm)
    gf = ref.grad_fold(parts, g.reshape(-1, C).shape[0], gamma, f["mean"], f["invstd"])
    return g, gf, ref.grad_operand(g, y, gf["k1"], gf["k2"], gf["k3"])


@pytest.mark.parametrize("ka,kb", [((1, 1, 1), (1, 3, 3)), ((1, 3, 3), (3, 1, 1)), ((3, 1, 1), (1, 1, 1))])
def test_chain_matches_the_oracle_tape(ka, kb):
    rng = np.random.default_rng(11)
    shape, Ca, Cm, Cb = (2, 4, 7, 7), 8, 12, 8
    x = rng.standard_normal(shape + (Ca,))
    wa = rng.standard_normal(ka + (Ca, Cm)) * 0.3
    wb = rng.standard_normal(kb + (Cm, Cb)) * 0.3
    gamma, beta = rng.uniform(0.5, 1.5, Cm), rng.standard_normal(Cm)
    mm0, mv0 = rng.standard_normal(Cm), rng.uniform(0.5, 2.0, Cm)
    dz = rng.standard_normal(shape + (Cb,))
    # the oracle
    t = nn.Tape()
    X, WA, WB, G, B = nn.Var(x), nn.Var(wa), nn.Var(wb), nn.Var(gamma), nn.Var(beta)
    mm, mv = mm0.copy(), mv0.copy()
    Y = nn.conv3d(t, X, WA)
    Z = nn.conv3d(t, nn.relu(t, nn.batch_normalization(t, Y, G, B, mm, mv, True)), WB)
    Z.grad = dz
    for fn in reversed(t.ops):
        fn()
    t.apply_updates()
    # the laws
    y = ref.conv(x, wa)
    close(y, Y.data, "conv_a")
    M = y.size // Cm
    f = fold_of(y, gamma, beta, [0, 5, 64, 200, 333, M])
    close(ref.conv(ref.relu_operand(y, f["scale"], f["shift"]), wb), Z.data, "output")
    close(ref.moving_update(mm0, f["mean"]), mm, "moving mean")
    close(ref.moving_update(mv0, f["var"]), mv, "moving variance")
    v = ref.conv_input_grad(dz, wb)
    _, gf, dy = backward_through(v, y, f, gamma, 64)
    close(gf["dgamma"], G.grad, "dgamma")
    close(gf["dbeta"], B.grad, "dbeta")
    close(ref.conv_input_grad(dy, wa), X.grad, "dx")
    close(ref.conv_filter_grad(x, dy, ka), WA.grad, "dW_a (dyt)")
    close(ref.conv_filter_grad(ref.relu_operand(y, f["scale"], f["shift"]), dz, kb), WB.grad, "dW_b (xt = 1)")


def test_two_source_sum_matches_the_oracle_tape():
    """ST_B / ST_C: conv_b reads relu(bn1(y1)) + relu(bn2(y2)); one input gradient feeds both gates."""
    rng = np.random.default_rng(12)
    shape, Ca, Cm, Cb = (1, 2, 5, 6), 8, 12, 16
    k1, k2, kb = (1, 3, 3), (3, 1, 1), (1, 1, 1)
    x = rng.standard_normal(shape + (Ca,))
    w1, w2 = rng.standard_normal(k1 + (Ca, Cm)) * 0.3, rng.standard_normal(k2 + (Ca, Cm)) * 0.3
    wb = rng.standard_normal(kb + (Cm, Cb)) * 0.3
    gam = [rng.uniform(0.5, 1.5, Cm) for _ in range(2)]
    bet = [rng.standard_normal(Cm) for _ in range(2)]
    dz = rng.standard_normal(shape + (Cb,))
    t = nn.Tape()
    X, W1, W2, WB = nn.Var(x), nn.Var(w1), nn.Var(w2), nn.Var(wb)
    Gs, Bs = [nn.Var(g) for g in gam], [nn.Var(b) for b in bet]
    Ys = [nn.conv3d(t, X, W1), nn.conv3d(t, X, W2)]
    acts = [nn.relu(t, nn.batch_normalization(t, Ys[q], Gs[q], Bs[q], np.zeros(Cm), np.ones(Cm), True)) for q in range(2)]
    Z = nn.conv3d(t, nn.add(t, acts[0], acts[1]), WB)
    Z.grad = dz
    for fn in reversed(t.ops):
        fn()
    ys = [ref.conv(x, w1), ref.conv(x, w2)]
    M = ys[0].size // Cm
    fs = [fold_of(ys[q], gam[q], bet[q], [0, 17, M]) for q in range(2)]
    a = ref.relu_operand(ys[0], fs[0]["scale"], fs[0]["shift"], ys[1], fs[1]["scale"], fs[1]["shift"])
    close(ref.conv(a, wb), Z.data, "output")
    close(ref.conv_filter_grad(a, dz, kb), WB.grad, "dW_b (xt = 2)")
    v = ref.conv_input_grad(dz, wb)
    dx = 0
    for q, (w, k, W) in enumerate(((w1, k1, W1), (w2, k2, W2))):
        _, gf, dy = backward_through(v, ys[q], fs[q], gam[q], 128)
        close(gf["dgamma"], Gs[q].grad, "dgamma %d" % q)
        close(gf["dbeta"], Bs[q].grad, "dbeta %d" % q)
        close(ref.conv_filter_grad(x, dy, k), W.grad, "dW %d" % q)
        dx = dx + ref.conv_input_grad(dy, w)
    close(dx, X.grad, "dx")


def test_fold_clamps_a_negative_variance_and_keeps_the_published_form():
    """A constant channel whose float32 partials give sum(x^2)/M - mean^2 < 0: the clamp, and scale = gamma / sqrt(eps)."""
    M = 392
    for c in np.linspace(1.0, 40.0, 400):
        y = np.full((M, 4), np.float32(c), np.float32)
        f = ref.fold(ref.partials_of(y, [0, 100, 250, M]), M, np.ones(4), np.zeros(4))
        if f["raw_var"].min() < 0:
            break
    else:
        pytest.fail("no constant with a negative raw variance found")
    assert (f["var"] == 0).all()
    close(f["scale"], np.full(4, 1 / np.sqrt(ref.EPS)), "scale at the clamp")
