"""The regularisation option's reference sets and helpers, without a GPU (tests/reg_ref.py).  Scales restated from the
reference: get_conv_weight(wd=0.001) in p3d.py:10-16 for the BatchNorm nets, wd=0.0005 in gn/p3d_gn.py:54-60 for the GroupNorm
nets; l2_reg() = 0.0005 * l2_loss in gn/p3d_gn.py:11-21."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import p3d      # noqa: E402
import reg_ref              # noqa: E402

CFG = p3d.NetConfig(base=16, blocks=(1, 2, 2))


@pytest.mark.parametrize("structure", reg_ref.BN_STRUCTURES)
def test_bn_nets_decay_the_get_conv_weight_kernels(structure, monkeypatch):
    wd, l2, names = reg_ref.recorded_sets(structure, CFG, monkeypatch)
    assert l2 == []
    assert "firstconv1" in wd
    assert set(wd) <= set(names) and len(set(wd)) == len(wd)
    for n in wd:
        assert not n.endswith(("_bias", "/bias", "gamma", "beta")), n
        assert "/" not in n, n                                  # no tf.layers head, attention or BatchNorm variable
        assert n == "firstconv1" or n.startswith(("conv3_", "dw3d_")) or n.endswith(("_S", "_T")), n
    # every bottleneck kernel: conv3_<id>_1, conv3_<id>_3, the S and T kernels, and the projection of each stage's first block
    assert sum(n.startswith("conv3_") and n.endswith("_1") for n in wd) == sum(CFG.blocks)
    assert sum(n.startswith("dw3d_") for n in wd) == 3
    assert not any(n.startswith("gamma") or "attention" in n or n.endswith("_sa") for n in wd)


@pytest.mark.parametrize("structure", ["gn_p3d", "gn_p3d_concat", "gn_p3d_decoder"])
def test_gn_nets(structure, monkeypatch):
    wd, l2, names = reg_ref.recorded_sets(structure, CFG, monkeypatch)
    prefix = "P3D/" if structure == "gn_p3d_decoder" else ""
    assert prefix + "firstconv1" in wd
    assert not any("cbam" in n or n.endswith(("_bias", "/bias", "gamma", "beta")) for n in wd)
    if structure != "gn_p3d_decoder":
        assert l2 == []
        return
    assert l2 == ["P3D/%s/kernel" % n for n in ("deconv_pool2", "deconv_pool3", "deconv_pool4", "conv_concat", "decoder1_conv1",
                                                 "decoder1_deconv", "decoder1_conv2", "decoder2_conv1", "decoder2_deconv",
                                                 "decoder2_conv2", "results")]
    assert set(l2) <= set(names) and not set(l2) & set(wd)


def test_term_and_gradient_on_a_hand_sized_example():
    params = {"a": np.array([1.0, 2.0], np.float32), "b": np.array([3.0], np.float32), "c": np.array([5.0], np.float32)}
    coef = reg_ref.coefficients(["a", "b"], ["c"], ("weightdecay",), wd=0.001)
    assert set(coef) == {"a", "b"} and coef["a"] == np.float32(0.0005)
    # (1/2) * [0.001 * 0.5 * (1 + 4) + 0.001 * 0.5 * 9] = 0.0035, with the float32 coefficient
    c = float(np.float32(0.0005))
    assert reg_ref.term64(params, coef) == pytest.approx(c * 0.5 * 14, rel=1e-15)
    assert abs(reg_ref.term64(params, coef) - 0.0035) < 1e-9          # float32(0.0005) is 0.0005 to 5e-8
    g = reg_ref.grad64(params, coef)
    assert np.allclose(g["a"], [c, 2 * c]) and np.allclose(g["b"], [3 * c])
    both = reg_ref.coefficients(["a", "b"], ["c"], ("weightdecay", "l2"), wd=0.001)
    assert both["c"] == np.float32(0.0005)
    assert reg_ref.decayed_grad32([1.0], 0.5, [3.0])[0] == np.float32(2.5)


def test_fma32_is_the_correctly_rounded_fma():
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(20000).astype(np.float32) for _ in range(3))
    from fractions import Fraction
    got = reg_ref.fma32(a, b, c)
    for i in range(0, 20000, 997):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        # the nearest float32: compare against both neighbours of the result
        r = got[i]
        lo, hi = np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))
        d = abs(Fraction(float(r)) - exact)
        assert d <= abs(Fraction(float(lo)) - exact) and d <= abs(Fraction(float(hi)) - exact)
    # exact a b + c = 1 + 2^-24 + 2^-60, just above a float32 midpoint: the float64 sum alone rounds to the midpoint and a
    # second rounding would give 1
    a, b, c = np.float32(-(2.0 ** -24) * (1 + 2.0 ** -18)), np.float32(1 - 2.0 ** -18), np.float32(1 + 2.0 ** -23)
    assert np.float32(float(a) * float(b) + float(c)) == np.float32(1.0)
    assert reg_ref.fma32(a, b, c)[0] == np.float32(1 + 2.0 ** -23)


def test_adam32_matches_plain_float32_on_the_tail_form():
    f = np.float32
    p, m, v, g = f([0.5]), f([0.1]), f([0.2]), f([0.3])
    p2, m2, v2 = reg_ref.adam32(p, m, v, g, 1e-3, 0.9, 0.999, 1e-8, whole=False)
    assert m2[0] == f(0.9) * f(0.1) + (f(1) - f(0.9)) * f(0.3)
    assert v2[0] == f(0.999) * f(0.2) + ((f(1) - f(0.999)) * f(0.3)) * f(0.3)


def test_the_c_abi_declares_the_option():
    import re
    from sap3d_tensorflow_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "p3d_hip.h")).read()
    m = re.search(r"enum \{ P3D_REG_WEIGHT_DECAY = (\d+), P3D_REG_L2 = (\d+) \};", hdr)
    assert m and _lib.REGULARIZATION == {"weightdecay": int(m.group(1)), "l2": int(m.group(2))}
    for sym in ("p3d_set_regularization", "p3d_last_regularization", "p3d_param_regularization", "p3d_debug_adam_decay"):
        assert sym in _lib.SIGNATURES and re.search(r"\b%s\(" % sym, hdr), sym
