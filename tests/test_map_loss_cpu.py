"""No-GPU checks of the per-map saliency loss P3D_LOSS_KLD_CC: the float64 restatement in map_loss_ref.py against finite
differences and against the reference's own constructions (utils/metrics.py CC and KLdiv, written out in float64), the C ABI
declarations and exports, and the Python and driver front ends."""
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_loss_ref as ref      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _edge_maps(n=30):
    """(name, s, y, kld_weight, cc_weight) on which the loss is smooth at the point (a constant prediction is not smooth in
    its CC term, which is undefined there: it is differentiated with the KL term alone)."""
    rng = np.random.default_rng(5)
    s = rng.uniform(0.05, 0.95, n)
    one = np.zeros(n); one[7] = 0.8
    binary = (rng.random(n) < 0.3).astype(np.float64); binary[0] = 1.0
    return [
        ("zero_target", s, np.zeros(n), 1.0, 1.0),
        ("constant_prediction", np.full(n, 0.3), rng.random(n), 1.0, 0.0),
        ("one_pixel_target", s, one, 1.0, 1.0),
        ("binary_target", s, binary, 1.0, 1.0),
    ]


def _central_difference(s, y, maps, kw, cw, h=1e-6):
    g = np.empty(s.size)
    for i in range(s.size):
        up, dn = s.copy(), s.copy()
        up[i] += h
        dn[i] -= h
        g[i] = (ref.loss_of_s(up, y, maps, kw, cw) - ref.loss_of_s(dn, y, maps, kw, cw)) / (2 * h)
    return g


@pytest.mark.parametrize("kw,cw", [(1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.7, 2.5)])
def test_gradient_matches_finite_differences_on_random_maps(kw, cw):
    rng = np.random.default_rng(int(kw * 10 + cw * 100))
    maps, n = 3, 20
    s = rng.uniform(0.05, 0.95, maps * n)
    y = rng.random(maps * n)
    rows = [ref.one_map(s[m * n:(m + 1) * n], y[m * n:(m + 1) * n], kw, cw) for m in range(maps)]
    want = np.concatenate([r["dlds"] for r in rows])
    got = _central_difference(s, y, maps, kw, cw)
    assert np.abs(got - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), np.abs(got - want).max()


@pytest.mark.parametrize("case", _edge_maps(), ids=lambda c: c[0])
def test_gradient_matches_finite_differences_on_edge_maps(case):
    _, s, y, kw, cw = case
    r = ref.one_map(s, y, kw, cw)
    got = _central_difference(s, y, 1, kw, cw)
    assert np.all(np.isfinite(r["dlds"])) and np.isfinite(r["loss"])
    assert np.abs(got - r["dlds"]).max() <= 1e-6 * max(1.0, np.abs(r["dlds"]).max())


def test_edge_map_conventions():
    rng = np.random.default_rng(2)
    s = rng.uniform(0.05, 0.95, 40)
    r = ref.one_map(s, np.zeros(40))                      # Y = 0: q = y = 0, KL 0; B = 0: no CC
    assert r["kl"] == 0 and np.isnan(r["cc"]) and r["loss"] == 0 and np.all(r["dlds"] == 0)
    r = ref.one_map(np.full(40, 0.25), rng.random(40))    # A = 0 exactly (centred sums): CC undefined, adds nothing
    assert r["A"] == 0 and np.isnan(r["cc"]) and r["loss"] == r["kl"]
    r = ref.one_map(np.zeros(40), rng.random(40))         # S = 0: p = s = 0, finite, and zero dlogits through the sigmoid
    assert np.isfinite(r["loss"]) and np.all(np.isfinite(r["dlds"]))
    _, _, dl, _ = ref.map_loss(np.zeros(40, np.float32), rng.random(40), 1)
    assert np.all(dl == 0)


def _normalize_standard(x):
    """utils/metrics.py normalize(method='standard'): zero mean, unit standard deviation."""
    return (x - x.mean()) / x.std()


def test_cc_is_the_references_construction():
    rng = np.random.default_rng(3)
    for _ in range(5):
        s = rng.random((9, 7))
        y = rng.random((9, 7)) * 0.5 + 0.3 * s
        want = np.corrcoef(_normalize_standard(s).ravel(), _normalize_standard(y).ravel())[0, 1]
        assert abs(ref.one_map(s, y)["cc"] - want) <= 1e-12


def test_kl_is_the_sum_of_the_references_score():
    rng = np.random.default_rng(4)
    for y in (rng.random((8, 8)), np.zeros((8, 8)), np.eye(8)):
        s = rng.random((8, 8))
        # KLdiv in float64, without the resize (the maps have one shape): map1 / sum if any, map2 / sum if any, the score sum
        map1 = s / s.sum() if s.any() else s
        map2 = y / y.sum() if y.any() else y
        eps = 2.2204e-16
        want = (map2 * np.log(eps + map2 / (map1 + eps))).sum()
        assert abs(ref.one_map(s, y)["kl"] - want) <= 1e-12 * max(1.0, abs(want))


def test_header_declares_the_map_loss_and_the_library_exports_it():
    src = open(os.path.join(ROOT, "include", "p3d_hip.h")).read()
    assert re.search(r"^enum \{ P3D_LOSS_KLD_CC = 3 \};$", src, re.M)
    assert re.search(r"int p3d_set_loss_weights\(p3d_handle\* h, float kld_weight, float cc_weight\);", src)
    assert re.search(r"int p3d_debug_map_loss\(int device, const float\* logits, const float\* pred, const float\* target, "
                     r"int64_t maps, int64_t map_elems,\s+int through_sigmoid, int offset, float kld_weight, float cc_weight, "
                     r"double\* loss, float\* dlogits,\s+double\* per_map, int\* info\);", src)
    from sap3d_tensorflow_amd import _lib
    lib = _lib.lib()
    for n in ("p3d_set_loss_weights", "p3d_debug_map_loss"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert _lib.MAP_LOSSES == {"kld": (1.0, 0.0), "kld_cc": (1.0, 1.0)}
    assert _lib.LOSSES == {"smooth_l1": 0, "bce": 1, "l1": 2}


def test_set_loss_weights_refuses_a_null_handle_without_a_device():
    from sap3d_tensorflow_amd import _lib
    lib = _lib.lib()
    assert lib.p3d_set_loss_weights(None, 1.0, 1.0) == -1
    assert b"null handle" in lib.p3d_last_error()
    assert lib.p3d_set_loss(None, 3) == -1


def test_session_rejects_bad_names_and_weights_before_the_library():
    from sap3d_tensorflow_amd import P3DSession
    s = P3DSession.__new__(P3DSession)          # no handle, no device: names and weights are checked first
    for bad in ("kl", "BCE", "smooth-l1", "", "KLD", "kld-cc"):
        with pytest.raises(ValueError):
            s.set_loss(bad)
    for kw, cw in ((-1.0, 1.0), (1.0, -0.5), (float("nan"), 1.0), (1.0, float("inf")), (0.0, 0.0), ("x", 1.0)):
        with pytest.raises(ValueError):
            s.set_loss("kld_cc", kld_weight=kw, cc_weight=cw)
    with pytest.raises(ValueError):
        s.set_loss("kld", cc_weight=0.0, kld_weight=0.0)
    with pytest.raises(ValueError):
        s.set_loss("bce", cc_weight=1.0)        # the element-wise losses have no weights


def _train_driver():
    spec = importlib.util.spec_from_file_location("train_driver", os.path.join(ROOT, "drivers", "train.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("argv,loss,ccw", [([], "smooth_l1", 1.0), (["--loss", "kld"], "kld", 1.0),
                                           (["--loss", "kld_cc"], "kld_cc", 1.0),
                                           (["--loss", "kld_cc", "--cc-weight", "0.5"], "kld_cc", 0.5)])
def test_train_driver_map_loss_flags(monkeypatch, argv, loss, ccw):
    monkeypatch.setattr(sys, "argv", ["train.py"] + argv)
    a = _train_driver().get_arguments()
    assert a.loss == loss and a.cc_weight == ccw


@pytest.mark.parametrize("bad", ["kl", "BCE", "mse", "cc"])
def test_train_driver_still_rejects_other_losses(monkeypatch, bad):
    monkeypatch.setattr(sys, "argv", ["train.py", "--loss", bad])
    with pytest.raises(SystemExit):
        _train_driver().get_arguments()
