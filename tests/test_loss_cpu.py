"""No-GPU checks of the loss option (p3d_set_loss, BASELINE.json configs[2]): the header declares it and the library exports
it, a null handle is refused without a device, drivers/train.py takes `--loss`, and the float64 sigmoid cross-entropy the GPU
tests hold the kernels to (tests/test_gpu_loss.py) is the textbook -[y log p + (1-y) log(1-p)] where that form is finite."""
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bce64(z, y):
    """Sigmoid cross-entropy on logits in float64, the stable form of tf.nn.sigmoid_cross_entropy_with_logits."""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    return np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))


def sigmoid64(z):
    z = np.asarray(z, np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1 / (1 + e), e / (1 + e))


def test_header_declares_the_loss_switch_and_the_library_exports_it():
    src = open(os.path.join(ROOT, "include", "p3d_hip.h")).read()
    assert re.search(r"P3D_LOSS_SMOOTH_L1\s*=\s*0\s*,\s*P3D_LOSS_BCE\s*=\s*1\s*,\s*P3D_LOSS_L1\s*=\s*2", src)
    assert re.search(r"int p3d_set_loss\(p3d_handle\* h, int kind\);", src)
    assert re.search(r"int p3d_debug_loss\(int device, int kind, const float\* logits, const float\* pred, const float\* target, "
                     r"int64_t n, int through_sigmoid,\s+int offset, double\* loss, float\* dlogits, int\* info\);", src)
    from sap3d_tensorflow_amd import _lib
    lib = _lib.lib()
    for n in ("p3d_set_loss", "p3d_debug_loss"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert _lib.LOSSES == {"smooth_l1": 0, "bce": 1, "l1": 2}


def test_set_loss_refuses_a_null_handle_without_a_device():
    from sap3d_tensorflow_amd import _lib
    lib = _lib.lib()
    assert lib.p3d_set_loss(None, 1) == -1
    assert b"null handle" in lib.p3d_last_error()


def test_session_set_loss_rejects_unknown_names_before_the_library():
    from sap3d_tensorflow_amd import P3DSession
    s = P3DSession.__new__(P3DSession)          # no handle, no device: the name is checked first
    for bad in ("kl", "BCE", "smooth-l1", ""):
        with pytest.raises(ValueError):
            s.set_loss(bad)


def _train_driver():
    spec = importlib.util.spec_from_file_location("train_driver", os.path.join(ROOT, "drivers", "train.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("argv,want", [([], "smooth_l1"), (["--loss", "bce"], "bce"), (["--loss", "l1"], "l1"),
                                       (["--loss", "smooth_l1"], "smooth_l1")])
def test_train_driver_loss_flag(monkeypatch, argv, want):
    monkeypatch.setattr(sys, "argv", ["train.py"] + argv)
    assert _train_driver().get_arguments().loss == want


@pytest.mark.parametrize("bad", ["kl", "BCE", "mse"])
def test_train_driver_rejects_other_losses(monkeypatch, bad):
    monkeypatch.setattr(sys, "argv", ["train.py", "--loss", bad])
    with pytest.raises(SystemExit):
        _train_driver().get_arguments()


def test_stable_bce_reference_matches_the_naive_form():
    rng = np.random.default_rng(0)
    z = np.concatenate([rng.normal(0, 3, 4000), [0.0, 1e-8, -1e-8, 15, -15, 30, -30]])
    y = np.concatenate([rng.random(4000), [0, 1, 0.5, 0.37, 1, 0, 0.5]])
    p = sigmoid64(z)
    with np.errstate(divide="ignore", invalid="ignore"):
        naive = -(y * np.log(p) + (1 - y) * np.log(1 - p))
    ok = np.isfinite(naive)
    assert ok.sum() > 4000
    stable = bce64(z, y)
    assert np.all(np.isfinite(stable))
    # the naive form loses log(1-p) to cancellation as p -> 1: relative agreement scaled by 1/(1-p)
    tol = 1e-12 * (1 + np.abs(z)) / np.minimum(p, 1 - p)[ok]
    assert np.all(np.abs(stable[ok] - naive[ok]) <= tol * np.maximum(np.abs(naive[ok]), 1)), np.abs(stable[ok] - naive[ok]).max()
    # and where the naive form is not finite, the stable one is the asymptote: |z| (1 - y) or |z| y
    assert bce64(100.0, 0.25) == pytest.approx(75.0) and bce64(-100.0, 0.25) == pytest.approx(25.0)
    # z = 0: log 2 whatever y is; the gradient sigmoid(z) - y is 0.5 - y
    assert np.allclose(bce64(np.zeros(3), [0, 0.5, 1]), np.log(2))
