"""No-GPU checks of the per-map loss with NSS and SIM terms, P3D_LOSS_SALIENCY: the float64 restatement in
saliency_loss_ref.py against the oracle's metrics and against central differences, its degenerate maps, its agreement with
map_loss_ref.py when the new weights are 0, and the Python front ends (fixations_to_grid, the names and weights of set_loss,
the driver's flags, the declared and bound symbols)."""
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_loss_ref as klcc          # noqa: E402
import saliency_loss_ref as ref      # noqa: E402
from oracle import metrics as oracle_metrics      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 63


def _maps(seed, maps=3, n=N):
    """s, y, f without ties: p' != q' everywhere (asserted), so that the loss is smooth at the point."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.05, 0.95, (maps, n))
    y = rng.random((maps, n))
    f = np.where(rng.random((maps, n)) < 0.15, 255, 0).astype(np.uint8)
    f[:, 5] = 200
    for m in range(maps):
        pp, qp = ref.nss_sim(s[m], y[m], f[m])["pq"]
        assert np.all(pp != qp) and np.abs(pp - qp).min() > 1e-7
    return s, y, f


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_nss_and_sim_equal_the_oracle_metrics(seed):
    s, y, f = _maps(seed, maps=4, n=7 * 9)
    for m in range(4):
        e = ref.nss_sim(s[m], y[m], f[m])
        assert abs(e["nss"] - oracle_metrics.NSS(s[m].reshape(7, 9), (f[m] >= 128).reshape(7, 9))) <= 1e-12
        assert abs(e["sim"] - oracle_metrics.SIM(s[m].reshape(7, 9), y[m].reshape(7, 9))) <= 1e-12


def test_threshold_is_128():
    s, y, f = _maps(3, maps=1)
    f127 = np.where(f[0] >= 128, 128, 127).astype(np.uint8)
    a, b = ref.nss_sim(s[0], y[0], f[0]), ref.nss_sim(s[0], y[0], f127)
    assert a["nss"] == b["nss"] and a["F"] == b["F"] == int((f[0] >= 128).sum())
    assert ref.nss_sim(s[0], y[0], np.full(N, 127, np.uint8))["F"] == 0


@pytest.mark.parametrize("weights", [(0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0), (1.0, 1.0, 1.0, 1.0), (0.7, 2.5, 0.3, 4.0)])
def test_gradient_matches_central_differences(weights):
    maps = 3
    s, y, f = _maps(int(sum(weights) * 10), maps)
    rows = [ref.one_map(s[m], y[m], f[m], *weights) for m in range(maps)]
    ranges = [r["range_s"] for r in rows]
    want = np.concatenate([r["dlds"] for r in rows])
    h = 1e-6
    got = np.empty(s.size)
    flat = s.ravel()
    for i in range(flat.size):
        up, dn = flat.copy(), flat.copy()
        up[i] += h
        dn[i] -= h
        got[i] = (ref.loss_of_s(up, y, f, maps, weights, ranges) - ref.loss_of_s(dn, y, f, maps, weights, ranges)) / (2 * h)
    assert np.abs(got - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), np.abs(got - want).max()


def test_degenerate_maps_add_zero_and_report_nan():
    s, y, f = _maps(7, maps=1)
    s, y, f = s[0], y[0], f[0]
    base = klcc.one_map(s, y, 1.0, 1.0)
    # no fixation: NSS undefined, SIM and the rest as they were
    r = ref.one_map(s, y, np.zeros(N, np.uint8), 1.0, 1.0, 1.0, 0.0)
    assert np.isnan(r["nss"]) and r["loss"] == base["loss"] and np.array_equal(r["dlds"], base["dlds"])
    r = ref.one_map(s, y, np.zeros(N, np.uint8), 1.0, 1.0, 1.0, 1.0)
    assert np.isnan(r["nss"]) and np.isfinite(r["sim"]) and r["loss"] == base["loss"] + (1.0 - r["sim"])
    # constant s: no NSS, no SIM, no CC
    const = np.full(N, 0.25)          # (exactly representable: the mean of the map is the value, A = 0)
    r = ref.one_map(const, y, f, 1.0, 1.0, 1.0, 1.0)
    k = klcc.one_map(const, y, 1.0, 1.0)
    assert np.isnan(r["nss"]) and np.isnan(r["sim"]) and np.isnan(r["cc"])
    assert r["loss"] == k["loss"] and np.array_equal(r["dlds"], k["dlds"])
    # constant y (and an all-zero one): no SIM; NSS does not read y
    for yc in (np.full(N, 0.5), np.zeros(N)):
        r = ref.one_map(s, yc, f, 1.0, 1.0, 1.0, 1.0)
        k = klcc.one_map(s, yc, 1.0, 1.0)
        assert np.isnan(r["sim"]) and np.isfinite(r["nss"])
        assert r["loss"] == k["loss"] - r["nss"] and np.array_equal(r["dlds"], k["dlds"] - r["dnss"])
        assert np.all(np.isfinite(r["dlds"]))


@pytest.mark.parametrize("a,b", [(1.0, 1.0), (0.25, 2.5), (1.0, 0.0)])
def test_without_the_new_terms_it_is_map_loss_ref(a, b):
    s, y, f = _maps(9, maps=3)
    s32 = s.astype(np.float32)
    y32 = y.astype(np.float32)
    loss, per, dl, _ = ref.saliency_loss(s32, y32, f, 3, a, b, 0.0, 0.0)
    loss0, per0, dl0, _ = klcc.map_loss(s32, y32, 3, a, b)
    assert loss == loss0 and np.array_equal(dl, dl0) and np.array_equal(per[:, :2], per0)


def test_fixations_to_grid():
    from sap3d_tensorflow_amd.dataflow import fixations_to_grid
    f = np.zeros((2, 6, 8), np.uint8)
    f[0, 0, 0] = 255          # -> cell (0, 0)
    f[0, 1, 1] = 128          # -> cell (0, 0) again
    f[0, 5, 7] = 200          # -> cell (2, 3)
    f[0, 2, 3] = 127          # below the threshold: not a fixation
    f[0, 3, 4] = 255          # -> cell (1, 2)
    f[1, 4, 2] = 129          # -> cell (2, 1)
    g = fixations_to_grid(f, 3, 4)
    want = np.zeros((2, 3, 4), np.uint8)
    want[0, 0, 0] = want[0, 2, 3] = want[0, 1, 2] = want[1, 2, 1] = 255
    assert g.dtype == np.uint8 and np.array_equal(g, want)
    assert np.array_equal(fixations_to_grid(f[0], 3, 4), want[:1])
    assert np.array_equal(fixations_to_grid(want, 3, 4), want)          # already on the grid: unchanged
    with pytest.raises(ValueError):
        fixations_to_grid(f.astype(np.float32), 3, 4)


def test_synthetic_fixations_are_deterministic_and_never_empty():
    from sap3d_tensorflow_amd import synthetic
    y = synthetic.synthetic_target(4, (2, 3, 8, 8))
    a, b = synthetic.synthetic_fixations(5, y), synthetic.synthetic_fixations(5, y)
    assert a.dtype == np.uint8 and a.shape == y.shape and np.array_equal(a, b)
    assert set(np.unique(a)) <= {0, 255} and np.all((a.reshape(6, -1) == 255).sum(axis=1) >= 1)
    assert not np.array_equal(a, synthetic.synthetic_fixations(6, y))


def test_names_and_symbols():
    from sap3d_tensorflow_amd import _lib
    assert _lib.SALIENCY_LOSSES == {"kld_cc_nss": (1, 1, 1, 0), "kld_cc_nss_sim": (1, 1, 1, 1)}
    assert _lib.P3D_LOSS_SALIENCY == 4
    hdr = open(os.path.join(ROOT, "include", "p3d_hip.h")).read()
    assert re.search(r"enum\s*\{\s*P3D_LOSS_SALIENCY\s*=\s*4\s*\}", hdr)
    lib = _lib.lib()
    for name in ("p3d_set_saliency_weights", "p3d_upload_fixations", "p3d_last_loss_terms", "p3d_debug_saliency_loss"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


class _FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name,) + tuple(args[1:]))
            return 0
        return f


def _session_with_fake_lib(monkeypatch):
    from sap3d_tensorflow_amd import session
    fake = _FakeLib()
    monkeypatch.setattr(session, "lib", lambda: fake)
    s = object.__new__(session.P3DSession)
    s._h = None
    s.y_shape = (1, 2, 3, 4)
    return s, fake


def test_set_loss_argument_validation(monkeypatch):
    s, fake = _session_with_fake_lib(monkeypatch)
    s.set_loss("kld_cc_nss")
    assert fake.calls == [("p3d_set_saliency_weights", 1.0, 1.0, 1.0, 0.0), ("p3d_set_loss", 4)]
    fake.calls.clear()
    s.set_loss("kld_cc_nss_sim", cc_weight=0.5, nss_weight=2, sim_weight=0.25)
    assert fake.calls == [("p3d_set_saliency_weights", 1.0, 0.5, 2.0, 0.25), ("p3d_set_loss", 4)]
    fake.calls.clear()
    for kw in (dict(nss_weight=-1.0), dict(sim_weight=float("nan")), dict(kld_weight=float("inf")), dict(nss_weight="x"),
               dict(kld_weight=0, cc_weight=0, nss_weight=0)):
        with pytest.raises(ValueError):
            s.set_loss("kld_cc_nss", **kw)
    with pytest.raises(ValueError):
        s.set_loss("kld_cc", nss_weight=1.0)          # the older names have no NSS / SIM weight
    with pytest.raises(ValueError):
        s.set_loss("smooth_l1", sim_weight=1.0)
    with pytest.raises(ValueError):
        s.set_loss("kld_cc_nss_cc")
    assert fake.calls == []
    s.set_loss("kld_cc", cc_weight=0.5)               # and keep working as before
    assert fake.calls == [("p3d_set_loss_weights", 1.0, 0.5), ("p3d_set_loss", 3)]


def test_upload_fixations_checks_dtype_and_shape(monkeypatch):
    s, fake = _session_with_fake_lib(monkeypatch)
    with pytest.raises(ValueError):
        s.upload_fixations(np.zeros((1, 2, 3, 4), np.float32))
    with pytest.raises(ValueError):
        s.upload_fixations(np.zeros((1, 2, 3, 5), np.uint8))
    s.upload_fixations(np.zeros((1, 2, 3, 4), np.uint8))
    assert [c[0] for c in fake.calls] == ["p3d_upload_fixations"]


def test_train_driver_flags(monkeypatch):
    spec = importlib.util.spec_from_file_location("train_driver", os.path.join(ROOT, "drivers", "train.py"))
    tr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tr)
    monkeypatch.setattr(sys, "argv", ["train.py", "--loss", "kld_cc_nss", "--batch", "1", "--videolength", "2", "--imagesize", "4", "4",
                                      "--steps", "2"])
    args = tr.get_arguments()
    assert args.nss_weight == 1.0 and args.sim_weight is None and tr.with_fixations(args)
    out = list(tr.batches(args, np.random.default_rng(0)))
    assert len(out) == 2 and all(f.dtype == np.uint8 and f.shape == y.shape for _, y, f in out)
    again = list(tr.batches(args, np.random.default_rng(1)))
    assert all(np.array_equal(a[2], b[2]) for a, b in zip(out, again))      # from the seed, not from the generator
    monkeypatch.setattr(sys, "argv", ["train.py", "--loss", "kld_cc_nss", "--nss-weight", "0", "--steps", "1", "--batch", "1",
                                      "--videolength", "2", "--imagesize", "4", "4"])
    args = tr.get_arguments()
    assert not tr.with_fixations(args) and next(tr.batches(args, np.random.default_rng(0)))[2] is None
    monkeypatch.setattr(sys, "argv", ["train.py", "--loss", "kld_cc"])
    assert not tr.with_fixations(tr.get_arguments())
    # --data: fix on the grid is taken as it is, any other resolution goes through fixations_to_grid
    full = np.zeros((3, 2, 8, 8), np.uint8)
    full[1, 0, 7, 7] = 255
    g = tr.grid_fixations(full, (3, 2, 4, 4))
    assert g.shape == (3, 2, 4, 4) and g[1, 0, 3, 3] == 255 and g.sum() == 255
    assert tr.grid_fixations(g, (3, 2, 4, 4)) is g
    with pytest.raises(SystemExit):
        tr.grid_fixations(full.astype(np.float32), (3, 2, 4, 4))
