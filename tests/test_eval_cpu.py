"""The evaluation pass of test.py without a GPU: the float32 resize oracle against closed forms, the oracle's AUC_shuffled
against a literal Python-2-semantics loop, the draw order of the per-clip composition, and drivers/test.py's host logic."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import dataflow as odf
from oracle import evaluation as oev
from oracle import metrics as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- resize oracle: closed forms -------------------------------------------------------------------------------------
def test_resize_oracle_keeps_a_constant_map_constant():
    for (h, w, H, W) in ((112, 112, 1080, 960), (7, 5, 3, 11), (1, 9, 1, 31)):
        m = np.full((h, w), 0.3125, np.float32)
        out = odf.resize_linear(m, H, W)           # c (1 - w) + c w: float32 roundings only
        assert out.shape == (H, W) and np.abs(out - np.float32(0.3125)).max() <= 2 * np.spacing(np.float32(0.3125))


def test_resize_oracle_reproduces_a_ramp_inside_the_borders():
    h, w, H, W = 16, 20, 64, 72
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    m = (0.25 * x + 0.5 * y).astype(np.float32)
    out = odf.resize_linear(m, H, W)
    X = (np.arange(W) + 0.5) * (w / W) - 0.5                 # source coordinates of the output pixels
    Y = (np.arange(H) + 0.5) * (h / H) - 0.5
    inner_x = (X >= 0) & (X <= w - 1)
    inner_y = (Y >= 0) & (Y <= h - 1)
    want = 0.25 * X[None, :] + 0.5 * Y[:, None]
    assert np.abs(out - want)[np.ix_(inner_y, inner_x)].max() < 1e-5


def test_resize_oracle_clamps_at_the_borders():
    m = np.arange(12, dtype=np.float32).reshape(3, 4) ** 2
    out = odf.resize_linear(m, 12, 16)                      # x 4 upscale: the outer 2 columns / rows sit past the centres
    assert np.array_equal(out[:, 0], out[:, 1]) and np.array_equal(out[:, -1], out[:, -2])
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[-1], out[-2])
    assert out[0, 0] == m[0, 0] and out[-1, -1] == m[-1, -1]


def test_resize_oracle_of_one_row_maps():
    m = np.array([[0.0, 1.0, 4.0]], np.float32)
    out = odf.resize_linear(m, 1, 6)                        # scale 0.5: centres at -0.25, 0.25, 0.75, 1.25, 1.75, 2.25
    assert np.allclose(out[0], [0.0, 0.25, 0.75, 1.75, 3.25, 4.0], atol=1e-6)
    assert np.array_equal(odf.resize_linear(m, 3, 6), np.repeat(out, 3, axis=0))        # one source row: every row the same
    col = odf.resize_linear(m.T.copy(), 6, 1)
    assert np.allclose(col[:, 0], out[0], atol=1e-6)


# ---- AUC_shuffled: oracle vs the reference's Python-2 code, spelled out ------------------------------------------------
def _py2_auc_shuffled(saliency_map, fixation_map, other_map, n_rep, step_size, random):
    """utils/metrics.py:88-154 + 157-197 as Python 2 runs it (`map` returns a list)."""
    other_map = np.array(other_map) > 0.5
    S = np.asarray(saliency_map, np.float64)
    S = ((S - S.min()) / (S.max() - S.min())).ravel()
    F = (np.asarray(fixation_map) > 0.5).ravel()
    S_fix = S[F]
    n_fix = len(S_fix)
    fixated = np.nonzero(other_map.ravel())[0]
    indexer = list(map(lambda x: random.permutation(x)[:n_fix], np.tile(range(len(fixated)), [n_rep, 1])))
    # an empty other map tiles to an empty float array, which Python-2-era numpy accepted as an index
    S_rand = S[fixated[np.transpose(indexer).astype(np.int64)]] if len(fixated) else np.zeros((0, n_rep))
    auc = np.zeros(n_rep) * np.nan
    for rep in range(n_rep):
        thresholds = np.r_[0:np.max(np.r_[S_fix, S_rand[:, rep]]):step_size][::-1]
        tp = np.zeros(len(thresholds) + 2)
        fp = np.zeros(len(thresholds) + 2)
        tp[0] = 0; tp[-1] = 1
        fp[0] = 0; fp[-1] = 1
        for k, thresh in enumerate(thresholds):
            tp[k + 1] = np.sum(S_fix >= thresh) / float(n_fix)
            fp[k + 1] = np.sum(S_rand[:, rep] >= thresh) / float(n_fix)
        auc[rep] = om._trapz(tp, fp)
    return np.mean(auc)


@pytest.mark.parametrize("n_other", [400, 40, 0])
def test_oracle_auc_shuffled_equals_the_python2_loop(n_other):
    rng = np.random.default_rng(n_other)
    s = rng.random((60, 50)).astype(np.float32)
    f = np.zeros((60, 50), np.float32)
    f.flat[rng.choice(3000, 120, replace=False)] = 1
    o = np.zeros((60, 50), np.float32)
    o.flat[rng.choice(3000, n_other, replace=False)] = 1
    want = _py2_auc_shuffled(s, f, o, 12, 0.1, np.random.RandomState(9))
    r1 = np.random.RandomState(9)
    got, per = oev.AUC_shuffled(s, f, o, 12, 0.1, rng=r1)
    assert got == want and per.shape == (12,)
    if n_other == 0:                                     # no random sample: fp stays 0 until the closing point (1, 1)
        assert got == pytest.approx(1.0) and np.array_equal(r1.get_state()[1], np.random.RandomState(9).get_state()[1])


def test_oracle_auc_shuffled_refuses_a_shape_mismatch_and_skips_draws_without_fixation():
    s = np.random.default_rng(1).random((10, 10))
    with pytest.raises(ValueError):
        oev.AUC_shuffled(s, np.ones((10, 10)), np.ones((10, 11)))
    r = np.random.RandomState(3)
    assert np.isnan(oev.AUC_shuffled(s, np.zeros((10, 10)), np.ones((10, 10)), rng=r)[0])
    assert np.array_equal(r.get_state()[1], np.random.RandomState(3).get_state()[1])


# ---- the per-clip composition of test.py: draw order ----------------------------------------------------------------
def test_composition_draws_in_the_reference_order_and_skips_empty_clips():
    H, W, n_rep = 30, 20, 7
    rng = np.random.default_rng(4)
    preds = rng.random((4, 12, 12)).astype(np.float32)
    dens = rng.integers(0, 256, (4, 9, 8), dtype=np.uint8)
    fix = np.zeros((4, H, W), np.uint8)
    fix[0].flat[[3, 50, 51, 400]] = 255
    fix[2].flat[[7, 8]] = 200
    fix[3].flat[[9]] = 127                               # 127 / 255 < 0.5: not a fixation
    np.random.seed(21)
    got = [oev.test_py_clip_metrics(preds[b], dens[b], fix[b], n_rep=n_rep) for b in range(4)]
    after = np.random.get_state()
    np.random.seed(21)
    for b, n_fix in ((0, 4), (2, 2)):                   # clips 1 and 3 have no fixation: nothing drawn for them
        np.random.rand(H, W)
        np.random.randint(0, H * W, [n_fix, n_rep])
    want = np.random.get_state()
    assert np.array_equal(after[1], want[1]) and after[2] == want[2]
    for b in (1, 3):
        assert np.isnan(got[b][2:]).all() and np.isfinite(got[b][:2]).all()
    # AUC_Borji and NSS see the jittered map, CC and SIM the clean one
    np.random.seed(21)
    p = odf.resize_linear(preds[0], H, W)
    j = (p.astype(np.float64) + np.random.rand(H, W) * 1e-7).astype(np.float32)
    r = np.random.randint(0, H * W, [4, n_rep])
    assert got[0][3] == om.AUC_Borji(j, fix[0] / 255., r)[0]
    assert got[0][4] == om.NSS(j, fix[0] / 255.)
    assert got[0][0] == om.CC(p, odf.resize_linear_u8(dens[0], H, W) / 255.)


def test_product_synthetic_test_set_matches_the_oracle_law():
    from sap3d_tensorflow_amd import synthetic
    a = synthetic.synthetic_test_set(5, 4, (50, 40), (20, 30), frames=16, crop=8)
    b = oev.synthetic_test_set(5, 4, (50, 40), (20, 30), frames=16, crop=8)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    assert not a[2][2].any() and a[2][0].any()          # every third clip has no fixation


# ---- drivers/test.py -------------------------------------------------------------------------------------------------
def _driver():
    import importlib.util
    spec = importlib.util.spec_from_file_location("test_driver", os.path.join(ROOT, "drivers", "test.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_driver_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "drivers", "test.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--sauc" in r.stdout and "--time" in r.stdout


def test_driver_host_logic():
    d = _driver()
    assert d.batches(7, 2) == [(0, 2), (2, 4), (4, 6)]          # remainder=False (test.py:89)
    assert d.batches(1, 2) == []
    cols = [[0.5, np.nan, 0.7], [1, 2, 3], [np.nan, 0.2, 0.4], [0.1, 0.1, np.nan], [2.0, np.nan, 4.0]]
    assert d.nan_dropped_means(cols) == pytest.approx([0.6, 2.0, 0.3, 0.1, 3.0])
    line = d.metric_line(d.ALL_LINE, 3, d.nan_dropped_means(cols))
    assert line == " All: 3, Metrics: CC: 0.600  SIM: 2.000   NSS: 3.000  AUC_Judd: 0.300   AUC_Borji: 0.100"
    assert d.metric_line(d.STEP_LINE, 100, [1, 2, 3, 4, 5, 0.25]).endswith("sAUC: 0.250")
    assert np.array_equal(d.last_frame(np.zeros((2, 16, 4, 5))), np.zeros((2, 4, 5)))
