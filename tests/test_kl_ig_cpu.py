"""No-GPU checks of KL divergence and information gain (p3d_set_eval_extra): the numpy replay of include/p3d_hip.h
(tests/kl_ig_ref.py) against the reference's KLdiv formula evaluated in float64 and the MIT benchmark's InfoGain formula, the NaN
and zero cases of the law, the byte rules, that the order of the sums cannot reach the GPU tests' gate on the shared inputs, and
that the header declares and the built library exports the new entry points."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import eval_maps_ref as R
import kl_ig_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("p3d_set_eval_extra", "p3d_get_eval_extra", "p3d_last_eval_extra", "p3d_debug_eval_maps_extra", "p3d_metric_kldiv",
               "p3d_metric_info_gain")


def kldiv_formula_f64(saliency, density):
    """utils/metrics.py:338-362 on two maps of one shape (its resize is then the identity), every step in float64."""
    m1 = np.asarray(saliency, np.float64)
    m2 = np.asarray(density, np.float64)
    if m1.any():
        m1 = m1 / m1.sum()
    if m2.any():
        m2 = m2 / m2.sum()
    eps = 2.2204e-16
    return (m2 * np.log(eps + m2 / (m1 + eps))).sum()


def info_gain_formula(saliency, fixation, baseline):
    """The MIT saliency benchmark's InfoGain(saliencyMap, fixationMap, baselineMap): both maps scaled to their range, then to sum
    1; the mean over the fixated locations of log2(eps + map) - log2(eps + baseline)."""
    eps = 2.2204e-16
    m = np.asarray(saliency, np.float64).ravel()
    b = np.asarray(baseline, np.float64).ravel()
    m = (m - m.min()) / (m.max() - m.min())
    b = (b - b.min()) / (b.max() - b.min())
    m = m / m.sum()
    b = b / b.sum()
    at = np.asarray(fixation).ravel() > 0
    return np.mean(np.log2(eps + m[at]) - np.log2(eps + b[at]))


def test_header_declares_and_library_exports_the_entry_points():
    from sap3d_tensorflow_amd import _lib
    src = open(os.path.join(ROOT, "include", "p3d_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(p3d_[a-z0-9_]+)\s*\(", code))
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"enum\s*\{\s*P3D_EVAL_KLDIV\s*=\s*1\s*,\s*P3D_EVAL_INFO_GAIN\s*=\s*2\s*\}", code)
    assert _lib.EVAL_EXTRA == {"kldiv": 1, "info_gain": 2}
    # the law is in the header: the literal eps, both names, and that parity is unpinned
    assert "2.2204e-16" in src and "KLDIV" in src and "INFO GAIN" in src and "tests/kl_ig_ref.py" in src


def test_python_surface():
    from sap3d_tensorflow_amd import P3DSession, metrics
    for name in ("KLdiv", "KLdiv_batch", "InfoGain", "InfoGain_batch"):
        assert callable(getattr(metrics, name))
    for name in ("set_eval_extra", "last_eval_extra"):
        assert callable(getattr(P3DSession, name))
    assert isinstance(P3DSession.eval_extra, property)
    assert metrics.eval_extra_flags("kldiv") == 1 and metrics.eval_extra_flags(("kldiv", "info_gain")) == 3
    with pytest.raises(ValueError):
        metrics.eval_extra_flags("emd")


def test_byte_rules():
    b = np.arange(256, dtype=np.uint8)
    q = K.density_f32(b)
    assert q.dtype == np.float32
    assert np.array_equal(K.density(q), b / 255.0)              # density() takes the float32 back to byte / 255. in double
    assert not np.array_equal(q.astype(np.float64), b / 255.0)   # ... which the float32 itself is not
    assert K.fixated_bytes(np.array([0, 1, 127, 128, 129, 255], np.uint8)).tolist() == [False, False, False, True, True, True]
    assert np.array_equal(K.fixated_bytes(b), b / 255.0 > 0.5)


@pytest.mark.parametrize("k", range(len(K.SHAPES)))
def test_replay_follows_the_two_formulas(k):
    c = K.case(k)
    for b in (K.ORDINARY, K.NO_FIX, K.CONSTANT):
        y = K.density(K.density_f32(c["dens_bytes"][b]))
        got = K.kldiv(c["full"][b], y)
        want = kldiv_formula_f64(c["full"][b], c["dens_bytes"][b] / 255.0)
        print("KL", k, b, got, want)
        assert got == pytest.approx(want, rel=1e-14)
    got = K.info_gain(c["full"][K.ORDINARY], K.fixated_bytes(c["fixation"][K.ORDINARY]), c["baseline"])
    want = info_gain_formula(c["full"][K.ORDINARY], c["fixation"][K.ORDINARY], c["baseline"])
    print("IG", k, got, want)
    # the law forms sum(u) as (S1 - n min) / (max - min), the formula adds the u_i: n roundings of 2^-53 each, far below this
    assert got == pytest.approx(want, rel=1e-12)


def test_nan_and_zero_cases_of_the_law():
    rng = np.random.default_rng(3)
    s = (0.05 + rng.random((9, 11))).astype(np.float32)
    y = rng.integers(0, 256, (9, 11)) / 255.0
    f = rng.random((9, 11)) < 0.2
    base = K.prior(9, 11)
    with np.errstate(all="ignore"):
        assert K.kldiv(s, np.zeros_like(y)) == 0.0                               # an all-zero density
        assert K.kldiv(np.zeros_like(s), np.zeros_like(y)) == 0.0
        assert np.isfinite(K.kldiv(np.zeros_like(s), y)) and K.kldiv(np.zeros_like(s), y) > 1.0      # p = s where no s is nonzero
        bad = s.copy(); bad[4, 5] = np.nan
        assert np.isnan(K.kldiv(bad, y))
        ybad = y.copy(); ybad[0, 0] = np.nan
        assert np.isnan(K.kldiv(s, ybad))
        neg = s.copy(); neg[2, 2] = -0.5                                          # p + eps < 0 there: log of a negative
        assert np.isnan(K.kldiv(neg, y)) and np.isnan(kldiv_formula_f64(neg, y))
        assert np.isfinite(K.info_gain(s, f, base))
        assert np.isnan(K.info_gain(s, np.zeros_like(f), base))                  # F = 0
        assert np.isnan(K.info_gain(np.full_like(s, 0.25), f, base))             # constant s
        assert np.isnan(K.info_gain(s, f, np.full_like(base, 0.5)))              # constant b
        assert np.isnan(K.info_gain(bad, f, base)) and np.isnan(K.info_gain(s, f, bad))
        assert K.info_gain(s, f, s) == 0.0                                       # every term is x - x
    assert np.array_equal(np.isnan(K.replay(K.case(0))), K.expected_nan())
    assert np.array_equal(np.isnan(K.replay(K.case(1))), K.expected_nan())


def test_the_shapes_reach_the_block_paths():
    """23x31: one block whose last stride is ragged; 70x67: two blocks of 2345 elements, neither a multiple of the block's 256."""
    tpb = R.kernel_constants()["TPB"]
    n0, n1 = (H * W for _, (H, W) in K.SHAPES)
    assert R.full_blocks(n0) == 1 and n0 % tpb != 0
    assert R.full_blocks(n1) == 2
    r0, r1 = R.block_range(n1, 0), R.block_range(n1, 1)
    assert r0[1] == r1[0] and r1[1] == n1 and (r0[1] - r0[0]) % tpb != 0 and r1[0] % tpb != 0


def test_the_order_of_the_sums_stays_two_decades_under_the_gpu_gate():
    """The GPU kernels add in another order than numpy.  On the very inputs the GPU tests use, three orders (np.sum, np.sum over
    the reversed array, math.fsum) agree to 1e-11 relative, so a disagreement of 1e-9 on the GPU is not one of summation order.
    The values are away from zero, where a relative gate means something."""
    seen = K.spreads()
    recorded = json.load(open(K.GATES))
    print(seen)
    assert recorded["order_gate"] == K.ORDER_GATE == 1e-11 and recorded["gpu_gate"] == K.GPU_GATE == 1e-9
    assert sorted(recorded["spreads"]) == sorted(seen)
    for name, s in seen.items():
        assert s["kl"] <= K.ORDER_GATE and s["ig"] <= K.ORDER_GATE, (name, s)
        assert recorded["spreads"][name]["kl"] <= K.ORDER_GATE and recorded["spreads"][name]["ig"] <= K.ORDER_GATE
    for k in range(len(K.SHAPES)):
        rows = K.replay(K.case(k))
        nan = K.expected_nan()
        assert (np.abs(rows[~nan]) > 0.1).all(), rows
        assert not np.array_equal(K.case(k)["baseline"], K.case(k)["full"][K.ORDINARY])


def _driver():
    spec = importlib.util.spec_from_file_location("test_driver_kl_ig", os.path.join(ROOT, "drivers", "test.py"))
    d = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(d)
    return d


def test_driver_lines_and_baseline_check(tmp_path):
    d = _driver()
    cols = [0.5, 0.25, 0.75, 0.625, 1.5]
    plain = " All: 2, Metrics: CC: 0.500  SIM: 0.250   NSS: 1.500  AUC_Judd: 0.750   AUC_Borji: 0.625"
    assert d.metric_line(d.ALL_LINE, 2, cols) == plain
    assert d.metric_line(d.ALL_LINE, 2, cols, [("KLdiv", 0.1234), ("IG", -1.0)]) == plain + "   KLdiv: 0.123   IG: -1.000"
    assert d.nan_dropped_mean([1.0, float("nan"), 3.0]) == 2.0 and np.isnan(d.nan_dropped_mean([]))
    np.save(str(tmp_path / "b.npy"), K.prior(9, 11))
    assert d.load_baseline(str(tmp_path / "b.npy"), (9, 11)).dtype == np.float32
    with pytest.raises(ValueError, match="--info-gain"):
        d.load_baseline(str(tmp_path / "b.npy"), (11, 9))
    args = d.parse_args(["--kldiv", "--info-gain", "x.npy"])
    assert args.kldiv and args.info_gain == "x.npy"
    args = d.parse_args([])
    assert not args.kldiv and args.info_gain == ""
