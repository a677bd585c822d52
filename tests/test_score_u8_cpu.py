"""What tests/score_u8_ref.py claims, without a GPU: the replay of include/p3d_hip.h's "Scoring 8-bit maps" agrees with the float64
oracle on the same bytes, the EXPECTED-ties AUC is the exhaustive mean over every order of the tied pixels, the NaN cases are the
oracle's, and the boundary (symbols, plan hook, refusals) answers without a device."""
import json
import os

import numpy as np
import pytest

import kl_ig_ref
import score_u8_ref as R
from oracle import metrics as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("p3d_video_score", "p3d_score_maps_u8", "p3d_debug_score_u8", "p3d_debug_score_plan")


def _oracle(s, d, x):
    """CC, SIM, AUC_Judd(jitter=False), KL, NSS of the bytes taken as float64."""
    s64, d64, f = s.astype(np.float64), d.astype(np.float64), R.fixated(x).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.array([om.CC(s64, d64), om.SIM(s64, d64), om.AUC_Judd(s64, f, jitter=None), kl_ig_ref.kldiv(s64, d64), om.NSS(s64, f)])


@pytest.mark.parametrize("shape", [s for s in R.SHAPES] + [(270, 240)])
def test_replay_agrees_with_the_oracle_on_bytes(shape):
    c = R.case(*shape, n=2 if shape == (270, 240) else 5)
    worst = np.zeros(5)
    for i in range(len(c["sal"])):
        want = _oracle(c["sal"][i], c["den"][i], c["fix"][i])
        t = R.tables(c["sal"][i], c["den"][i], c["fix"][i])
        for how in R.HOWS:
            got = R.score(c["sal"][i], c["den"][i], c["fix"][i], R.ALL, R.REFERENCE, how)
            worst = np.maximum(worst, [R.rel(g, w) for g, w in zip(got, want)])
        # the closed form is the stated sweep, rounded once
        assert R.rel(R.auc_reference(t), R.auc_reference_sweep(t)) <= R.AUC_GATE
    print("largest relative disagreement with the oracle, CC SIM AUC KL NSS:", worst)
    assert worst[0] <= R.ORDER_GATE and worst[1] <= R.ORDER_GATE and worst[3] <= R.ORDER_GATE and worst[4] <= R.ORDER_GATE, worst
    assert worst[2] <= R.AUC_GATE, worst


def test_reference_ties_reproduce_the_reference_inside_tied_levels():
    """Heavy ties (two grey levels, fixations on both): fp runs backwards inside a level, in the oracle and in the replay alike."""
    rng = np.random.default_rng(5)
    for _ in range(20):
        s = rng.integers(0, 3, size=(6, 7)).astype(np.uint8) * 100
        x = np.where(rng.random((6, 7)) < 0.3, 255, 0).astype(np.uint8)
        if not 0 < np.count_nonzero(x) < x.size:
            continue
        t = R.tables(s, s, x)
        want = om.AUC_Judd(s.astype(np.float64), R.fixated(x).astype(np.float64), jitter=None)
        assert R.rel(R.auc_reference(t), want) <= R.AUC_GATE
        assert R.rel(R.auc_reference_sweep(t), want) <= R.AUC_GATE


def test_expected_ties_equal_the_exhaustive_mean_over_every_order():
    maps = [
        (np.array([[3, 3, 3], [7, 7, 1], [1, 7, 3]], np.uint8), np.array([[255, 0, 0], [255, 0, 0], [128, 0, 200]], np.uint8)),      # ties on both sides
        (np.array([[5, 5, 5], [5, 5, 5]], np.uint8), np.array([[255, 0, 0], [0, 255, 0]], np.uint8)),                                  # one level
        (np.array([[0, 9, 9], [9, 0, 0], [4, 4, 4]], np.uint8)[:, :2], np.array([[0, 255, 0], [0, 0, 127], [0, 255, 0]], np.uint8)[:, :2]),      # none at the lowest level
        (np.array([[2, 2, 8], [8, 8, 2]], np.uint8), np.array([[255, 255, 0], [0, 0, 0]], np.uint8)),                                  # every fixation at the lowest level
    ]
    for s, x in maps:
        got = R.auc_expected(R.tables(s, s, x))
        want = R.auc_exhaustive(s, x)
        print(s.ravel(), got, want)
        assert abs(got - want) <= R.AUC_GATE * abs(want)


def test_both_laws_coincide_on_pairwise_distinct_bytes():
    rng = np.random.default_rng(11)
    for n in (9, 100, 256):
        s = rng.permutation(256)[:n].astype(np.uint8)
        x = np.where(rng.random(n) < 0.2, 255, 0).astype(np.uint8)
        x[0], x[1] = 255, 0
        t = R.tables(s, s, x)
        assert R.rel(R.auc_reference(t), R.auc_expected(t)) <= R.AUC_GATE
        assert R.rel(R.auc_expected(t), om.AUC_Judd(s.astype(np.float64), R.fixated(x).astype(np.float64), jitter=None)) <= R.AUC_GATE


def test_nan_cases_match_the_oracle():
    c = R.edge_case(7, 19)
    for i, name in enumerate(c["names"]):
        want = _oracle(c["sal"][i], c["den"][i], c["fix"][i])
        for ties in (R.REFERENCE, R.EXPECTED):
            got = R.score(c["sal"][i], c["den"][i], c["fix"][i], R.ALL, ties)
            for j in (0, 1, 3, 4):
                assert np.isnan(got[j]) == np.isnan(want[j]), (name, j, got, want)
                if name == "every pixel fixated" and j == 4:      # the mean of a standardised map: 0, which only the integers give
                    assert got[j] == 0.0 and abs(want[j]) < 1e-15, (got, want)
                elif not np.isnan(want[j]):
                    assert R.rel(got[j], want[j]) <= R.ORDER_GATE, (name, j, got, want)
            if name == "every pixel fixated":
                assert np.isnan(got[2])                       # the reference divides by zero there: NaN here, not pinned
            elif name == "no fixation":
                assert np.isnan(got[2]) and np.isnan(want[2])
            elif ties == R.REFERENCE:
                assert R.rel(got[2], want[2]) <= R.AUC_GATE, (name, got, want)
            else:
                assert 0.0 <= got[2] <= 1.0
    # the cases named in the header: constant map -> CC, SIM, NSS NaN; no fixation -> AUC, NSS NaN; zero maps -> KL finite
    k = {n: i for i, n in enumerate(c["names"])}
    const = R.score(c["sal"][k["constant saliency"]], c["den"][k["constant saliency"]], c["fix"][k["constant saliency"]])
    assert np.isnan(const[[0, 1, 4]]).all() and np.isfinite(const[[2, 3]]).all()
    zero = R.score(c["sal"][k["all-zero saliency"]], c["den"][k["all-zero saliency"]], c["fix"][k["all-zero saliency"]])
    assert np.isfinite(zero[3])


def test_unselected_columns_are_nan():
    c = R.case(7, 19)
    got = R.score(c["sal"][0], c["den"][0], c["fix"][0], R.MATLAB)
    assert np.isfinite(got[[0, 1, 2]]).all() and np.isnan(got[[3, 4]]).all()


def test_order_spreads_stay_under_the_gate_and_match_the_recorded_ones():
    seen = R.spreads()
    print(json.dumps(seen))
    for shape, cols in seen.items():
        for name, v in cols.items():
            assert v <= R.ORDER_GATE, (shape, name, v)
    rec = json.load(open(R.GATES))
    assert rec["order_gate"] == R.ORDER_GATE and rec["gpu_gate"] == R.GPU_GATE
    assert set(rec["spreads"]) == set(seen)


def test_symbols_are_declared_exported_and_bound():
    from test_abi_cpu import declared_symbols
    from sap3d_tensorflow_amd import _lib
    assert set(SYMBOLS) <= set(declared_symbols())
    for n in SYMBOLS:
        assert hasattr(_lib.lib(), n) and n in _lib.SIGNATURES
    assert _lib.SCORE_COLUMNS == {"cc": R.CC, "sim": R.SIM, "judd": R.JUDD, "kl": R.KL, "nss": R.NSS}
    assert _lib.SCORE_TIES == {"reference": R.REFERENCE, "expected": R.EXPECTED}
    from sap3d_tensorflow_amd import P3DSession
    assert hasattr(P3DSession, "video_score")


def test_plan_hook_needs_no_device():
    """p3d_debug_score_plan is host only.  A lane's 32-bit sum of products holds 66 051 products of 255 * 255; the plan stays far
    below for every size the entry points accept, whatever the alignment."""
    from sap3d_tensorflow_amd import P3dError, metrics
    assert (2 ** 32 - 1) // (255 * 255) == 66051
    assert metrics.score_plan(15) == (1, 16, 1)
    assert metrics.score_plan(7 * 19, n=5, offset=0)[:2] == (1, 144)
    b, c, k = metrics.score_plan(263 * 251)
    assert b >= 3 and c % 16 == 0 and b * c >= 263 * 251 > (b - 1) * c
    assert metrics.score_plan(1080 * 960)[:2] == (32, 32400)
    for n_pix, n, off in ((2 ** 23, 1, 0), (2 ** 23, 2, 7), (3840 * 2160, 3, 15), (2 ** 23 - 5, 4, 0), (133, 5, 1)):
        b, c, k = metrics.score_plan(n_pix, n, off)
        assert b <= 256 and c % 16 == 0 and 1 <= k <= 130, (n_pix, n, off, b, c, k)
    # aligned alike, whole words: 16 products a trip; aligned unalike: one a trip
    assert metrics.score_plan(8192, 1, 0)[2] == 32 and metrics.score_plan(8192, 1, 3)[2] == 32
    for bad in ((0, 1, 0), (2 ** 23 + 1, 1, 0), (100, 0, 0), (100, 1, 16)):
        with pytest.raises(P3dError):
            metrics.score_plan(*bad)


def test_python_refusals_come_before_the_library():
    from sap3d_tensorflow_amd import metrics
    z = np.zeros((4, 4), np.uint8)
    with pytest.raises(ValueError):
        metrics.score_bytes(z, z, z, flags=("cc", "auc"))
    with pytest.raises(ValueError):
        metrics.score_bytes(z, z, z, ties="random")
    with pytest.raises(ValueError):
        metrics.score_bytes(z, z.astype(np.float32), z)
    with pytest.raises(ValueError):
        metrics.score_bytes(z, np.zeros((4, 5), np.uint8), z)
    assert metrics.score_flags("matlab") == R.MATLAB and metrics.score_flags(("kl", "nss")) == R.KL | R.NSS
