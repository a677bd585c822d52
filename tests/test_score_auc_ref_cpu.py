"""tests/score_auc_ref.py, the numpy replay of include/p3d_hip.h's SPLIT SWEEP, held to oracle.metrics.AUC_Borji and
oracle.evaluation.AUC_shuffled on byte maps cast to float64 (no GPU): per split within 1e-12, the bound of np.trapz's own
summation order; the recorded worst difference; and the cases the header names."""
import json
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import score_auc_ref as A       # noqa: E402

from oracle import evaluation as oe      # noqa: E402
from oracle import metrics as om         # noqa: E402


@pytest.fixture(scope="module")
def observed():
    return A.worst_against_oracle()


def test_replay_equals_the_oracle_within_the_summation_order(observed):
    worst, cases = observed
    assert cases == len(A.SHAPES) * len(A.CONTENTS) * len(A.STEPS) * 3      # AUC_Borji; AUC_shuffled with rows below nf, and with none
    assert worst <= A.ORACLE_GATE, worst


def test_recorded_worst_difference_stays_under_the_gate(observed):
    with open(A.GATES) as f:
        rec = json.load(f)
    assert rec["oracle_gate"] == A.ORACLE_GATE and rec["cases"] == observed[1]
    assert 0.0 <= rec["worst"] <= A.ORACLE_GATE
    assert observed[0] <= A.ORACLE_GATE


@pytest.mark.parametrize("step", A.STEPS + (0.7, 1.0 / 3))
def test_the_number_of_points_is_numpy_aranges(step):
    kmax = A.kmax_of(step)
    for v in range(256):
        u = v / 255.0
        K = 0 if u == 0.0 else int(math.ceil(u / step))
        assert K == len(np.arange(0, u, step)) and K <= kmax
    t = dict(lo=0, hi=255)
    lev = A.levels(t, step)
    tk = np.arange(kmax) * step
    assert all(lev[v] == np.count_nonzero(tk <= v / 255.0) for v in range(256)) and (np.diff(lev) >= 0).all()


def test_no_fixation_and_a_flat_map_give_nan():
    sal, fix = A.case(7, 19)
    idx = np.zeros((0, 4), np.int64)
    r = A.sweep(sal, np.zeros_like(fix), idx)
    assert np.isnan(r["per_rep"]).all() and (r["top"] == -1).all() and r["nf"] == 0
    nf = int(np.count_nonzero(fix >= 128))
    r = A.sweep(np.full_like(sal, 9), fix, np.random.RandomState(0).randint(0, sal.size, [nf, 4]))
    assert np.isnan(r["per_rep"]).all() and (r["lev"] == 0).all() and (r["top"] == 9).all()
    assert om.AUC_Borji(sal.astype(np.float64), np.zeros_like(fix), idx)[1] is None          # the reference: NaN before any draw


def test_every_pixel_fixated_is_finite_and_equals_the_oracle():
    sal, _ = A.case(7, 19)
    fix = np.full_like(sal, 200)
    idx = np.random.RandomState(1).randint(0, sal.size, [sal.size, 6])
    got = A.sweep(sal, fix, idx)["per_rep"]
    assert np.isfinite(got).all()
    assert np.abs(got - om.AUC_Borji(sal.astype(np.float64), fix / 255.0, idx)[1]).max() <= A.ORACLE_GATE


def test_no_rows_closes_at_one_one():
    sal, fix = A.case(16, 16)
    got = A.sweep(sal, fix, np.zeros((0, 3), np.int64))["per_rep"]
    assert np.array_equal(got, np.ones(3))               # every point at fp = 0, the last at tp = 1, then (1, 1)
    _, want = oe.AUC_shuffled(sal.astype(np.float64), fix / 255.0, np.zeros(sal.shape, bool), 3, 0.1, other_idx=np.zeros((0, 3), np.int64))
    assert np.abs(got - want).max() <= A.ORACLE_GATE
    dark = np.where(fix >= 128, 0, sal)                  # every fixation on the lowest level: no point at all, area 1 / 2
    dark.ravel()[np.flatnonzero(fix.ravel() < 128)[0]] = 255
    assert np.array_equal(A.sweep(dark, fix, np.zeros((0, 3), np.int64))["per_rep"], np.full(3, 0.5))


def test_false_positive_rate_divides_by_nf_when_rows_are_fewer():
    sal, fix = A.case(16, 16)
    nf = int(np.count_nonzero(fix >= 128))
    idx = np.random.RandomState(2).randint(0, sal.size, [nf // 3, 4])
    other = np.zeros(sal.size, bool)
    other[idx.ravel()] = True
    _, want = oe.AUC_shuffled(sal.astype(np.float64), fix / 255.0, other.reshape(sal.shape), 4, 0.1, other_idx=idx)
    assert np.abs(A.sweep(sal, fix, idx)["per_rep"] - want).max() <= A.ORACLE_GATE


def test_steps_outside_the_law_are_refused():
    for step in (0.0, -0.1, float("nan"), 1.0 / 1025):
        with pytest.raises(ValueError):
            A.kmax_of(step)
    assert A.kmax_of(1.0 / 1024) == 1024 and A.kmax_of(1.0) == 1 and A.kmax_of(0.3) == 4
