"""No-GPU checks of tests/eval_maps_ref.py: every case holds the property of the input that takes the kernels of
csrc/metrics_full.hip down the path it is named for, and the oracle's values are ones a relative tolerance can be put on."""
import numpy as np
import pytest

from oracle import metrics as om

import eval_maps_ref as R

K = R.kernel_constants()


def test_kernel_constants_are_the_ones_the_cases_were_sized_for():
    assert (K["TPB"], K["SORT_TPB"], K["LCAP"], K["BLOCK_PIX"]) == (256, 1024, 4096, 4096)


def test_batch_case_straddles_the_sort_and_lds_limits():
    c = R.case("batch")
    assert c.n_fix == (0, 1, 2, 1000, 2048, 4096, 4097, 5000) and c.jitter is None and (c.n_rep, c.step) == (5, 0.1)
    assert c.maps.shape == (8, 96, 80) and R.full_blocks(96 * 80) == 2
    assert R.next_pow2(5000) > K["SORT_TPB"] and R.next_pow2(1000) <= K["SORT_TPB"]      # strided compare-exchange, pad fill
    assert 5000 - R.next_pow2(5000) < -K["SORT_TPB"]                                       # pads beyond the first thread trip
    assert K["LCAP"] in c.n_fix and K["LCAP"] + 1 in c.n_fix                               # both sides of the LDS histogram
    assert {0, 1, 2} <= set(c.n_fix) and R.next_pow2(2048) == 2048                         # empty, no sort, one exchange, exact 2^k
    # slots of the batch: distinct offsets that depend on every map before
    offs = np.cumsum([0] + [R.next_pow2(k) for k in c.n_fix])
    assert len(set(offs.tolist())) == 9


def test_tie_cases_hold_equal_thresholds_and_pixels_on_thresholds():
    for name, step in (("ties", 0.1), ("ties_fine", 0.03), ("ties_jitter", 0.1)):
        c = R.case(name)
        assert c.n_fix == (5000, 300) and c.step == step
        assert np.array_equal(c.maps, R.case("ties").maps) and np.array_equal(c.fixation, R.case("ties").fixation)
        assert (c.jitter is not None) == (name == "ties_jitter")
        if c.jitter is not None:
            assert c.jitter.shape == c.maps.shape and c.jitter.min() >= 0 and c.jitter.max() < 1e-7
            continue
        for b in range(2):
            s = c.maps[b].ravel().astype(np.float64)
            fixed = s[c.fixation[b].ravel() >= 128]
            assert len(np.unique(s)) == 16 and len(np.unique(fixed)) < len(fixed)          # equal thresholds (AUC_Judd)
            assert np.isin(s[c.fixation[b].ravel() < 128], fixed).any()                     # other pixels equal to a threshold
            norm = om.normalize(s, method="range")
            thr = np.r_[0:norm.max():step]                                                   # AUC_Borji's thresholds, :140-146
            hit = np.isin(thr[1:], norm)
            assert hit.any(), (name, b)                                                      # S >= thr decided by equality
    assert R.next_pow2(5000) > K["SORT_TPB"] and 5000 > K["LCAP"]


def _fixations_in_block(c, block):
    i0, i1 = R.block_range(c.fixation[0].size, block)
    return int(np.count_nonzero(c.fixation.ravel()[i0:i1] >= 128))


def test_large_cases_take_a_second_trip_of_the_folds_and_of_the_slot_offsets():
    c = R.case("blocks257")
    assert c.maps.shape == (1, 1025, 1025) and c.density.shape == (1, 1025, 1025) and c.n_fix == (6000,)
    # the folds run j = tid, tid + TPB, ... < nblk: a second trip from 257 blocks on, which 1080x960 does not reach
    assert R.full_blocks(1025 * 1025) == 257 > K["TPB"] and R.full_blocks(1080 * 960) <= K["TPB"]
    assert _fixations_in_block(c, 256) > 0                            # the partial of the second trip is not zero
    # pass B's "fixations before my block" sum runs j < blockIdx.x: its second trip (j = TPB) needs a block index above TPB
    assert R.full_blocks(1025 * 1025) - 1 <= K["TPB"]                 # ... which 257 blocks do not have
    d = R.case("blocks258")
    assert d.maps.shape == (1, 1027, 1027) and d.density.shape == (1, 1027, 1027) and d.n_fix == (6000,)
    nblk = R.full_blocks(1027 * 1027)
    assert nblk == 258 and nblk - 1 > K["TPB"]
    i0, i1 = R.block_range(1027 * 1027, nblk - 1)
    assert 0 <= i0 < i1 == 1027 * 1027                                 # the last block is not empty
    assert _fixations_in_block(d, K["TPB"]) > 0                       # the j = 256 term of block 257's sum is not zero
    assert _fixations_in_block(d, nblk - 1) > 0                       # and block 257 has slots that depend on it


def test_shape_cases():
    assert R.case("odd").maps.shape == (1, 33, 47) and R.case("odd").n_fix == (2,) and (33 * 47) % 64 != 0
    assert R.case("row").maps.shape == (1, 1, 300)
    r = R.case("resize")
    assert r.maps.shape == (1, 24, 20) and r.fixation.shape == (1, 96, 80)
    w = R.case("strided")
    assert w.maps.shape == (1, 96, 80, 3) and np.isnan(w.maps[..., 1:]).all() and np.isfinite(w.maps[..., 0]).all()


def test_byte_case_and_the_byte_rules():
    c = R.case("bytes")
    assert set(np.unique(c.density).tolist()) == set(range(256))
    assert set(np.unique(c.fixation).tolist()) == {0, 1, 127, 128, 129, 254, 255}
    assert c.n_fix == (int(np.count_nonzero(c.fixation / 255. > 0.5)),) == (700,)           # dataflow.py:239-241
    assert c.density.shape == c.fixation.shape                                              # the uint8 resize is a copy
    # density(): the kernels get float32(v / 255.) and recover the byte, so that v / 255. in double is the oracle's value
    v = np.arange(256)
    q = (v / 255.).astype(np.float32)
    assert np.array_equal(np.rint(q * np.float32(255)), v)
    assert np.array_equal(np.rint(q.astype(np.float64) * 255.0), v)
    assert np.array_equal(np.rint(q.astype(np.float64) * 255.0) / 255.0, v / 255.)


def test_degenerate_case():
    c = R.case("degenerate")
    assert c.n_fix[0] == 96 * 80 > K["LCAP"] and (c.fixation[0] == 255).all()
    bad = np.isnan(c.maps[1])
    assert bad.sum() == 1 and not np.isnan(c.maps[0]).any() and c.fixation[1][bad] == 0
    rows, _ = R.oracle_rows("degenerate")
    assert np.isfinite(rows[0, [0, 1, 3]]).all() and np.isnan(rows[0, 2])                   # AUC_Judd: 0 / 0
    assert abs(rows[0, 4]) < R.NSS_ALL_FIXATED_ABS                                            # the mean of all z-scores
    assert np.isnan(rows[1]).all()


@pytest.mark.parametrize("name", list(R.BUILDERS))
def test_oracle_values_can_carry_a_relative_tolerance(name):
    c = R.case(name)
    rows, _ = R.oracle_rows(name)
    assert rows.shape == (len(c.maps), 5)
    for b, n_fix in enumerate(c.n_fix):
        if (name, b) == R.NAN_PIXEL:
            continue
        assert np.isfinite(rows[b, :2]).all() and abs(rows[b, 0]) >= 0.05 and rows[b, 1] >= 0.05, (name, b, rows[b])
        if n_fix == 0:
            assert np.isnan(rows[b, 2:]).all()
        elif n_fix == c.fixation[b].size:
            assert np.isnan(rows[b, 2]) and np.isfinite(rows[b, 3])
        else:
            assert np.isfinite(rows[b, 2:]).all() and abs(rows[b, 4]) >= 0.05, (name, b, rows[b])
            assert 0.0 <= rows[b, 2] <= 1.0 and 0.0 <= rows[b, 3] <= 1.0
    again, _ = R.oracle_rows.__wrapped__(name)
    assert np.array_equal(rows, again, equal_nan=True)                                       # seeded and deterministic


def test_oracle_auc_judd_equals_the_reference_loop_on_the_tie_case():
    """oracle.metrics.AUC_Judd counts with a sort and searchsorted; on 5000 thresholds from 16 levels it must still equal
    np.sum(S >= thresh) per threshold."""
    c = R.case("ties")
    f = c.fixation[0] / 255.
    assert om.AUC_Judd(c.maps[0], f) == pytest.approx(R.reference_auc_judd_loop(c.maps[0], f), abs=1e-14)
