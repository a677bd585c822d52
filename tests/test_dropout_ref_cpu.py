"""Pins tests/dropout_ref.py, the CPU replay of the dropout mask that the GPU tests hold the kernels to: its values against a
plain-Python big-integer evaluation of the definition (include/p3d_hip.h at p3d_forward), its range, the keep share and the
independence of seeds and of neighbouring elements."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dropout_ref as dr                   # noqa: E402

MASK = (1 << 64) - 1
SEEDS = [11, 12, 2 ** 63 + 5]


def u24_bigint(seed, e):
    """The top 24 bits of the SplitMix64 finaliser of seed + golden * (e + 1), in Python integers."""
    z = (seed + 0x9E3779B97F4A7C15 * (e + 1)) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z >> 40


def test_anchor():
    """SplitMix64's first output for state 0 is 0xE220A8397B1DCDAF; u01(0, 0) is its top 24 bits times 2^-24."""
    assert 0xE220A8397B1DCDAF >> 40 == 14819496
    assert u24_bigint(0, 0) == 14819496
    assert float(dr.u01(0, 0)) * 2 ** 24 == 14819496


@pytest.mark.parametrize("seed,e", [(0, 1), (0, 2 ** 31 + 7), (11, 2 ** 40 + 3), (2 ** 63 + 5, 0), (2 ** 63 + 5, 123456789),
                                    (2 ** 64 - 1, 2 ** 33)])
def test_against_big_integers(seed, e):
    """Further indices (past 2^31 and 2^32: nothing may be truncated) and seeds with bit 63 set, scalar and in an array."""
    want = u24_bigint(seed, e)
    assert float(dr.u01(seed, e)) * 2 ** 24 == want
    got = dr.u01(seed, np.array([e, e + 1, e + 2], dtype=np.uint64))
    assert got.dtype == np.float32
    assert [float(g) * 2 ** 24 for g in got] == [u24_bigint(seed, e + k) for k in range(3)]


def test_keep_is_the_dense_index():
    k = dr.keep(11, 0.5, 130, 72)
    assert k.shape == (130, 72) and k.dtype == np.bool_
    for row, c in [(0, 0), (1, 0), (129, 71), (64, 5)]:
        assert bool(k[row, c]) == (u24_bigint(11, row * 72 + c) * 2.0 ** -24 >= 0.5)


@pytest.mark.parametrize("seed", SEEDS)
def test_range_and_float32_compare(seed):
    u = dr.u01(seed, np.arange(1 << 16, dtype=np.uint64))
    assert u.dtype == np.float32
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0
    # rate and u01 compare as float32: 0.3 is not a float32, and u01 == float32(0.3) is kept although it is < 0.3 in double
    r32 = np.float32(0.3)
    assert float(r32) > 0.3 - 1e-7 and float(r32) != 0.3
    for rate in (0.5, 0.3, 0.999):
        assert np.array_equal(dr.keep(seed, rate, 1 << 10, 64).ravel(), u >= np.float32(rate))
    assert dr.keep(seed, 0.0, 64, 64).all()
    assert dr.scale(0.5) == np.float32(2.0) and dr.scale(0.3).dtype == np.float32


@pytest.mark.parametrize("n", [65536, 65600, 524288])
@pytest.mark.parametrize("rate", [0.5, 0.3, 0.999])
@pytest.mark.parametrize("seed", SEEDS)
def test_keep_share(seed, rate, n):
    share = dr.keep(seed, rate, n // 64, 64).mean()
    sd = (rate * (1 - rate) / n) ** 0.5
    print("seed %d rate %g n %d: %.2f sigma" % (seed, rate, n, (share - (1 - rate)) / sd))
    assert abs(share - (1 - rate)) <= 4 * sd, (share, sd)


def test_independence():
    """Over 2^20 elements at rate 0.5: the masks of seeds 11 and 12 agree on half the elements, and so do e and e + 1."""
    n = 1 << 20
    a, b = dr.keep(11, 0.5, n // 64, 64).ravel(), dr.keep(12, 0.5, n // 64, 64).ravel()
    sd = 0.5 / n ** 0.5
    print("seeds: %.2f sigma; neighbours: %.2f sigma" % (((a == b).mean() - 0.5) / sd, ((a[1:] == a[:-1]).mean() - 0.5) / sd))
    assert abs((a == b).mean() - 0.5) <= 4 * sd
    assert abs((a[1:] == a[:-1]).mean() - 0.5) <= 4 * 0.5 / (n - 1) ** 0.5
