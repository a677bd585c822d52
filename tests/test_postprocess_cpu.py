"""No-GPU checks of the smoothing / normalisation stage (P3DSession.set_postprocess): the library's host-only taps
(p3d_blur_taps) against the contract of include/p3d_hip.h, the properties of the numpy replay the kernels are held to
(tests/postprocess_ref.py) with those taps, and the launcher's host-side strip table."""
import numpy as np
import pytest

import postprocess_ref as ref


def lib_taps(sigma, radius=0):
    from sap3d_tensorflow_amd import dataflow
    return dataflow.blur_taps(sigma, radius)


def test_radius_rule():
    for sigma, r in ((0.3, 1), (0.5, 2), (1.0, 4), (2.5, 10), (32.0, 128)):
        assert len(lib_taps(sigma)) == 2 * r + 1, sigma
        assert ref.radius(sigma) == r
    assert len(lib_taps(2.5, 3)) == 7                  # an explicit radius wins
    assert len(lib_taps(32.0, 255)) == 511
    assert len(lib_taps(0.0)) == 0                      # sigma == 0: no blur


@pytest.mark.parametrize("sigma,radius", [(0.3, 0), (1.0, 0), (2.5, 0), (2.5, 3), (8.0, 0), (32.0, 0), (40.0, 255), (3.0, 36)])
def test_taps_match_numpy_within_one_ulp(sigma, radius):
    w = lib_taps(sigma, radius)
    r = ref.radius(sigma, radius)
    want = ref.taps(sigma, r)
    assert w.dtype == np.float32 and w.shape == want.shape
    assert np.all(np.abs(w.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want).astype(np.float64))
    assert np.array_equal(w, w[::-1])                   # exactly symmetric
    assert abs(float(np.sum(w.astype(np.float64))) - 1.0) <= (2 * r + 1) * 2.0 ** -24
    assert np.all(w >= 0) and w[r] == w.max()


def test_refusals():
    from sap3d_tensorflow_amd import P3dError
    for sigma, radius in ((-1.0, 0), (float("nan"), 0), (float("inf"), 0), (1.0, -1), (1.0, 256), (0.0, 3), (64.0, 0)):
        with pytest.raises(P3dError):
            lib_taps(sigma, radius)


def test_impulse_gives_the_outer_product_of_the_taps():
    w = lib_taps(1.0)                                   # r = 4
    r = 4
    m = np.zeros((1, 15, 17), np.float32)
    m[0, 7, 8] = 1.0                                    # farther than r from every border
    out = ref.blur(m, w)
    want = np.zeros_like(m)
    want[0, 7 - r:7 + r + 1, 8 - r:8 + r + 1] = w[:, None] * w[None, :]
    assert want.dtype == np.float32 and np.array_equal(out, want)


def test_reflect101_is_numpy_reflect_padding():
    rng = np.random.RandomState(0)
    m = rng.rand(9, 11).astype(np.float32)
    for r in (1, 4, 8):
        for axis, n in ((0, 9), (1, 11)):
            pad = [(0, 0), (0, 0)]
            pad[axis] = (r, r)
            got = np.take(m, ref.reflect101(np.arange(-r, n + r), n), axis=axis)
            assert np.array_equal(got, np.pad(m, pad, mode="reflect"))


@pytest.mark.parametrize("sigma,radius,shape", [(1.0, 0, (21, 33)), (3.0, 9, (37, 53)), (12.0, 36, (37, 53))])
def test_replay_against_a_float64_separable_convolution(sigma, radius, shape):
    rng = np.random.RandomState(1)
    w = lib_taps(sigma, radius)
    r = (len(w) - 1) // 2
    m = (rng.randn(*shape) * 3).astype(np.float32)
    w64 = w.astype(np.float64)
    p = np.pad(m.astype(np.float64), ((0, 0), (r, r)), mode="reflect")
    t = sum(w64[k] * p[:, k:k + shape[1]] for k in range(2 * r + 1))
    p = np.pad(t, ((r, r), (0, 0)), mode="reflect")
    want = sum(w64[k] * p[k:k + shape[0], :] for k in range(2 * r + 1))
    got = ref.blur(m[None], w)[0]
    # two passes of r + 1 products and 2r sums with non-negative weights that sum to about 1: (2r + 3) roundings of 2^-24 .. 2^-23
    assert np.abs(got - want).max() <= (2 * r + 3) * 2.0 ** -23 * np.abs(m).max()


def test_flip_commutation_is_bitwise():
    rng = np.random.RandomState(2)
    w = lib_taps(3.0, 9)
    m = (rng.randn(2, 37, 53) * 3).astype(np.float32)
    out = ref.blur(m, w)
    assert np.array_equal(ref.blur(m[:, :, ::-1], w), out[:, :, ::-1])
    assert np.array_equal(ref.blur(m[:, ::-1, :], w), out[:, ::-1, :])


def test_normalisation_edge_cases():
    const = np.full((1, 5, 7), 0.25, np.float32)
    assert np.array_equal(ref.normalise(const, "range"), np.zeros_like(const))       # RANGE of a constant map: all zeros
    neg = -np.abs(np.random.RandomState(3).randn(2, 5, 7)).astype(np.float32)
    assert np.array_equal(ref.normalise(neg, "max"), neg)                              # MAX with mx <= 0: the identity
    zero = np.zeros((1, 5, 7), np.float32)
    assert np.array_equal(ref.normalise(zero, "max"), zero)
    m = np.random.RandomState(4).rand(1, 5, 7).astype(np.float32)
    got = ref.normalise(m, "range")
    assert got.min() == 0.0 and got.max() == 1.0
    assert ref.normalise(m, "max").max() == 1.0
    assert np.array_equal(ref.quantise(np.array([0.0, 0.5, 1.0, 2.0, -1.0, np.nan], np.float32), 255.0), [0, 128, 255, 255, 0, 0])


def test_strip_table_fits_the_lds_for_every_radius():
    from sap3d_tensorflow_amd import dataflow
    for r in range(0, 256):
        cols, rows, lds = dataflow.blur_strip(r)
        assert cols in (16, 32, 64) and rows >= 1, r
        assert lds == ((rows + 2 * r) * cols + r + 1) * 4 and lds <= 64 * 1024, (r, cols, rows, lds)
