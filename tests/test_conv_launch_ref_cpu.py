"""No-GPU checks of conv_launch_ref.py, the float64 reference of tests/test_gpu_conv_launch.py: slices against the dense oracle,
the adjoint identities of the transposed conv, the empty-class mask of a strided input gradient against where
conv3d_backward_input is identically zero, and the two halves of the fp16 assertion from the references alone."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conv_launch_ref as ref              # noqa: E402

from oracle import nn              # noqa: E402

TOL = 2e-5


@pytest.mark.parametrize("C,ld,offset", [(8, 8, 0), (8, 12, 4), (12, 36, 24), (48, 108, 0)])
def test_embed_and_outside_are_inverse(C, ld, offset):
    rng = np.random.default_rng(C + ld)
    a = rng.standard_normal((3, 5, C)).astype(np.float32)
    fill = ref.nan_fill()
    buf = ref.embed(a, ld, offset, fill)
    assert buf.shape == (15, ld)
    assert np.array_equal(buf[:, offset:offset + C], a.reshape(15, C))
    out = ref.outside(buf, C, offset)
    assert out.shape == (15, ld - C)
    # the wrappers of sap3d_tensorflow_amd.ops lay their buffers out with a pair of their own: the same floats, bit for bit
    from sap3d_tensorflow_amd import ops
    assert ref.same_bits(ops._embed(a.reshape(15, C), ld, offset, fill), buf)
    assert ref.same_bits(ops._outside(buf, C, offset), out)
    assert ref.same_bits(out, np.full((15, ld - C), fill, np.float32))
    # a conv on the slice of a wider row is the dense conv on the slice
    x = rng.standard_normal((1, 2, 3, 3, C))
    w = rng.standard_normal((1, 1, 1, C, 4))
    wide = ref.embed(x, ld, offset, 7.0).reshape(1, 2, 3, 3, ld).astype(np.float64)
    assert np.array_equal(ref.forward(wide[..., offset:offset + C], w, (1, 1, 1)), ref.forward(x.astype(np.float32), w, (1, 1, 1)))


def test_nan_fill_keeps_its_payload_and_differs_from_the_default_nan():
    f = ref.nan_fill()
    assert np.isnan(f)
    assert not ref.same_bits(np.array([f]), np.array([np.nan], np.float32))
    assert ref.same_bits(np.array([f]), np.array([ref.nan_fill()]))
    assert not ref.same_bits(np.array([0.0], np.float32), np.array([-0.0], np.float32))


@pytest.mark.parametrize("xs,k,co,s", [((1, 2, 3, 3, 4), (3, 3, 3), 8, (2, 2, 2)), ((1, 1, 3, 3, 4), (3, 3, 3), 4, (4, 4, 4)),
                                       ((2, 1, 4, 3, 8), (1, 3, 3), 4, (2, 2, 2)), ((1, 2, 3, 2, 4), (2, 3, 3), 4, (2, 2, 2))])
def test_transposed_conv_adjoint_identities(xs, k, co, s):
    """<transpose(x), g> = <x, transpose_input_grad(g)> = <K, transpose_filter_grad(x, g)> (the op is linear in x and in K)."""
    rng = np.random.default_rng(sum(xs))
    x = rng.standard_normal(xs)
    kern = rng.standard_normal(k + (co, xs[4]))
    y = ref.transpose(x, kern, s)
    assert y.shape == (xs[0], xs[1] * s[0], xs[2] * s[1], xs[3] * s[2], co)
    g = rng.standard_normal(y.shape)
    lhs = (y * g).sum()
    assert abs(lhs - (x * ref.transpose_input_grad(g, kern, s)).sum()) < 1e-10 * max(abs(lhs), 1.0)
    assert abs(lhs - (kern * ref.transpose_filter_grad(x, g, kern.shape, s)).sum()) < 1e-10 * max(abs(lhs), 1.0)
    b = rng.standard_normal(co)
    assert np.allclose(ref.transpose(x, kern, s, b), y + b, rtol=0, atol=1e-12)


@pytest.mark.parametrize("xs,k,s", [((2, 4, 14, 14, 8), (1, 1, 1), (1, 2, 2)), ((1, 4, 13, 11, 4), (1, 1, 1), (1, 2, 2)),
                                    ((1, 4, 10, 10, 4), (3, 3, 3), (2, 2, 2)), ((1, 4, 12, 12, 4), (3, 3, 3), (4, 4, 4)),
                                    ((1, 4, 12, 12, 4), (1, 3, 3), (4, 4, 4)), ((1, 2, 6, 6, 4), (2, 3, 3), (2, 2, 2)),
                                    ((1, 3, 5, 5, 4), (3, 3, 3), (1, 1, 1))])
def test_empty_mask_is_where_the_input_gradient_vanishes_for_every_dy(xs, k, s):
    """dy = 1 and w = 1 make every (tap, output) pair contribute +1 to the positions it reaches: dx > 0 there, 0 elsewhere."""
    co = 4
    oshape = (xs[0],) + tuple(-(-xs[1 + i] // s[i]) for i in range(3)) + (co,)
    dx = nn.conv3d_backward_input(np.ones(oshape), np.ones(k + (xs[4], co)), s, xs)
    mask = ref.empty_mask(xs, k, s)
    assert mask.shape == xs[1:4]
    assert np.array_equal(mask, (dx == 0).all(axis=(0, 4)))
    assert np.array_equal(~mask, (dx > 0).all(axis=(0, 4)))
    if all(kk >= ss for kk, ss in zip(k, s)):
        assert not mask.any()
    else:
        assert mask.any()


def test_accumulated_is_prior_plus_result_in_float64():
    p = np.array([1e8, -3.0], np.float32)
    r = np.array([1.0, 1e-9])
    assert np.array_equal(ref.accumulated(p, r), np.array([1e8 + 1.0, -3.0 + 1e-9]))


# K, N of the fp16 cases of the GPU test, 4096 rows, weights x 0.1
@pytest.mark.parametrize("K,N", [(64, 256), (256, 64), (32, 48), (256, 128)])
def test_fp16_reference_is_told_apart_from_the_unrounded_one(K, N):
    """Both halves of the GPU assertion have room: the rounded-operand reference is more than 10 x TOL from the un-rounded one,
    and a float32 evaluation of the rounded operands is far inside TOL of the rounded float64 one."""
    rng = np.random.default_rng(K * 1000 + N)
    x = ref.draw16(rng, (1, 4, 32, 32, K))
    w = ref.draw16(rng, (1, 1, 1, K, N), 0.1)
    assert np.abs(x).min() >= 2.0 ** -6 * (1 - 1e-6) and np.abs(x).max() <= 4.0
    assert np.abs(w).min() >= 0.1 * 2.0 ** -6 * (1 - 1e-6) > 2.0 ** -14      # no fp16 subnormal
    exact = ref.forward(x, w, (1, 1, 1))
    rounded = ref.forward(x, w, (1, 1, 1), f16=True)
    scale = np.abs(rounded).max()
    assert np.abs(rounded - exact).max() / scale > 10 * TOL
    x16 = x.astype(np.float16).astype(np.float32).reshape(-1, K)
    w16 = w.astype(np.float16).astype(np.float32).reshape(K, N)
    assert ref.f32_distance((x16 @ w16).reshape(rounded.shape), rounded) < TOL / 10
    # input-gradient direction
    dy = ref.draw16(rng, (1, 4, 32, 32, N))
    e2, r2 = ref.input_grad(dy, w, (1, 1, 1), x.shape), ref.input_grad(dy, w, (1, 1, 1), x.shape, f16=True)
    assert np.abs(r2 - e2).max() / np.abs(r2).max() > 10 * TOL
