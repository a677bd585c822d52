"""The small-tensor BatchNorm kernels (csrc/bn_small.hip) at the edges of their block -> channel-slab order (xcd_slab: the
blocks of one XCD own a contiguous run of slabs) and of their 4-channel blocks with split chains (8- and 16-channel summation
orders: below and from 512 channels), at op level through ops.bn_pass(..., path=1).

Every case is test_gpu_bn.bn_pass_case: the float64 oracle with that file's tolerances, and run-to-run bit equality.  The
shapes: row counts 1, 130, 784 (no multiple of the row stride 256 / G of any slab width) and 1024 (the kernels' limit);
channel counts 8, 24 (fewer than 8 blocks: identity order), 64, 72 (18 blocks of 4 channels, no multiple of 8), 256, 520 (not
divisible by 16: the 8-channel order above 512) and 1024.

The order itself is checked without reference to another build: BatchNorm is per-channel and a channel's sum tree does not
depend on which slab holds it, so the pass on channel-permuted operands must give the permuted results BIT FOR BIT.  An order
that drops, repeats or crosses channels cannot (the outputs start from uninitialised memory)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_gpu_bn import EPS32, bn_inputs, bn_oracle, bn_pass_case          # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = [1, 130, 784, 1024]
CHANNELS = [8, 24, 64, 72, 256, 520, 1024]
FULL = [(784, 256), (784, 1024)]            # the two shapes of the benchmark step's stage 3: every mode and option
EDGE = [(M, C) for M in ROWS for C in CHANNELS if (M, C) not in FULL]


@pytest.mark.parametrize("mode,acc2", [(0, False)] + [(m, a) for m in (1, 2, 3, 4) for a in (False, True)])
@pytest.mark.parametrize("batch", [1, 0])
@pytest.mark.parametrize("M,C", FULL)
def test_stage3_shapes_every_mode(M, C, batch, mode, acc2):
    """All five modes with batch and moving statistics, the second gradient overwritten and accumulated."""
    info = bn_pass_case(mode, M, C, 1, batch=(batch, batch), acc2=acc2)
    assert info[0] == 1


def one_row_case(mode, C):
    """bn_pass_case for M = 1, where it cannot be called: a single row has variance 0, and bn_pass_case divides its
    cancellation term 4 mu^2 / sigma^2 by that.  Here mu = 0, so the term is 0 and the bounds are bn_pass_case's with it left
    out; the checks are the same (run-to-run bits, float64 oracle for z, the gradients, the parameter gradients and the moving
    statistics).  With one row the normalised value is exactly beta, so beta keeps away from 0 to hold the ReLU margin."""
    from sap3d_tensorflow_amd import ops
    from oracle import nn
    rng = np.random.default_rng(1009 * mode + C)
    y1, y2 = bn_inputs(rng, 1, C, mode)
    bns = 2 if mode in (2, 3) else 1
    beta = rng.uniform(0.05, 0.1, (bns, C)) * np.where(rng.random((bns, C)) < 0.5, -1.0, 1.0)
    params = np.stack([np.stack([rng.uniform(0.5, 1.5, C), beta[q]]) for q in range(bns)]).astype(np.float32)
    moving = np.array([[rng.standard_normal(C), rng.uniform(0.5, 2.0, C)] for _ in range(bns)], dtype=np.float32)
    dz = rng.standard_normal((1, C)).astype(np.float32)
    z, dy1, dy2, grads, mv, info = ops.bn_pass(mode, y1, y2, params, moving, dz, path=1)
    again = ops.bn_pass(mode, y1, y2, params, moving, dz, path=1)
    for a, b in zip((z, dy1, dy2, grads, mv), again[:5]):
        assert (a is None and b is None) or np.array_equal(a, b)
    zw, g1w, g2w, gw, mvw = bn_oracle(mode, y1, y2, params, moving, dz, (1, 1))
    tol = 1e-4 + 64 * EPS32
    gis = np.abs(params[:, 0]).max() / np.sqrt(nn.BN_EPS)
    assert np.abs(z - zw).max() <= tol * max(np.abs(zw).max(), 1.0), (np.abs(z - zw).max(), info)
    gscale = np.abs(dz).max() * max(gis, 1.0)
    assert np.abs(dy1 - g1w).max() <= tol * gscale, (np.abs(dy1 - g1w).max() / gscale, info)
    if mode != 0:
        assert np.abs(dy2 - g2w).max() <= tol * gscale, info
    pscale = np.abs(gw).max() + np.abs(dz).max() * 2.0
    assert np.abs(grads - gw).max() <= tol * pscale, (np.abs(grads - gw).max() / pscale, info)
    mtol = 12 * EPS32 * np.abs(mvw).max()
    assert np.abs(mv - mvw).max() <= mtol, (np.abs(mv - mvw).max(), mtol, info)
    return info


@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("M,C", EDGE)
def test_slab_order_edges(M, C, mode):
    """One input and two normalised inputs at every other (rows, channels) pair."""
    info = one_row_case(mode, C) if M == 1 else bn_pass_case(mode, M, C, 1)
    assert info[0] == 1


@pytest.mark.parametrize("mode", [0, 1, 3])
@pytest.mark.parametrize("M,C", FULL)
def test_channel_permutation_equivariance(M, C, mode):
    """bn_pass(permuted operands) == permuted bn_pass(operands) under np.array_equal: z, dy1, dy2 (mode 1: added to what dy2
    held), dgamma / dbeta and the moving statistics."""
    from sap3d_tensorflow_amd import ops
    rng = np.random.default_rng(20 + 7 * mode + C)
    perm = rng.permutation(C)
    assert not np.array_equal(perm, np.arange(C))
    y1, y2 = bn_inputs(rng, M, C, mode)
    bns = 2 if mode == 3 else 1
    params = np.stack([np.stack([rng.uniform(0.5, 1.5, C), rng.uniform(-0.1, 0.1, C)]) for _ in range(bns)]).astype(np.float32)
    moving = np.stack([np.stack([rng.standard_normal(C), rng.uniform(0.5, 2.0, C)]) for _ in range(bns)]).astype(np.float32)
    dz = rng.standard_normal((M, C)).astype(np.float32)
    pre = rng.standard_normal((M, C)).astype(np.float32) if mode == 1 else None

    def cols(a):
        return None if a is None else np.ascontiguousarray(a[..., perm])

    z, dy1, dy2, grads, mv, info = ops.bn_pass(mode, y1, y2, params, moving, dz, acc2=pre, path=1)
    zp, dy1p, dy2p, gradsp, mvp, infop = ops.bn_pass(mode, cols(y1), cols(y2), cols(params), cols(moving), cols(dz), acc2=cols(pre),
                                                     path=1)
    assert info[0] == 1 and infop[0] == 1
    assert not np.array_equal(mv, moving)                    # batch statistics: the moving statistics were updated
    for name, a, b in (("z", z, zp), ("dy1", dy1, dy1p), ("dy2", dy2, dy2p), ("grads", grads, gradsp), ("moving", mv, mvp)):
        if a is None:
            assert b is None and mode == 0, name
            continue
        assert np.all(np.isfinite(a)), name
        assert np.array_equal(cols(a), b), name
