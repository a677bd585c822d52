"""The dropout mask of every kernel that drops out, held to its definition (include/p3d_hip.h at p3d_forward) by the CPU
replay tests/dropout_ref.py: keep(e) = u01(seed, e) >= rate with e = row * C + c the DENSE index of the element.  The other
tests read the keep pattern back from the output and hand it to the oracle; they would pass with a generator indexed by
row * ld + c or by a slab-local row, with an index or a seed cut to 32 bits, with another stream when the seed is read from device
memory (captured steps), or with one of the three copies of u01 (elementwise.hip, gn.hip, attention.hip) drifting from the
others.  Here mask equality is exact and holds at every element that can tell: wherever the value before dropout is non-zero,
the output is zero exactly where the replay drops.

BatchNorm under dropout (p3d_debug_bn_pass with drop_rate): bn_apply_kernel's mask on z and bn_bwd_gates' on dz, which serve the
dropout site of every BatchNorm structure, and the rule that a pass that drops out takes neither the small-tensor kernels nor
fold-apply (with path 0 every case reports path 3).  Modes 0-4 on test_gpu_bn.bn_inputs' sign-balanced data -- mode 4,
z = r + relu(..) with dy2 = dz * mask, tells at every element -- and mode 0 with beta = 4, where every ReLU is on (asserted on the
oracle's pre-activation).  Shapes (M, C): (130, 72), (1024, 64) -- the small kernels' without dropout --, (1025, 8) and
(2048, 64) -- fold-apply's without dropout; rates 0.5, 0.3, 0.999; seeds 11, 12 and 2^63 + 5, each as an argument and from device
memory, on dense rows and on slices (ld1, ld2, ldz all different, NaN outside that must stay).  Every run is made twice
and must be bit-identical, and the seed from device memory must give the bits of the seed as an argument.
Values: test_gpu_bn.bn_oracle followed by oracle nn.dropout with the replayed mask, within bn_pass_case's tolerances with the
scales of z and of dz multiplied by 1 / (1 - rate): the mask multiplies both by at most that factor and changes nothing else.

GroupNorm (ops.gn_pass, path 2, modes 0 and 5, row = n * R + r, strided z) and the attention block's mix (ops.attn_mix, slices,
seed and seed_dev) are held to the same replay, with test_gpu_gn's / attention_ref's oracles and tolerances fed the REPLAYED
mask.  Network: one small session per structure with a dropout site; the dropped set of the site's activation equals the replay
over (N*D*H*W, C), and kept values are base * float32(1 / (1 - rate)) within the 2e-4 of test_dropout_statistics."""
import os
import sys

import numpy as np
import pytest

from oracle import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attention_ref as ar                 # noqa: E402
import conv_launch_ref as ref              # noqa: E402
import dropout_ref as dr                   # noqa: E402
from test_gpu_bn import EPS32, bn_inputs, bn_oracle                        # noqa: E402
from test_gpu_determinism import CASES as NET_CASES                         # noqa: E402
from test_gpu_gn import gn_inputs, gn_oracle                                # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
SEEDS = [11, 12, 2 ** 63 + 5]
RATES = [0.5, 0.3, 0.999]
NAN = ref.nan_fill()


# ---- BatchNorm -----------------------------------------------------------------------------------------------------------------
BN_SHAPES = [(130, 72), (1024, 64), (1025, 8), (2048, 64)]


def bn_operands(mode, M, C, beta4, key):
    rng = np.random.default_rng([mode, M, C, int(beta4)] + list(key))
    y1, y2 = bn_inputs(rng, M, C, mode)
    bns = 2 if mode in (2, 3) else 1
    params = np.stack([np.stack([rng.uniform(0.5, 1.5, C), np.full(C, 4.0) if beta4 else rng.uniform(-0.1, 0.1, C)])
                       for _ in range(bns)]).astype(f32)
    moving = np.array([[rng.standard_normal(C), rng.uniform(0.5, 2.0, C)] for _ in range(bns)], dtype=f32)
    dz = rng.standard_normal((M, C)).astype(f32)
    return y1, y2, params, moving, dz


def run_bn(mode, y1, y2, params, moving, dz, forms=None, **kw):
    """ops.bn_pass twice (bit-identical), dense or on the slices `forms` = ((ld, off) of y1, of y2, of z) of NaN-filled rows whose
    outside must keep its bits and whose inside must hold no NaN afterwards.  Returns the dense results."""
    from sap3d_tensorflow_amd import ops
    M, C = y1.shape
    has2 = mode != 0
    if forms is None:
        args, extra = (y1, y2), {}
    else:
        def emb(a, form):
            out = np.full((M, form[0]), NAN, f32)
            out[:, form[1]:form[1] + C] = a
            return out
        nan = np.full((M, C), np.nan, f32)
        args = (emb(y1, forms[0]), emb(y2, forms[1]) if has2 else None)
        dz = emb(dz, forms[2])
        extra = dict(C_=C, offset=tuple(f[1] for f in forms), z=emb(nan, forms[2]), dy1=emb(nan, forms[0]),
                     dy2=emb(nan, forms[1]) if has2 else None)
    out = ops.bn_pass(mode, args[0], args[1], params, moving, dz, **extra, **kw)
    again = ops.bn_pass(mode, args[0], args[1], params, moving, dz, **extra, **kw)
    for a, b in zip(out[:5], again[:5]):
        assert (a is None and b is None) or ref.same_bits(a, b)
    assert out[5] == again[5]
    if forms is None:
        return out
    cut = []
    for buf, form in zip(out[:3], (forms[2], forms[0], forms[1])):
        if buf is None:
            cut.append(None)
            continue
        outside = np.delete(buf, np.s_[form[1]:form[1] + C], 1)
        assert ref.same_bits(outside, np.full(outside.shape, NAN, f32)), "floats outside the slice changed"
        cut.append(np.ascontiguousarray(buf[:, form[1]:form[1] + C]))
        assert not np.isnan(cut[-1]).any()
    return tuple(cut) + out[3:]


def bn_drop_case(mode, M, C, rate, seed, beta4=False):
    y1, y2, params, moving, dz = bn_operands(mode, M, C, beta4, [int(rate * 1000), seed % 9973])
    keep = dr.keep(seed, rate, M, C)
    s = float(dr.scale(rate))

    # the oracle: bn_oracle, then nn.dropout with the replayed mask (its backward hands bn_oracle the masked dz)
    zw0 = bn_oracle(mode, y1, y2, params, moving, dz, (1, 1))[0]
    t = nn.Tape()
    v = nn.Var(zw0)
    out = nn.dropout(t, v, float(f32(rate)), True, keep.astype(np.float64))          # (the rate the kernels get: a float32)
    out.grad = dz.astype(np.float64)
    for fn in reversed(t.ops):
        fn()
    zw = out.data
    _, g1w, g2w, gw, mvw = bn_oracle(mode, y1, y2, params, moving, v.grad, (1, 1))
    if beta4:          # every ReLU is on: every element tells
        pre = nn.batch_normalization(nn.Tape(), nn.Var(y1.astype(np.float64)), nn.Var(params[0][0].astype(np.float64)),
                                     nn.Var(params[0][1].astype(np.float64)), moving[0][0].astype(np.float64),
                                     moving[0][1].astype(np.float64), True).data
        assert mode == 0 and (pre > 0).all() and (zw0 != 0).all()
    if mode == 4:
        assert (zw0 != 0).all()
    tell = zw0 != 0
    assert tell.mean() > 0.4

    bns = 2 if mode in (2, 3) else 1
    sig2 = min(float(np.var(y.astype(np.float64), 0).min()) for y in [y1, y2][:bns])
    tol = 1e-4 + 64 * EPS32                                         # bn_pass_case's, mu = 0
    gis = np.abs(params[:, 0]).max() / np.sqrt(sig2 + nn.BN_EPS)
    zscale = max(np.abs(zw0).max(), 1.0) * s
    dzmax = np.abs(dz).max() * s
    gscale = dzmax * max(gis, 1.0)
    pscale = np.abs(gw).max() + np.sqrt(M) * dzmax * 2.0
    mtol = 12 * EPS32 * np.abs(mvw).max() + 1e-2 * 64 * EPS32 * sig2

    forms = ((C + 4, 4), (2 * C + 12, C + 12), (C + 8, 4))          # three strides, none of them C: e is not row * ld + c
    for layout in (None, forms):
        got = {}
        for dev in (False, True):
            z, dy1, dy2, grads, mv, info = run_bn(mode, y1, y2, params, moving, dz, forms=layout, drop_rate=rate, seed=seed,
                                                  seed_dev=dev)
            what = (mode, M, C, rate, seed, "sliced" if layout else "dense", "seed_dev" if dev else "seed")
            got[dev] = (z, dy1, dy2, grads, mv)
            assert info[0] == 3, what                               # a pass that drops out: finalize + apply
            # the mask, exactly
            assert np.array_equal((z == 0)[tell], ~keep[tell]), (what, int(((z == 0) != ~keep)[tell].sum()))
            if mode == 4:
                assert np.array_equal(dy2 == 0, ~keep), what        # dy2 = dz * mask
            # the values
            ez = np.abs(z - zw).max()
            e1 = np.abs(dy1 - g1w).max()
            eg = np.abs(grads - gw).max()
            print("%s: z %.3g of %.3g, dy1 %.3g of %.3g, grads %.3g of %.3g" % (what, ez, tol * zscale, e1, tol * gscale, eg,
                                                                                  tol * pscale))
            assert ez <= tol * zscale, (what, ez)
            assert e1 <= tol * gscale, (what, e1 / gscale)
            if mode != 0:
                assert np.abs(dy2 - g2w).max() <= tol * gscale, what
            assert eg <= tol * pscale, (what, eg / pscale)
            assert np.abs(mv - mvw).max() <= mtol, what
        for a, b in zip(got[False], got[True]):                     # the seed from device memory: the same stream
            assert (a is None and b is None) or ref.same_bits(a, b)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("M,C", BN_SHAPES)
@pytest.mark.parametrize("mode,beta4", [(0, False), (0, True), (1, False), (2, False), (3, False), (4, False)])
def test_bn_dropout(mode, beta4, M, C, rate, seed):
    bn_drop_case(mode, M, C, rate, seed, beta4)


@pytest.mark.parametrize("M,C,taken", [(130, 72, 1), (1024, 64, 1), (1025, 8, 3), (2048, 64, 2)])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_bn_rate_zero_is_no_dropout(mode, M, C, taken):
    """Rate 0 returns the bits of the call without dropout and takes that call's path, whatever the seed and where it is read."""
    y1, y2, params, moving, dz = bn_operands(mode, M, C, False, [0])
    plain = run_bn(mode, y1, y2, params, moving, dz)
    for dev in (False, True):
        zero = run_bn(mode, y1, y2, params, moving, dz, drop_rate=0.0, seed=2 ** 63 + 5, seed_dev=dev)
        for a, b in zip(plain[:5], zero[:5]):
            assert (a is None and b is None) or ref.same_bits(a, b)
        assert plain[5] == zero[5] and zero[5][0] == taken


def raw_bn_pass(mode, M, C, rate, path, pattern):
    """The hook itself on dense operands whose outputs hold `pattern`: (return code, z, dy1, dy2, grads, moving after)."""
    import ctypes
    from sap3d_tensorflow_amd._lib import fptr, lib
    y1, y2, params, moving, dz = bn_operands(mode, M, C, False, [1])
    z, dy1, dy2 = (np.full((M, C), pattern, f32) for _ in range(3))
    grads, mv = np.full((1, 2, C), pattern, f32), moving.copy()
    info = (ctypes.c_int * 3)(-1, -1, -1)
    rc = lib().p3d_debug_bn_pass(0, mode, M, C, fptr(y1), C, 0, fptr(y2), C, 0, fptr(params), 1, 1, 1, fptr(dz), 0, rate, 11, 0, path,
                                 fptr(z), C, 0, fptr(dy1), fptr(dy2), fptr(grads), fptr(mv), info)
    return rc, (z, dy1, dy2, grads), (mv, moving), tuple(info)


@pytest.mark.parametrize("rate,path", [(1.0, 0), (-0.25, 0), (float("nan"), 0), (1.5, 3), (0.5, 1), (0.5, 2), (0.999, 1), (0.3, 2)])
def test_bn_dropout_refusals(rate, path):
    """A rate outside [0, 1) is refused, and so are the small-tensor kernels and fold-apply for a pass that drops out ((1024, 64):
    both take the shape without dropout); a refusal writes nothing."""
    from sap3d_tensorflow_amd import ops, P3dError
    M, C, mode, pattern = 1024, 64, 1, f32(-7.25)
    if 0 < rate < 1:
        for ok in (raw_bn_pass(mode, M, C, 0.0, path, pattern), raw_bn_pass(mode, M, C, rate, 3, pattern)):
            assert ok[0] == 0 and ok[3][0] in (path, 3) and not (ok[1][0] == pattern).any()
    rc, outs, (mv, moving), info = raw_bn_pass(mode, M, C, rate, path, pattern)
    assert rc != 0
    for a in outs:
        assert ref.same_bits(a, np.full(a.shape, pattern, f32))
    assert ref.same_bits(mv, moving) and info == (-1, -1, -1)
    y1, y2, params, moving, dz = bn_operands(mode, M, C, False, [1])
    with pytest.raises(P3dError, match="does not take" if 0 < rate < 1 else "dropout rate"):
        ops.bn_pass(mode, y1, y2, params, moving, dz, drop_rate=rate, seed=11, path=path)


# ---- GroupNorm -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [11, 2 ** 63 + 5])
@pytest.mark.parametrize("rate", [0.5, 0.3])
@pytest.mark.parametrize("N,R,C,ldz", [(2, 98, 128, 140), (1, 4096, 64, 68)])
@pytest.mark.parametrize("mode", [0, 5])
def test_gn_dropout_replay(mode, N, R, C, ldz, rate, seed):
    """gn_apply_kernel and the GroupNorm backward on the statistics path, z at a row stride past C: the mask is the replay's at
    row = n * R + r (mode 5, z = gn(y1), tells at every element), and test_gpu_gn.gn_case's comparison with its oracle holds with
    the replayed mask in place of the one read back."""
    from sap3d_tensorflow_amd import ops
    G, eps = 32, 1e-5
    rng = np.random.default_rng([mode, N, R, C, int(rate * 1000), seed % 9973])
    y1, y2, cs, ss = gn_inputs(rng, mode, N, R, C, G, 0.0)
    params = np.stack([np.stack([rng.uniform(0.5, 1.5, C), rng.uniform(-0.05, 0.05, C)])]).astype(f32)
    dz = rng.standard_normal((N, R, C)).astype(f32)
    ld = (None, None, ldz)
    base = ops.gn_pass(mode, y1, y2, params, dz, G, eps=eps, path=2, ld=ld)[0]
    out = ops.gn_pass(mode, y1, y2, params, dz, G, eps=eps, path=2, ld=ld, drop_rate=rate, seed=seed)
    again = ops.gn_pass(mode, y1, y2, params, dz, G, eps=eps, path=2, ld=ld, drop_rate=rate, seed=seed)
    z, dy1, _, grads, _, taken, pads = out
    assert taken == 2 and ref.same_bits(z, again[0]) and ref.same_bits(dy1, again[1]) and ref.same_bits(grads, again[3])
    assert all(p is None or np.isnan(p).all() for p in pads)
    keep = dr.keep(seed, rate, N * R, C).reshape(N, R, C)
    tell = base != 0
    assert tell.all() if mode == 5 else tell.mean() > 0.4
    assert np.array_equal((z == 0)[tell], ~keep[tell])
    # values, and with them the backward's mask: the oracle with the replayed keep pattern, gn_case's tolerances
    zw, g1w, _, gw = gn_oracle(mode, y1, y2, params, dz, G, eps, cs, ss, keep, rate)
    sig2 = float(np.var(y1.astype(np.float64).reshape(N, R, G, -1), axis=(1, 3)).min())
    mu_max = float(np.abs(y1.astype(np.float64).reshape(N, R, G, -1).mean(axis=(1, 3))).max())
    tol = 1e-4 + 64 * EPS32 * (1.0 + mu_max ** 2 / sig2)
    s = 1.0 / (1.0 - rate)
    assert np.abs(z - zw).max() <= tol * max(np.abs(zw).max(), 1.0)
    gscale = np.abs(dz).max() * s * max(np.abs(params[:, 0]).max() / np.sqrt(sig2 + eps), 1.0)
    assert np.abs(dy1 - g1w).max() <= tol * gscale
    assert np.abs(grads - gw).max() <= tol * (np.abs(gw).max() + np.sqrt(N * R) * np.abs(dz).max() * s * 2.0)


# ---- the attention block's mix -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [11, 2 ** 63 + 5])
@pytest.mark.parametrize("rate", [0.5, 0.3])
@pytest.mark.parametrize("C", [32, 36])
@pytest.mark.parametrize("M", [3, 777, 4099])
def test_attn_mix_dropout_replay(M, C, rate, seed):
    """attn_mix on slices (strides and offsets of test_mix_slices): z == 0 exactly where the replay drops and r * gamma + x is
    non-zero, dr and dx are zero exactly there, with the seed as an argument and in device memory; values by attention_ref's rule."""
    from sap3d_tensorflow_amd import ops
    gamma, extra, offset = -0.7, (8, 12, 16), (4, 8, 12)
    rng = np.random.default_rng([M, C, int(rate * 1000), seed % 9973])
    r, x, dz = (rng.standard_normal((M, C)).astype(f32) for _ in range(3))

    def emb(a, k):
        out = np.full((M, C + extra[k]), NAN, f32)
        out[:, offset[k]:offset[k] + C] = a
        return out

    def cut(buf, k):
        outside = np.delete(buf, np.s_[offset[k]:offset[k] + C], 1)
        assert ref.same_bits(outside, np.full(outside.shape, NAN, f32)), "guard columns"
        return buf[:, offset[k]:offset[k] + C]
    nan = np.full((M, C), np.nan, f32)
    keep = dr.keep(seed, rate, M, C)
    base = ar.mix(r, x, gamma, dtype=f32)
    assert (base != 0).all() and (dz != 0).all()
    runs = []
    for dev in (False, True):
        zb, drb, dxb, dgm = ops.attn_mix(emb(r, 0), emb(x, 1), gamma, C, offset=offset, drop_rate=rate, seed=seed, seed_dev=dev,
                                         z=emb(nan, 2), dz=emb(dz, 2), dr=emb(nan, 0), dx=emb(nan, 1), dgamma=0.375)
        z, g_r, g_x = cut(zb, 2), cut(drb, 0), cut(dxb, 1)
        assert np.array_equal(z == 0, ~keep), ("z", dev, int(((z == 0) != ~keep).sum()))
        assert np.array_equal(g_r == 0, ~keep) and np.array_equal(g_x == 0, ~keep), ("backward", dev)
        tag = "mix %dx%d rate %g seed %d dev %d" % (M, C, rate, seed, dev)
        ar.rule(z, ar.mix(r, x, gamma, keep, rate), ar.mix(r, x, gamma, keep, rate, f32), what=tag + " z")
        w64, w32 = ar.mix_bwd(dz, r, gamma, keep, rate, None, 0.375), ar.mix_bwd(dz, r, gamma, keep, rate, None, 0.375, f32)
        ar.rule(g_r, w64[0], w32[0], what=tag + " dr")
        ar.rule(g_x, w64[1], w32[1], what=tag + " dx")
        ar.rule(np.array([dgm]), np.array([w64[2]]), np.array([w32[2]]), what=tag + " dgamma")
        runs.append((zb, drb, dxb, np.array([dgm], f32)))
    assert all(ref.same_bits(a, b) for a, b in zip(*runs))


# ---- the network ---------------------------------------------------------------------------------------------------------------
SITES = {"unet": "deconv3_re", "concat": "deconv1_revise", "unet++nonsa": "x_1_3", "unet++ds": "x_1_3_sa",
         "gn_p3d": "deconv_revise", "gn_p3d_decoder": "decoder2_conv2"}
NET = {}
for _st, _cfg, _shape in NET_CASES:
    NET.setdefault(_st, (_cfg, _shape))          # (the first config of a structure that test_gpu_determinism has two of)


def site_is_the_replay(base, dropped, rate, seed, what=""):
    """The checks of a dropout site's activation `dropped` against the one without dropout: the dropped set is the replay's over
    (N*D*H*W, C) wherever base is non-zero, and kept values are base * float32(1 / (1 - rate)) within 2e-4."""
    C = base.shape[-1]
    keep = dr.keep(seed, rate, base.size // C, C).reshape(base.shape)
    tell = base != 0
    assert tell.mean() > 0.1, what
    assert np.array_equal((dropped == 0)[tell], ~keep[tell]), (what, int(((dropped == 0) != ~keep)[tell].sum()), int(tell.sum()))
    assert (dropped[~tell] == 0).all(), what
    kept = tell & keep
    assert np.abs(dropped[kept] - base[kept] * dr.scale(rate)).max() < 2e-4, what
    return keep


@pytest.mark.parametrize("rate", [0.5, 0.3])
@pytest.mark.parametrize("structure", sorted(SITES))
def test_network_site_mask_is_the_replay(structure, rate):
    from sap3d_tensorflow_amd import P3DSession
    from oracle import p3d
    cfg, shape = NET[structure]
    s = P3DSession(structure, batch=shape[0], frames=shape[1], height=shape[2], width=shape[3], base=cfg.base, blocks=cfg.blocks,
                   seed=1)
    try:
        x = p3d.synthetic_clip(0, shape + (3,))
        s.forward(x, 0.0, True)
        base = s.activation(SITES[structure])
        masks = []
        for seed in (11, 2 ** 63 + 5):
            s.forward(x, rate, True, seed)
            masks.append(site_is_the_replay(base, s.activation(SITES[structure]), rate, seed, (structure, rate, seed)))
        assert 0.3 < (masks[0] != masks[1]).mean() < 0.7
    finally:
        s.close()
