"""Op-level parity of the GroupNorm passes (gn.hip, through p3d_debug_gn_pass) and of CBAM (cbam.hip, through p3d_debug_cbam)
against the float64 oracle (oracle/nn.py group_norm / reduce_max, oracle/p3d_gn.py channel_attention / spatial_attention),
element by element.  Every hook case runs twice and must be bit-equal run to run.

GroupNorm has two implementations, chosen by p3d_gn_small_ok: the one-launch small-tensor kernels (a (sample, group) slab
of R rows x C/G channels with R * C/G / 4 <= 2048, two-pass moments in float32 registers) and statistics -> finalize ->
apply (var = E[y^2] - mean^2 in double from float32 per-slice partials).  The cases sit on both sides of that boundary and
force each path where both take the shape.

Inputs.  Every (sample, group) slab of a GroupNorm input is mu_g + delta_c + p, where the parts p have magnitude >= 0.5 and
sum to exactly zero over the slab (pairs p, -p; one triple a, b, -(a + b) when the slab is odd) and the channel offsets
delta_c in [-0.2, 0.2] also sum to zero over the group.  The group mean is then mu_g and every normalised value is at least
0.3 / sigma away from zero; with gamma in [0.5, 1.5] and |beta| <= 0.05 no ReLU argument comes within ~0.09 of zero, and a
residual that meets a ReLU has the sign of its element.  A ReLU decision that flipped between float32 and float64 would
otherwise move a whole element of the gradient.

GroupNorm tolerances (those of tests/test_gpu_bn.py, none looser).  z within 1e-4 of its scale.  The backward of a
normalisation cancels, so every gradient is compared within 1e-4 of the scale of its terms: max|dz| * max(gamma * invstd, 1)
for the input gradients, max|want| + sqrt(N R) * max|dz| * 2 for dgamma / dbeta (sums of N R terms).
Offset means: the statistics path forms var = sum(y^2) / n - mean^2 from float32 partials.  A float32 partial sum of k squares
carries a rounding error of at most about sqrt(k) * eps32 * k * (sigma^2 + mu^2), and the double-precision fold adds nothing
comparable, so |d var| <~ K * eps32 * (sigma^2 + mu^2) with K = sqrt(k) of the largest partial.  The launcher's partials
cover at most ceil(R / slices) <= 4096 rows here (asserted per case), so K = 64 bounds them; it is the K of the BatchNorm
file.  That bound, against the statistics of the kernel's own y in float64, is asserted on the mean / invstd tables of both
paths, and K * eps32 * (1 + mu^2 / sigma^2) is added to every relative tolerance above.

CBAM.  x is drawn from a coarse grid (multiples of 1/64, then ReLU) with ties built in: whole-zero channels (a channel max
tied over R rows), whole-zero positions (a spatial max tied over C channels), and channel maxima repeated over many rows.
At every other position one channel's x is at least twice any other's; with cs in about [0.35, 0.65] the spatial maximum
of x * cs then leads by more than 8 %, so float32 and float64 agree on it.  The spatial stage (sp, ss, dK7) is compared
against the oracle fed the kernel's own cs, products rounded to float32, so that its tie sets are decided by the same
float32 products the kernel compares; the channel stage (cs, dx, the MLP's gradients) against the full float64 oracle.
Tolerance: 1e-4 of the scale of each quantity (for sums over positions, of max|want| + sqrt(M) * the largest term).  Every
parameter gradient is added to what it held, exactly: the result with a prefilled gradient is float32(prefill + result from
zero), bit for bit."""
import numpy as np
import pytest

from oracle import nn
from oracle import p3d_gn
from oracle.p3d import Graph

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
D2 = (1, 3, 4, 6)          # modes with a second input gradient


# ---- GroupNorm ---------------------------------------------------------------------------------------------------------------
def zero_sum_parts(rng, N, R, C, G):
    """[N, R, C] float64, |v| >= 0.5, summing to exactly zero over every (sample, group) slab."""
    cg = C // G
    n = R * cg
    assert n >= 2
    u = 0.5 + rng.random((N * G, n))
    v = u.copy()
    k = 3 if n % 2 else 0
    if k:
        v[:, 2] = -(u[:, 0] + u[:, 1])
    half = (n - k) // 2
    v[:, k + half:] = -u[:, k:k + half]
    v = np.take_along_axis(v, rng.permuted(np.tile(np.arange(n), (N * G, 1)), axis=1), 1)
    return v.reshape(N, G, R, cg).transpose(0, 2, 1, 3).reshape(N, R, C)


def channel_deltas(C, G):
    cg = C // G
    ramp = np.linspace(-0.2, 0.2, cg) if cg > 1 else np.zeros(1)
    return np.tile(ramp, G)


def gn_inputs(rng, mode, N, R, C, G, mu):
    mug = np.repeat(mu * (0.9 + 0.2 * rng.random(G)), C // G)
    p1 = zero_sum_parts(rng, N, R, C, G)
    y1 = mug + channel_deltas(C, G) + p1
    sgn = np.sign(p1)
    cs = ss = None
    if mode in (1, 4):
        y2 = sgn * (0.2 + rng.random((N, R, C)))
    elif mode == 2:
        y2 = 2.0 * mug + channel_deltas(C, G) + 1.5 * p1        # second GN input: same sign after normalisation
    elif mode == 3:
        y2 = -mug + channel_deltas(C, G) + zero_sum_parts(rng, N, R, C, G)
    elif mode == 6:
        y2 = sgn * (0.2 + rng.random((N, R, C)))
        cs = rng.uniform(0.3, 1.0, (N, C)).astype(np.float32)
        ss = rng.uniform(0.3, 1.0, (N, R)).astype(np.float32)
    else:
        y2 = None
    f = lambda a: a.astype(np.float32) if a is not None else None
    return f(y1), f(y2), cs, ss


def gn_oracle(mode, y1, y2, params, dz, G, eps, cs=None, ss=None, keep=None, rate=0.0):
    """float64 tape: group_norm + relu + add (+ dropout), then the backward from dz.  Returns (z, dy1, dy2, grads)."""
    N, R, C = y1.shape
    shp = (N, R, 1, 1, C)
    t = nn.Tape()
    gns = 2 if mode in (2, 3) else 1
    g = [nn.Var(params[q][0].astype(np.float64)) for q in range(gns)]
    b = [nn.Var(params[q][1].astype(np.float64)) for q in range(gns)]
    v1 = nn.Var(y1.astype(np.float64).reshape(shp))
    n1 = nn.group_norm(t, v1, g[0], b[0], G, eps)
    v2 = None
    if y2 is not None:
        y2d = y2.astype(np.float64)
        if mode == 6:      # the kernel's dy2 is the gradient of the CBAM output r * cs * ss
            y2d = y2d * cs.astype(np.float64)[:, None, :] * ss.astype(np.float64)[:, :, None]
        v2 = nn.Var(y2d.reshape(shp))
    if mode == 0:
        out = nn.relu(t, n1)
    elif mode in (1, 6):
        out = nn.relu(t, nn.add(t, n1, v2))
    elif mode == 2:
        out = nn.relu(t, nn.add(t, n1, nn.group_norm(t, v2, g[1], b[1], G, eps)))
    elif mode == 3:
        out = nn.add(t, nn.relu(t, n1), nn.relu(t, nn.group_norm(t, v2, g[1], b[1], G, eps)))
    elif mode == 4:
        out = nn.add(t, v2, nn.relu(t, n1))
    else:
        out = n1
    if rate:
        out = nn.dropout(t, out, rate, True, keep.reshape(shp).astype(np.float64))
    if mode == 2:
        return out.data.reshape(N, R, C), None, None, None
    out.grad = dz.astype(np.float64).reshape(shp)
    for fn in reversed(t.ops):
        fn()
    grads = np.stack([np.stack([g[q].grad, b[q].grad]) for q in range(gns)])
    dy2 = None
    if mode in D2:
        dy2 = v2.grad.reshape(N, R, C) if v2.grad is not None else np.zeros((N, R, C))
    return out.data.reshape(N, R, C), v1.grad.reshape(N, R, C), dy2, grads


def slice_rows(R, C):
    """Rows per channel that one float32 partial of gn_stats_kernel / gn_bwd_reduce_kernel covers (slice_grid, gn.hip)."""
    rpi = 256 // (C // 4)
    slices = min(max(-(-R // (rpi * 32)), 1), 256)
    return -(-R // slices)


def check_stats(y, tables, G, eps, q):
    """The mean / invstd tables of GN q against the statistics of the kernel's own y: the docstring's cancellation bound."""
    N, R, C = y.shape
    cg = C // G
    yg = y.astype(np.float64).reshape(N, R, G, cg)
    m = yg.mean(axis=(1, 3))
    v = ((yg - m[:, None, :, None]) ** 2).mean(axis=(1, 3))
    m_c, v_c = np.repeat(m, cg, axis=1), np.repeat(v, cg, axis=1)
    mean, invstd = tables[q, 2].astype(np.float64), tables[q, 3].astype(np.float64)
    var_got = 1.0 / invstd ** 2 - eps
    sig2, mu2 = v_c.max(), (m_c ** 2).max()
    bound = 64 * EPS32 * (sig2 + mu2) + 4 * EPS32 * (sig2 + eps)     # (+ the float32 rounding of invstd itself)
    assert np.abs(var_got - v_c).max() <= bound, (np.abs(var_got - v_c).max(), bound)
    assert np.abs(mean - m_c).max() <= 64 * EPS32 * np.sqrt(sig2 + mu2)


def run_gn(mode, y1, y2, params, dz, G, **kw):
    from sap3d_tensorflow_amd import ops
    out = ops.gn_pass(mode, y1, y2, params, dz, G, **kw)
    again = ops.gn_pass(mode, y1, y2, params, dz, G, **kw)
    for a, b in zip(out[:5], again[:5]):                              # bit-reproducible run to run
        assert (a is None and b is None) or np.array_equal(a, b, equal_nan=True)
    assert out[5] == again[5]
    return out


def gn_case(mode, N, R, C, G=32, path=0, eps=1e-5, mu=0.0, acc2=False, prefill=False, ld=(None, None, None), drop=0.0,
            seed=0):
    """Checks one pass against the oracle; returns (path taken, the hook's results)."""
    # (the path is not part of the seed: forced paths see the same input)
    rng = np.random.default_rng(seed + 1009 * mode + 17 * R + 3 * C + 7 * G + 11 * N + int(acc2) + int(100 * mu))
    assert slice_rows(R, C) <= 4096                                  # K = 64 of the docstring covers the partials
    y1, y2, cs, ss = gn_inputs(rng, mode, N, R, C, G, mu)
    gns = 2 if mode in (2, 3) else 1
    params = np.stack([np.stack([rng.uniform(0.5, 1.5, C), rng.uniform(-0.05, 0.05, C)]) for _ in range(gns)]).astype(np.float32)
    dz = rng.standard_normal((N, R, C)).astype(np.float32)
    pre = rng.standard_normal((N, R, C)).astype(np.float32) if (acc2 and mode in D2) else None
    grads0 = rng.standard_normal((gns, 2, C)).astype(np.float32) if prefill else None
    z, dy1, dy2, grads, tables, taken, pads = run_gn(mode, y1, y2, params, dz, G, eps=eps, cs=cs, ss=ss, acc2=pre, grads=grads0,
                                                     drop_rate=drop, seed=1234 + seed, path=path, ld=ld)
    for p in pads:                                                     # nothing is written past column C
        assert p is None or np.isnan(p).all()
    keep = None
    if drop:
        keep = z != 0
    zw, g1w, g2w, gw = gn_oracle(mode, y1, y2, params, dz, G, eps, cs, ss, keep, drop)

    for q, y in enumerate([y1, y2][:gns]):
        check_stats(y, tables, G, eps, q)
    sig2 = min(float(np.var(y.astype(np.float64).reshape(N, R, G, -1), axis=(1, 3)).min()) for y in [y1, y2][:gns])
    mu_max = max(float(np.abs(y.astype(np.float64).reshape(N, R, G, -1).mean(axis=(1, 3))).max()) for y in [y1, y2][:gns])
    tol = 1e-4 + 64 * EPS32 * (1.0 + mu_max ** 2 / sig2)
    scale_drop = 1.0 / (1.0 - drop) if drop else 1.0
    assert np.abs(z - zw).max() <= tol * max(np.abs(zw).max(), 1.0), (np.abs(z - zw).max(), taken)
    if mode == 2:
        assert dy1 is None and grads is None
        return taken, (z, tables)
    gis = np.abs(params[:, 0]).max() / np.sqrt(sig2 + eps)
    gscale = np.abs(dz).max() * scale_drop * max(gis, 1.0)
    assert np.abs(dy1 - g1w).max() <= tol * gscale, (np.abs(dy1 - g1w).max() / gscale, taken)
    if mode in D2:
        want2 = g2w + (pre.astype(np.float64) if pre is not None else 0.0)
        assert np.abs(dy2 - want2).max() <= tol * (gscale + (np.abs(pre).max() if pre is not None else 0.0)), taken
    else:
        assert dy2 is None
    pscale = np.abs(gw).max() + np.sqrt(N * R) * np.abs(dz).max() * scale_drop * 2.0
    assert np.abs(grads - gw).max() <= tol * pscale, (np.abs(grads - gw).max() / pscale, taken)
    return taken, (z, dy1, dy2, grads, tables, keep, y1)


def small_ok(R, C, G):
    cpg = C // G
    return C % G == 0 and cpg % 4 == 0 and 256 % (cpg // 4) == 0 and R * (cpg // 4) <= 2048


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("mode,acc2", [(0, False), (5, False)] + [(m, a) for m in D2 for a in (False, True)])
def test_gn_modes(mode, acc2, path):
    """Every mode with a backward, on both paths at one shape (C = 128, G = 32, R = 98: the small kernels take it), the
    second gradient overwritten and accumulated."""
    taken, _ = gn_case(mode, 2, 98, 128, path=path, acc2=acc2)
    assert taken == path


@pytest.mark.parametrize("path,taken", [(0, 2), (2, 2), (1, None)])
@pytest.mark.parametrize("G,eps", [(32, 1e-5), (128, 1e-3)])
def test_gn_mode2_forward(path, taken, G, eps):
    """Mode 2, relu(gn1(y1) + gn2(y2)), forward only: the statistics path at every shape; the small kernels refuse it."""
    from sap3d_tensorflow_amd import P3dError
    if taken is None:
        with pytest.raises(P3dError, match="does not take"):
            gn_case(2, 2, 98, 128, G=G, eps=eps, path=path)
        return
    assert gn_case(2, 2, 98, 128, G=G, eps=eps, path=path)[0] == taken


@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("C,R", [(128, 2048), (256, 1024), (1024, 256)])      # cpg 4, 8, 32: R * cpg / 4 = 2048
@pytest.mark.parametrize("extra", [0, 1])
def test_gn_small_boundary(C, R, extra, mode):
    """Both sides of the small-path boundary: the network's rule, then each path forced; one row more is refused by the
    small kernels.  Both paths must agree with the oracle on the same input."""
    from sap3d_tensorflow_amd import P3dError
    R += extra
    assert small_ok(R, C, 32) == (extra == 0)
    taken, _ = gn_case(mode, 1, R, C)
    assert taken == (1 if extra == 0 else 2)
    if extra == 0:
        assert gn_case(mode, 1, R, C, path=2)[0] == 2
    else:
        with pytest.raises(P3dError, match="does not take"):
            gn_case(mode, 1, R, C, path=1)


@pytest.mark.parametrize("C,drop", [(32, 0.0), (64, 0.0), (128, 0.25)])      # cpg 1, cpg 2, dropout
def test_gn_small_refuses(C, drop):
    from sap3d_tensorflow_amd import P3dError
    mode = 0
    assert gn_case(mode, 2, 98, C, drop=drop)[0] == 2
    with pytest.raises(P3dError, match="does not take"):
        gn_case(mode, 2, 98, C, drop=drop, path=1)


@pytest.mark.parametrize("C", [64, 256, 1024])
@pytest.mark.parametrize("mode", [0, 2])
def test_gn_per_sample_batchnorm(C, mode):
    """G = C with eps 1e-3: the per-sample BatchNorm of p3d_predict_windows (mode 2 is its projected block end)."""
    assert gn_case(mode, 2, 98, C, G=C, eps=1e-3)[0] == 2


@pytest.mark.parametrize("N,R,C,path", [(1, 98, 128, 1), (3, 98, 128, 1), (3, 98, 128, 2), (1, 1, 256, 1), (2, 1, 256, 2),
                                         (2, 1001, 64, 2), (3, 333, 256, 1), (3, 333, 256, 2), (1, 40000, 256, 2)])
def test_gn_rows(N, R, C, path):
    """N = 1 and 3, R = 1, ragged R, and R = 40000 at C = 256: past the 256-slice cap of slice_grid (above R = 32768)."""
    assert gn_case(0, N, R, C, path=path)[0] == path
    if R > 32768:
        assert slice_rows(R, C) > 128                      # every slice partial covers more rows than below the cap


@pytest.mark.parametrize("C", [96, 160, 224])
@pytest.mark.parametrize("mode", [0, 3, 5])
def test_gn_groups_not_power_of_two(C, mode):
    """C / G = 3, 5, 7 with G = 32: the finalize folds must sum exactly the group's channels (they used to fold with xor
    shuffles, which mix in the neighbouring group's lanes when C / G is not a power of two)."""
    from sap3d_tensorflow_amd import P3dError
    assert gn_case(mode, 2, 98, C)[0] == 2
    with pytest.raises(P3dError, match="does not take"):
        gn_case(mode, 2, 98, C, path=1)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("mode", [1, 3, 6])
def test_gn_strided(mode, path):
    """Row strides past C for y1 / dy1, y2 / dy2 and z / dz (the concat heads' views); the pad columns hold NaN and must be
    neither read nor written."""
    assert gn_case(mode, 2, 98, 128, path=path, ld=(132, 136, 140), acc2=True)[0] == path


@pytest.mark.parametrize("mode", [0, 3])
def test_gn_param_grads_stored(mode):
    """dgamma / dbeta are stored, not added, on both paths (prefilled with values; every other case prefills NaN), and both
    paths agree."""
    _, r1 = gn_case(mode, 2, 98, 128, path=1, prefill=True)
    _, r2 = gn_case(mode, 2, 98, 128, path=2, prefill=True)
    g1, g2 = r1[3], r2[3]
    assert np.abs(g1 - g2).max() <= 1e-4 * (np.abs(g2).max() + np.sqrt(2 * 98) * 8.0)


@pytest.mark.parametrize("mode", [0, 5])
@pytest.mark.parametrize("R,C", [(4096, 64), (98, 128)])
def test_gn_dropout(mode, R, C):
    """Dropout on z: the keep pattern is read back from z (the oracle's backward then applies it, so a backward with another
    mask fails the dy1 comparison), and the keep fraction is within 4 sigma of 1 - rate."""
    rate = 0.3
    N = 2
    _, (z, dy1, _, _, tables, keep, y1) = gn_case(mode, N, R, C, drop=rate)
    if mode == 5:
        seen = keep                                           # gn(y1) is never 0: z == 0 exactly where dropped
    else:                                                     # z == 0 wherever the ReLU is off: only its on-set tells
        on = tables[0, 0][:, None, :] * y1 + tables[0, 1][:, None, :] > 0
        seen = keep[on]
    frac = seen.mean()
    assert abs(frac - (1 - rate)) <= 4 * np.sqrt(rate * (1 - rate) / seen.size), (frac, seen.size)


@pytest.mark.parametrize("mu", [0.0, 4.0, 16.0])
@pytest.mark.parametrize("N,R,C,path", [(2, 98, 128, 1), (2, 98, 128, 2), (2, 2048, 128, 1), (1, 40000, 256, 2)])
@pytest.mark.parametrize("mode", [0, 5])
def test_gn_offset_means(mu, N, R, C, path, mode):
    """Group means at 0, 4 sigma and 16 sigma (sigma ~ 1), channels of one group at different offsets: the tables within the
    docstring's cancellation bound on both paths, including the statistics path past the slice cap."""
    assert gn_case(mode, N, R, C, path=path, mu=mu)[0] == path


# ---- CBAM --------------------------------------------------------------------------------------------------------------------
def cbam_inputs(rng, N, D, H, W, C, ld=None):
    """x on the 1/64 grid with the docstring's ties, and parameters that keep cs in about [0.35, 0.65]."""
    R, Ch = D * H * W, C // 8
    x = np.maximum(rng.integers(-32, 64, (N, R, C)) / 64.0, 0.0)           # ~1/3 zeros, the rest in (0, 1)
    zc = rng.choice(C, max(1, C // 8), replace=False)                      # whole-zero channels
    live = np.setdiff1d(np.arange(C), zc)
    win = live[rng.integers(0, live.size, (N, R))]
    np.put_along_axis(x, win[:, :, None], rng.choice([2.0, 3.0, 4.0], (N, R, 1)), axis=2)    # maxima repeated over rows
    x[:, :, zc] = 0.0
    zp = rng.choice(R, max(1, R // 8), replace=False)                      # whole-zero positions
    x[:, zp, :] = 0.0
    p = dict(k0=rng.normal(0, 0.1 / np.sqrt(C), (C, Ch)), b0=rng.uniform(-0.05, 0.05, Ch),
             k1=rng.normal(0, 0.1 / np.sqrt(Ch), (Ch, C)), b1=rng.uniform(-0.2, 0.2, C),
             k7=rng.normal(0, 0.05, (7, 7, 7, 2, 1)))
    p = {k: v.astype(np.float32) for k, v in p.items()}
    dout = rng.standard_normal((N, D, H, W, C)).astype(np.float32)
    return x.reshape(N, D, H, W, C).astype(np.float32), p, dout


def cbam_oracle(x, p, dout, cs32=None):
    """oracle/p3d_gn.py's channel_attention -> spatial_attention in float64, backward from dout.  cs32: skip the channel stage
    and feed the spatial stage f = x * cs32 with float32 products.  Returns (tape variables by name, x Var, f Var)."""
    names = {"ch/mlp_0/kernel": "k0", "ch/mlp_0/bias": "b0", "ch/mlp_1/kernel": "k1", "ch/mlp_1/bias": "b1",
             "sp/conv3d/kernel": "k7"}
    g = Graph(params={k: p[v].astype(np.float64) for k, v in names.items()}, dtype=np.float64, create=False)
    xv = nn.Var(x.astype(np.float64))
    if cs32 is None:
        f = p3d_gn.channel_attention(g, xv, "ch")
    else:
        f = nn.Var((x * cs32[:, None, None, None, :]).astype(np.float64))
    out = p3d_gn.spatial_attention(g, f, "sp")
    out.grad = dout.astype(np.float64)
    for fn in reversed(g.tape.ops):
        fn()
    return {names[k]: v.grad for k, v in g.trainable.items()}, xv, f


def spatial_forward(f):
    """sp = [mean_c f, max_c f] and ss = sigmoid(conv7(sp)) (utils/network.py:251-274) for the spatial comparison."""
    t = nn.Tape()
    v = nn.Var(f)
    sp = nn.concat(t, [nn.reduce_mean(t, v, (4,)), nn.reduce_max(t, v, (4,))])
    return sp.data, sp


def close(got, want, scale, what):
    err = np.abs(got.astype(np.float64) - want).max()
    assert err <= 1e-4 * scale, (what, err, scale)


def run_cbam(x, p, dout, **kw):
    from sap3d_tensorflow_amd import ops
    out = ops.cbam(x, p["k0"], p["b0"], p["k1"], p["b1"], p["k7"], dout, **kw)
    again = ops.cbam(x, p["k0"], p["b0"], p["k1"], p["b1"], p["k7"], dout, **kw)
    for a, b in zip(out[:4] + out[4], again[:4] + again[4]):          # bit-reproducible run to run
        assert np.array_equal(a, b, equal_nan=True)
    assert out[5] == again[5]
    return out


def cbam_case(N, D, H, W, C, chunks=0, accx=False, prefill=False, ld=None, seed=0):
    rng = np.random.default_rng(seed + 131 * C + 17 * D + 7 * H + W + N + chunks)
    x, p, dout = cbam_inputs(rng, N, D, H, W, C)
    R, M = D * H * W, N * D * H * W
    xr = x.reshape(N, R, C)
    assert (xr.max(axis=1) == 0).any() and (xr.max(axis=2) == 0).any()                 # both kinds of whole-zero ties
    dx0 = rng.standard_normal(x.shape).astype(np.float32) if accx else None
    pg0 = [rng.standard_normal(p[k].shape).astype(np.float32) for k in ("k0", "b0", "k1", "b1", "k7")] if prefill else None
    cs, sp, ss, dx, pg, used, pad = run_cbam(x, p, dout, chunks=chunks, dx=dx0, pgrads=pg0, ld=ld)
    assert np.isnan(pad).all()                                                        # nothing is written past column C
    assert used == (chunks if chunks else min(max(R // 16, 1), 64))

    # channel stage: the full float64 oracle
    grads, xv, f = cbam_oracle(x, p, dout)
    cs_want = f.data.reshape(N, R, C).max(axis=1) / np.where(xr.max(axis=1) > 0, xr.max(axis=1), 1.0)
    live = xr.max(axis=1) > 0
    close(np.where(live, cs, 0.0), np.where(live, cs_want, 0.0), 1.0, "cs")
    dx_want = xv.grad + (dx0.astype(np.float64) if accx else 0.0)
    close(dx, dx_want, np.abs(dx_want).max(), "dx")
    # spatial stage: the oracle fed the kernel's cs, products rounded to float32
    sgrads, _, fs = cbam_oracle(x, p, dout, cs32=cs)
    sp_want, _ = spatial_forward(fs.data)
    close(sp, sp_want, np.abs(sp_want).max(), "sp")
    t = nn.Tape()
    ss_want = nn.sigmoid(t, nn.conv3d(t, nn.Var(sp_want), nn.Var(p["k7"].astype(np.float64)))).data[..., 0]
    close(ss, ss_want, 1.0, "ss")
    term = np.abs(sp_want).max() * np.abs(dout).max() * np.abs(fs.data).max() * 0.25
    pre = pg0 if prefill else [0.0] * 5
    for k, got, want, p0 in zip(("k0", "b0", "k1", "b1"), pg[:4], [grads[k] for k in ("k0", "b0", "k1", "b1")], pre[:4]):
        close(got - p0 if prefill else got, want, np.abs(want).max(), "d" + k)
    dk7 = pg[4] - pre[4] if prefill else pg[4]
    close(dk7, sgrads["k7"], np.abs(sgrads["k7"]).max() + np.sqrt(M) * term, "dk7")
    return (cs, sp, ss, dx, pg, used), pg0


@pytest.mark.parametrize("C", [8, 40, 256, 288, 1024])
def test_cbam_widths(C):
    """C = 8 (Ch = 1), 40 (Ch = 5: the scalar tail of bwd_mlp2a), 256, 288 (C > 256: strided channel loops, vector loop and
    tail) and 1024."""
    cbam_case(2, 2, 7, 7, C)


@pytest.mark.parametrize("dhw", [(1, 3, 3), (2, 7, 7), (4, 14, 14), (8, 13, 10)])
def test_cbam_maps(dhw):
    """Maps smaller than the 7x7x7 halo (D = 1, 2) up to R = 1040, where the network's chunk rule leaves two chunks empty."""
    cbam_case(2, *dhw, 64)


@pytest.mark.parametrize("dhw", [(16, 32, 32), (16, 32, 33)])
def test_cbam_k7_blocks(dhw):
    """M = 16384 and 16896: bwd_k7_kernel's grid reaches its 256-block cap, then each block takes several position chunks."""
    cbam_case(1, *dhw, 16)


@pytest.mark.parametrize("dhw,chunks", [((1, 3, 3), 1), ((1, 3, 3), 9), ((1, 3, 3), 20), ((1, 3, 3), 64), ((2, 7, 7), 1),
                                        ((2, 7, 7), 200)])
def test_cbam_forced_chunks(dhw, chunks):
    """One chunk per sample, and more chunks than rows (empty chunks)."""
    cbam_case(2, *dhw, 64, chunks=chunks)


def test_cbam_accumulates():
    """accx = 1 adds to a prefilled dx; every parameter gradient is added to, exactly: float32(prefill + result from zero)."""
    (_, _, _, _, pg0, _), _ = cbam_case(2, 2, 7, 7, 64)
    (_, _, _, _, pg1, _), pre = cbam_case(2, 2, 7, 7, 64, accx=True, prefill=True)
    for a, b, q in zip(pg1, pg0, pre):
        assert np.array_equal(a, (q + b).astype(np.float32))


@pytest.mark.parametrize("accx", [False, True])
def test_cbam_strided(accx):
    """x and dx with rows of C + 4 floats (NaN in the pad columns: neither read nor written)."""
    cbam_case(2, 2, 7, 7, 64, ld=68, accx=accx)
