"""Helpers and float64 references for the non-finite contract of include/p3d_hip.h ("Non-finite values").

The contract in one line: a forward kernel's output is NaN / +inf / -inf exactly where the float64 reference of the same
operation is, every other element is finite, and where the operation couples nothing across the poisoned element the
finite elements keep the bits of the clean launch.  The references here are written with propagating primitives
(relu = np.maximum, a max-pool window holding a NaN gives NaN, sums are sums) and select gates in the backward pass
(np.where(pre > 0, g, 0), never g * mask).  References that already exist (conv_launch_ref, fused_bn_ref, attention_ref,
map_loss_ref, opt_ref, oracle.nn) are reused by the tests; only what they lack lives here."""
import numpy as np

from oracle import nn

NAN, PINF, NINF, NZERO = np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(-0.0)
SPECIALS = {"nan": NAN, "+inf": PINF, "-inf": NINF, "-0": NZERO}


def plant(rng, a, specials, k):
    """A copy of `a` with k values drawn (with repetition) from `specials` at k distinct drawn positions.  Returns (the copy,
    the flat positions)."""
    out = np.array(a, copy=True)
    flat = out.reshape(-1)
    pos = rng.choice(flat.size, size=k, replace=False)
    sp = np.asarray(list(specials), dtype=out.dtype)
    flat[pos] = sp[rng.integers(0, sp.size, size=k)]
    return out, pos


def footprint_equal(got, want, what=""):
    """Asserts that got and want are NaN, +inf and -inf at the same elements; returns the mask of the finite ones."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for name, f in (("nan", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        a, b = f(got), f(want)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError("%s: %s mask differs at %d of %d elements (got %d, want %d), first %s: got %r want %r"
                                 % (what, name, len(bad), a.size, a.sum(), b.sum(), tuple(bad[0]), got[tuple(bad[0])],
                                    want[tuple(bad[0])]))
    return np.isfinite(want)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def clean_bits_equal(got, clean, region, what=""):
    """Asserts that got holds the bits of the clean launch wherever the boolean `region` (broadcast to got) is set."""
    got, clean = np.asarray(got), np.asarray(clean)
    assert got.shape == clean.shape and got.dtype == clean.dtype, what
    region = np.broadcast_to(region, got.shape)
    diff = (bits(got) != bits(clean)) & region
    if diff.any():
        bad = np.argwhere(diff)
        raise AssertionError("%s: %d of %d elements outside the footprint lost the clean launch's bits, first %s: got %r clean %r"
                             % (what, len(bad), int(region.sum()), tuple(bad[0]), got[tuple(bad[0])], clean[tuple(bad[0])]))


def close_where(got, want, mask, tol, scale, what=""):
    """|got - want| <= tol * scale on the elements of `mask`."""
    if mask.any():
        err = np.abs(got.astype(np.float64)[mask] - want[mask]).max()
        assert err <= tol * scale, (what, err, tol * scale)


# ---- max-pool ----------------------------------------------------------------------------------------------------------------
def max_pool_ref(x, ksize, strides, dy=None):
    """Item 3 of the contract, from the definition (independent of oracle.nn.max_pool3d's tap loop): per window, the first NaN
    tap in (kd, kh, kw) scan order if there is one, else the first maximum; padded cells are ignored.  Returns (y, dx or None)."""
    x = np.asarray(x, np.float64)
    N, D, H, W, C = x.shape
    k, s = tuple(ksize), tuple(strides)
    out = [-(-v // st) for v, st in zip((D, H, W), s)]
    pads = [nn.same_pads(v, kk, st)[1] for v, kk, st in zip((D, H, W), k, s)]
    y = np.empty((N, out[0], out[1], out[2], C))
    dx = np.zeros_like(x) if dy is not None else None
    for od in range(out[0]):
        d0 = od * s[0] - pads[0]
        ds = [d for d in range(d0, d0 + k[0]) if 0 <= d < D]
        for oh in range(out[1]):
            h0 = oh * s[1] - pads[1]
            hs = [h for h in range(h0, h0 + k[1]) if 0 <= h < H]
            for ow in range(out[2]):
                w0 = ow * s[2] - pads[2]
                ws = [w for w in range(w0, w0 + k[2]) if 0 <= w < W]
                win = x[:, ds][:, :, hs][:, :, :, ws].reshape(N, -1, C)          # valid taps in scan order
                nanm = np.isnan(win)
                first_nan = nanm.argmax(1)
                first_max = np.where(nanm, -np.inf, win).argmax(1)                 # argmax returns the first maximum
                pick = np.where(nanm.any(1), first_nan, first_max)
                y[:, od, oh, ow] = np.take_along_axis(win, pick[:, None, :], 1)[:, 0]
                if dy is not None:
                    taps = [(d, h, w) for d in ds for h in hs for w in ws]
                    for n in range(N):
                        for c in range(C):
                            d, h, w = taps[pick[n, c]]
                            dx[n, d, h, w, c] += dy[n, od, oh, ow, c]
    return y, dx


# ---- CBAM forward --------------------------------------------------------------------------------------------------------------
def cbam_forward_ref(x, k0, b0, k1, b1, k7):
    """utils/network.py:198-274 in float64 with propagating pools and ReLU.  Returns (cs [N,C], sp [N,D,H,W,2], ss [N,D,H,W])."""
    x = np.asarray(x, np.float64)
    N, D, H, W, C = x.shape
    f64 = lambda a: np.asarray(a, np.float64)
    k0, b0, k1, b1, k7 = f64(k0), f64(b0), f64(k1), f64(b1), f64(k7)
    xf = x.reshape(N, -1, C)
    mlp = lambda v: np.maximum(v @ k0 + b0, 0) @ k1 + b1
    cs = 1.0 / (1.0 + np.exp(-(mlp(xf.mean(1)) + mlp(xf.max(1)))))           # np.max propagates NaN
    f = x * cs[:, None, None, None, :]
    sp = np.stack([f.mean(-1), f.max(-1)], -1)
    conv = nn.conv3d_forward(sp, k7.reshape(7, 7, 7, 2, 1), (1, 1, 1))[..., 0]
    return cs, sp, 1.0 / (1.0 + np.exp(-conv))
