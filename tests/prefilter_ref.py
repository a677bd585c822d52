"""The law of include/p3d_hip.h, "Pre-filtering frames by their 8-bit maps", replayed in numpy (int64 throughout), and the makers of
its test inputs.  The strength grid is, by the contract's own definition, the QP maps' qp, so it comes from qpmap_ref; the pixel
weight, the low-pass and the blend are written out here on their own, and nothing is shared with the library."""
import numpy as np

import qpmap_ref as qr

BLOCKS = qr.BLOCKS


def check_cfg(block, peak_weight, dilate, fall, rise, radius, passes, law):
    if block not in BLOCKS:
        raise ValueError("block")
    if not 0 <= peak_weight <= 256 or not 0 <= dilate <= 8 or not 0 <= fall <= 64 or not 0 <= rise <= 64:
        raise ValueError("range")
    if not 1 <= radius <= 16 or not 1 <= passes <= 3:
        raise ValueError("radius, passes")
    law = np.asarray(law)
    if law.shape != (256,) or law.min() < 0 or law.max() > 64:
        raise ValueError("law")


def grid(sal, law, block=16, peak_weight=128, dilate=0, fall=0, rise=0, shots=None):
    """STRENGTH GRID: g int64 [n, Hb, Wb], the QP maps' qp with balance = 0, target = 0, lo = 0, hi = 64."""
    return qr.qpmap(sal, law, block, peak_weight, dilate, fall, rise, 0, 0, 0, 64, shots)[0].astype(np.int64)


def axis_terms(size, cells, B):
    """Per pixel of one axis: (the clamped index below, the clamped index above, the fraction f in 0 .. D - 1)."""
    D = 2 * B
    u = 2 * np.arange(size, dtype=np.int64) + 1 - B
    j0 = u // D                                            # numpy's // on integers rounds towards minus infinity
    f = u - D * j0
    return np.clip(j0, 0, cells - 1), np.clip(j0 + 1, 0, cells - 1), f


def weight(g, H, W, B):
    """PIXEL WEIGHT of one frame: g [Hb, Wb] -> Wn int64 [H, W], in 0 .. Q = 64 (2 B)^2."""
    g = np.asarray(g, np.int64)
    D = 2 * B
    ja, jb, fy = axis_terms(H, g.shape[0], B)
    ia, ib, fx = axis_terms(W, g.shape[1], B)
    fy, fx = fy[:, None], fx[None, :]
    return ((D - fy) * (D - fx) * g[ja][:, ia] + (D - fy) * fx * g[ja][:, ib] + fy * (D - fx) * g[jb][:, ia] + fy * fx * g[jb][:, ib])


def box_pass(l, R):
    """One pass of LOW-PASS on one frame [H, W, 3] (int64): the clamped (2 R + 1)^2 sum, rounded once."""
    H, W, _ = l.shape
    A = (2 * R + 1) ** 2
    ys = np.clip(np.arange(-R, H + R), 0, H - 1)
    xs = np.clip(np.arange(-R, W + R), 0, W - 1)
    p = l[ys][:, xs]                                       # the frame with its replicated border
    total = np.zeros_like(l)
    for dy in range(2 * R + 1):
        for dx in range(2 * R + 1):
            total += p[dy:dy + H, dx:dx + W]
    return (2 * total + A) // (2 * A)


def low_pass(frame, R, P):
    l = np.asarray(frame, np.int64)
    for _ in range(P):
        l = box_pass(l, R)
    return l


def blend(frame, low, Wn, B):
    """BLEND of one frame -> (out int64 [H, W, 3], the largest numerator)."""
    lq = 8 + 2 * (int(B).bit_length() - 1)
    Q = 1 << lq
    num = np.asarray(frame, np.int64) * (Q - Wn[:, :, None]) + low * Wn[:, :, None] + Q // 2
    return num >> lq, int(num.max())


def prefilter(sal, frames, law, block=16, peak_weight=128, dilate=0, fall=0, rise=0, radius=4, passes=1, shots=None):
    """sal uint8 [n, H, W], frames uint8 [n, H, W, 3], law [256] -> (out uint8 [n, H, W, 3], grid int32 [n, Hb, Wb], Wn int64 [n, H, W])."""
    sal, frames = np.asarray(sal), np.asarray(frames)
    assert sal.dtype == np.uint8 and sal.ndim == 3 and frames.dtype == np.uint8 and frames.shape == sal.shape + (3,)
    check_cfg(block, peak_weight, dilate, fall, rise, radius, passes, law)
    n, H, W = sal.shape
    if not 1 <= n <= 65535 or H * W > 2 ** 23:
        raise ValueError("limits")
    g = grid(sal, law, block, peak_weight, dilate, fall, rise, shots)
    out, wn = np.empty(frames.shape, np.uint8), np.empty(sal.shape, np.int64)
    for f in range(n):
        wn[f] = weight(g[f], H, W, block)
        o, top = blend(frames[f], low_pass(frames[f], radius, passes), wn[f], block)
        assert top < 2 ** 31 and o.min() >= 0 and o.max() <= 255
        out[f] = o
    return out, g.astype(np.int32), wn


def falling_law(gate=200, full=40, strength=64):
    """A law of its own for the tests, integers only: `strength` up to level `full`, 0 from level `gate` on, linear between, rounded
    half up."""
    v = np.arange(256, dtype=np.int64)
    t = np.clip(gate - v, 0, gate - full)
    return ((2 * strength * t + (gate - full)) // (2 * (gate - full))).astype(np.int32)


def random_frames(n, H, W, seed):
    """Random bytes: every off-by-one of a window shows.  uint8 [n, H, W, 3]."""
    return np.random.RandomState(seed).randint(0, 256, (n, H, W, 3)).astype(np.uint8)
