"""numpy replay of include/p3d_hip.h's "Reframing around 8-bit maps" (p3d_reframe_u8, p3d_video_reframe; csrc/reframe.hip), written
from that text alone and independent of the product's dataflow helpers: the masses of all windows by brute force (one shifted slice
of the weights per pixel of the window, summed), the best window by an explicit sort under the tie law, the box-smoothed track in
Python integers.  Everything is integer arithmetic; every comparison against it is exact."""
import numpy as np


def weights(s, gate):
    """WEIGHT: wt(v) = v where v >= gate, else 0 -> int64."""
    s = np.asarray(s).astype(np.int64)
    return np.where(s >= gate, s, 0)


def masses(s, hc, wc, gate):
    """MASS: M [H - hc + 1, W - wc + 1] of one map [H, W], every window summed pixel by pixel, and T."""
    w = weights(s, gate)
    H, W = w.shape
    Hp, Wp = H - hc + 1, W - wc + 1
    M = np.zeros((Hp, Wp), np.int64)
    if hc * wc <= Hp * Wp:
        for dy in range(hc):
            for dx in range(wc):
                M += w[dy:dy + Hp, dx:dx + Wp]
    else:                                                  # fewer windows than pixels a window: one sum per window
        for y0 in range(Hp):
            for x0 in range(Wp):
                M[y0, x0] = w[y0:y0 + hc, x0:x0 + wc].sum()
    return M, int(w.sum())


def best_window(M, H, W, hc, wc):
    """BEST WINDOW: the largest M; among equals the smallest D; among those the smallest y0, then x0."""
    top = M.max()
    ys, xs = np.nonzero(M == top)
    cands = sorted((abs(2 * int(y) - (H - hc)) + abs(2 * int(x) - (W - wc)), int(y), int(x)) for y, x in zip(ys, xs))
    return cands[0][1], cands[0][2]


def smooth(raw, R):
    """SMOOTHED TRACK of raw [(y, x)] over the n frames given, in Python integers."""
    n = len(raw)
    if R == 0:
        return [tuple(p) for p in raw]
    out = []
    for f in range(n):
        sy = sx = 0
        for k in range(-R, R + 1):
            c = min(max(f + k, 0), n - 1)
            sy += int(raw[c][0])
            sx += int(raw[c][1])
        out.append(((2 * sy + (2 * R + 1)) // (2 * (2 * R + 1)), (2 * sx + (2 * R + 1)) // (2 * (2 * R + 1))))
    return out


def reframe(sal, frames, hc, wc, gate=0, R=0):
    """sal uint8 [n, H, W], frames uint8 [n, H, W, 3] or None -> (track int32 [n, 2], raw int32 [n, 2], mass uint32 [n, 3],
    crop uint8 [n, hc, wc, 3] or None)."""
    sal = np.asarray(sal)
    n, H, W = sal.shape
    assert 1 <= hc <= H and 1 <= wc <= W and 0 <= gate <= 255 and 0 <= R <= 255
    Ms, raw, mass = [], [], np.zeros((n, 3), np.int64)
    for f in range(n):
        M, T = masses(sal[f], hc, wc, gate)
        y0, x0 = best_window(M, H, W, hc, wc)
        Ms.append(M)
        raw.append((y0, x0))
        mass[f, 0], mass[f, 2] = M[y0, x0], T
    track = smooth(raw, R)
    for f, (y, x) in enumerate(track):
        mass[f, 1] = Ms[f][y, x]
    crop = None
    if frames is not None:
        fr = np.asarray(frames)
        crop = np.empty((n, hc, wc, 3), np.uint8)
        for f, (y, x) in enumerate(track):
            for yy in range(hc):
                crop[f, yy] = fr[f, y + yy, x:x + wc]
    assert (mass >= 0).all() and mass.max() < 2 ** 32
    return np.array(track, np.int32).reshape(n, 2), np.array(raw, np.int32).reshape(n, 2), mass.astype(np.uint32), crop


def aspect_window(H, W, a, b):
    """The driver's rule for --reframe-aspect a:b (width : height): the largest window of that aspect that fits H x W -- the full
    width where W / a <= H / b, else the full height, the other side floor of the exact ratio -- each side then rounded down to an
    even number (a side of one pixel stays one)."""
    if W * b <= H * a:
        hc, wc = W * b // a, W
    else:
        hc, wc = H, H * a // b
    return max(hc // 2 * 2, 1), max(wc // 2 * 2, 1)


# ---- the inputs of the GPU tests ----
def blobs(n, H, W, seed=0):
    """A bright blob that wanders from frame to frame, on noise: the raw track moves."""
    rng = np.random.default_rng([seed, n, H, W])
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n, H, W), np.uint8)
    for i in range(n):
        cy, cx = rng.uniform(0.05, 0.95) * (H - 1), rng.uniform(0.05, 0.95) * (W - 1)
        sy, sx = max(H * 0.2, 0.8), max(W * 0.2, 0.8)
        g = 235. * np.exp(-0.5 * (((yy - cy) / sy) ** 2 + ((xx - cx) / sx) ** 2)) + rng.normal(0., 14., (H, W))
        out[i] = np.clip(np.rint(g), 0, 255).astype(np.uint8)
    return out


def frames_for(sal, seed=1):
    return np.random.default_rng([seed] + list(sal.shape)).integers(0, 256, sal.shape + (3,), dtype=np.uint8)
