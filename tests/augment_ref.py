"""Bit-exact numpy replay of the clip augmentation of P3DSession.set_augment (include/p3d_hip.h, "Clip augmentation on the
device"): the transform on x [B,T,H,W,3], y [B,T,H,W] and the fixation bytes [B,T,H,W], and the host-side draws.

Per clip, one row of decisions (flip, reverse, y0, x0, ch, cw, a, b), in this order:
  1 the window [y0, y0+ch) x [x0, x0+cw) of every frame resized back to H x W: x (per channel) and y through
    oracle.dataflow.resize_linear on the slice (cv2.INTER_LINEAR in float32); the fixations through fixations_to_grid's law on
    the slice (cell (r * H // ch, c * W // cw) becomes 255 for a byte >= 128, every other cell 0).  A window equal to the frame
    copies the bits (bytes included);
  2 flip w -> W-1-w, 3 reverse t -> T-1-t, on all three;
  4 x alone: float32(float32(x * a) + b); a == 1 and b == 0 copies the bits.
Draws: SplitMix64's finaliser on seed ^ 0xA5A5A5A5A5A5A5A5 + 0x9E3779B97F4A7C15 * (1 + 8 g + j), u = (z >> 11) * 2^-53, in
Python integers and doubles on the float32-rounded settings."""
import numpy as np

from oracle.dataflow import resize_linear

f32 = np.float32
MASK = (1 << 64) - 1
NEUTRAL = dict(flip=0.0, reverse=0.0, min_scale=1.0, contrast=0.0, brightness=0.0)


def uniform(seed, g, j):
    z = (int(seed) ^ 0xA5A5A5A5A5A5A5A5) & MASK
    z = (z + 0x9E3779B97F4A7C15 * (1 + 8 * int(g) + j)) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return (z >> 11) * 2.0 ** -53


def _clamp(v, lo, hi):
    return max(lo, min(hi, v))


def draw(seed, g, H, W, flip=0.0, reverse=0.0, min_scale=1.0, contrast=0.0, brightness=0.0):
    """(flip, reverse, y0, x0, ch, cw, a, b) of clip g (global index rank * B + b); the settings as float32 holds them."""
    import math
    pf, pr, ms, ct, br = (float(f32(v)) for v in (flip, reverse, min_scale, contrast, brightness))
    s = 1.0 - uniform(seed, g, 2) * (1.0 - ms)
    ch = _clamp(int(math.floor(s * H + 0.5)), 1, H)
    cw = _clamp(int(math.floor(s * W + 0.5)), 1, W)
    y0 = int(math.floor(uniform(seed, g, 3) * (H - ch + 1)))
    x0 = int(math.floor(uniform(seed, g, 4) * (W - cw + 1)))
    a = f32(1.0 + (2.0 * uniform(seed, g, 5) - 1.0) * ct)
    b = f32((2.0 * uniform(seed, g, 6) - 1.0) * br)
    return (uniform(seed, g, 0) < pf, uniform(seed, g, 1) < pr, y0, x0, ch, cw, a, b)


def draws(seed, B, H, W, rank=0, **cfg):
    return [draw(seed, rank * B + b, H, W, **cfg) for b in range(B)]


def crop_f32(frames, y0, x0, ch, cw):
    """Step 1 on float32 frames [T,H,W] or [T,H,W,C]."""
    T, H, W = frames.shape[:3]
    if (ch, cw) == (H, W):
        return frames.copy()
    return np.stack([resize_linear(fr[y0:y0 + ch, x0:x0 + cw], H, W) for fr in frames])


def crop_fix(frames, y0, x0, ch, cw):
    """Step 1 on fixation bytes [T,H,W]: fixations_to_grid's law on the window."""
    T, H, W = frames.shape
    if (ch, cw) == (H, W):
        return frames.copy()
    out = np.zeros_like(frames)
    k, r, c = np.nonzero(frames[:, y0:y0 + ch, x0:x0 + cw] >= 128)
    out[k, r * H // ch, c * W // cw] = 255
    return out


def _flip_reverse(v, flip, reverse):
    if flip:
        v = v[:, :, ::-1]
    if reverse:
        v = v[::-1]
    return v


def clip(x, y, fix, decision):
    """One clip: x [T,H,W,3], y [T,H,W] float32, fix [T,H,W] uint8 or None -> the augmented three."""
    flip, reverse, y0, x0, ch, cw, a, b = decision
    H, W = y.shape[1:]
    assert 1 <= ch <= H and 1 <= cw <= W and 0 <= y0 <= H - ch and 0 <= x0 <= W - cw, decision
    xo = _flip_reverse(crop_f32(np.asarray(x, f32), y0, x0, ch, cw), flip, reverse)
    yo = _flip_reverse(crop_f32(np.asarray(y, f32), y0, x0, ch, cw), flip, reverse)
    fo = None if fix is None else np.ascontiguousarray(_flip_reverse(crop_fix(np.asarray(fix), y0, x0, ch, cw), flip, reverse))
    a, b = f32(a), f32(b)
    if not (a == f32(1) and b == f32(0)):
        with np.errstate(all="ignore"):
            xo = ((xo * a).astype(f32) + b).astype(f32)
    return np.ascontiguousarray(xo), np.ascontiguousarray(yo), fo


def batch(x, y, fix, decisions):
    """x [B,T,H,W,3], y [B,T,H,W], fix [B,T,H,W] uint8 or None, one decision per clip."""
    outs = [clip(x[b], y[b], None if fix is None else fix[b], decisions[b]) for b in range(len(decisions))]
    return (np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), None if fix is None else np.stack([o[2] for o in outs]))


def random_clip(seed, shape, specials=False):
    """x, y, fix of `shape` (B,T,H,W): normal deviates, uniform targets, bytes either side of 128.  specials: NaN (with a
    payload), +-inf, -0 and a denormal planted in x and y -- for the paths that copy bits; arithmetic on them is not pinned (a
    NaN an operation produces has the platform's sign and payload)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(tuple(shape) + (3,)).astype(f32)
    y = rng.random(tuple(shape)).astype(f32)
    fix = rng.choice(np.array([0, 1, 127, 128, 200, 255], np.uint8), size=tuple(shape), p=[0.7, 0.05, 0.05, 0.1, 0.05, 0.05])
    if specials:
        sp = np.array([0x7fc00000, 0xffc12345, 0x7f800000, 0xff800000, 0x80000000, 0x00000123], np.uint32).view(f32)
        for arr in (x, y):
            flat = arr.reshape(-1)
            idx = rng.choice(flat.size, size=min(flat.size, 2 * sp.size), replace=False)
            flat[idx] = np.resize(sp, idx.size)
    return x, y, fix
