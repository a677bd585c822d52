"""The law of include/p3d_hip.h, "QP maps of 8-bit maps", replayed in numpy (int64 throughout; the contract's sums fit 32 bits), and
the makers of its test inputs.  Nothing here is shared with the library: the block loop is written out block by block."""
import numpy as np

BLOCKS = (8, 16, 32, 64, 128)


def check_cfg(block, peak_weight, dilate, fall, rise, balance, target, lo, hi, law):
    if block not in BLOCKS:
        raise ValueError("block")
    if not 0 <= peak_weight <= 256 or not 0 <= dilate <= 8 or not 0 <= fall <= 254 or not 0 <= rise <= 254 or balance not in (0, 1):
        raise ValueError("range")
    if not -127 <= lo <= target <= hi <= 127:
        raise ValueError("lo <= target <= hi")
    law = np.asarray(law)
    if law.shape != (256,) or law.min() < -127 or law.max() > 127:
        raise ValueError("law")


def areas(H, W, B):
    """AREA [Hb, Wb]: the pixel count of every block, edge blocks partial."""
    Hb, Wb = -(-H // B), -(-W // B)
    hs = np.minimum(H, (np.arange(Hb) + 1) * B) - np.arange(Hb) * B
    ws = np.minimum(W, (np.arange(Wb) + 1) * B) - np.arange(Wb) * B
    return (hs[:, None] * ws[None, :]).astype(np.int64)


def level(s, B, peak_weight):
    """LEVEL of one map [H, W] -> L [Hb, Wb] int64, block by block."""
    H, W = s.shape
    Hb, Wb = -(-H // B), -(-W // B)
    L = np.zeros((Hb, Wb), np.int64)
    for by in range(Hb):
        for bx in range(Wb):
            blk = s[by * B:min(H, (by + 1) * B), bx * B:min(W, (bx + 1) * B)].astype(np.int64)
            total, peak, area = int(blk.sum()), int(blk.max()), blk.size
            mean = (2 * total + area) // (2 * area)
            L[by, bx] = (peak_weight * peak + (256 - peak_weight) * mean + 128) >> 8
    return L


def dilate(L, radius):
    """DILATE: the largest L within `radius` blocks either way, clipped to the grid."""
    Hb, Wb = L.shape
    out = np.empty_like(L)
    for by in range(Hb):
        for bx in range(Wb):
            out[by, bx] = L[max(0, by - radius):by + radius + 1, max(0, bx - radius):bx + radius + 1].max()
    return out


def limit(q0, fall, rise, shots=None):
    """LIMIT over the frames of the call: q0 [n, Hb, Wb] -> q1."""
    starts = {0} | (set(int(s) for s in shots) if shots is not None else set())
    q1 = np.array(q0, np.int64)
    for f in range(1, len(q1)):
        if f in starts:
            continue
        q = q1[f]
        if fall:
            q = np.maximum(q, q1[f - 1] - fall)
        if rise:
            q = np.minimum(q, q1[f - 1] + rise)
        q1[f] = q
    return q1


def floor_mean(S1, A):
    """m = floor((2 S1 + A) / (2 A)), towards minus infinity (Python's // on ints)."""
    return (2 * int(S1) + int(A)) // (2 * int(A))


def balance(q1, area, A, on, target, lo, hi):
    """BALANCE of one frame -> (q2, [min q2, max q2, S1, S2])."""
    S1 = int((area * q1).sum())
    shift = target - floor_mean(S1, A) if on else 0
    q2 = np.clip(q1 + shift, lo, hi)
    return q2, [int(q2.min()), int(q2.max()), S1, int((area * q2).sum())]


def qpmap(sal, law, block=16, peak_weight=128, dilate_r=0, fall=0, rise=0, balance_on=1, target=0, lo=-127, hi=127, shots=None):
    """sal uint8 [n, H, W], law [256] -> (qp int32 [n, Hb, Wb], levels uint8 [n, Hb, Wb], stats int32 [n, 4])."""
    sal = np.asarray(sal)
    assert sal.dtype == np.uint8 and sal.ndim == 3
    check_cfg(block, peak_weight, dilate_r, fall, rise, balance_on, target, lo, hi, law)
    n, H, W = sal.shape
    if not 1 <= n <= 65535 or H * W > 2 ** 23:
        raise ValueError("limits")
    law = np.asarray(law, np.int64)
    lev = np.stack([dilate(level(s, block, peak_weight), dilate_r) for s in sal])
    q1 = limit(law[lev], fall, rise, shots)
    area = areas(H, W, block)
    qp, stats = np.empty(lev.shape, np.int32), np.empty((n, 4), np.int32)
    for f in range(n):
        qp[f], stats[f] = balance(q1[f], area, H * W, balance_on, target, lo, hi)
    return qp, lev.astype(np.uint8), stats


def linear_law(lo=-20, hi=6):
    """A law of its own for the tests, integers only: from hi at level 0 down to lo at level 255, rounded half up."""
    v = np.arange(256, dtype=np.int64)
    return ((2 * (hi * 255 - (hi - lo) * v) + 255) // 510).astype(np.int32)


def blobs(n, H, W, seed, count=4, drift=1.7):
    """n frames of `count` Gaussian blobs that drift and breathe, over a little noise: uint8 [n, H, W]."""
    rng = np.random.RandomState(seed)
    cy, cx = rng.uniform(0, H, count), rng.uniform(0, W, count)
    vy, vx = rng.uniform(-drift, drift, count), rng.uniform(-drift, drift, count)
    sig = rng.uniform(1.0, max(1.5, min(H, W) / 5.0), count)
    amp = rng.uniform(90, 255, count)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n, H, W), np.uint8)
    for f in range(n):
        m = rng.uniform(0, 12, (H, W))
        for k in range(count):
            a = amp[k] * (0.75 + 0.25 * np.sin(0.9 * f + k))
            m = np.maximum(m, a * np.exp(-((yy - cy[k] - vy[k] * f) ** 2 + (xx - cx[k] - vx[k] * f) ** 2) / (2 * sig[k] ** 2)))
        out[f] = np.clip(np.floor(m + 0.5), 0, 255).astype(np.uint8)
    return out


def frames(n, H, W, seed, shots):
    """n frames whose content jumps at every start of `shots` (a new blob field per shot): (uint8 [n, H, W], int32 starts)."""
    starts = np.asarray(sorted(set([0] + [int(s) for s in shots])), np.int32)
    out = np.empty((n, H, W), np.uint8)
    for k, a in enumerate(starts):
        b = int(starts[k + 1]) if k + 1 < len(starts) else n
        out[a:b] = blobs(b - a, H, W, seed + 17 * k)
    return out, starts
