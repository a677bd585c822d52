"""numpy replay of the temporal smoothing of a resident video's maps (include/p3d_hip.h, "Temporal smoothing"): the settings'
refusals, the frames a read needs, MEAN's division on load (video_ref.read_out), GAUSS in np.float32 operations in the PASS
order and the EMA recurrence.  Bit for bit what the kernels of csrc/temporal.hip must produce."""
import math

import numpy as np

import video_ref as vr

OFF, GAUSS, EMA = 0, 1, 2
MAX_RADIUS = 24
KINDS = {"off": OFF, "gauss": GAUSS, "ema": EMA}


class Refused(ValueError):
    pass


def radius_of(sigma, radius):
    """RADIUS of the postprocess section with the temporal limits; raises Refused as p3d_set_video_temporal refuses."""
    sigma = np.float32(sigma)
    if not np.isfinite(sigma) or not sigma > 0:
        raise Refused("sigma")
    if radius < 0 or radius > MAX_RADIUS:
        raise Refused("radius")
    if radius > 0:
        return int(radius)
    k = float(np.rint(8.0 * float(sigma) + 1.0))
    if k > 2.0 * MAX_RADIUS + 1.0:
        raise Refused("the radius that follows from sigma")
    r = (int(k) | 1) // 2
    if r < 1:
        raise Refused("radius 0")
    return r


def taps(sigma, r):
    """TAPS: e_k in double, summed in ascending k, w_k = float32(e_k / S); the 2r + 1 weights."""
    s = float(np.float32(sigma))
    e = [math.exp(-float((k - r) * (k - r)) / (2.0 * (s * s))) for k in range(2 * r + 1)]
    S = 0.0
    for v in e:
        S += v
    return np.array([v / S for v in e], np.float64).astype(np.float32)


def parse(kind, sigma=0., radius=0, alpha=0.):
    """dict(kind, r, w, alpha) of a setting, or None for off; raises Refused as the set call does."""
    if kind is None or kind == OFF:
        return None
    if kind == GAUSS:
        r = radius_of(sigma, radius)
        return dict(kind=GAUSS, r=r, w=taps(sigma, r), alpha=np.float32(0))
    if kind == EMA:
        a = np.float32(alpha)
        if not np.isfinite(a) or not (a >= 0 and a < 1):
            raise Refused("alpha")
        return dict(kind=EMA, r=0, w=None, alpha=a)
    raise Refused("kind")


def needed(cfg, F, first, n):
    """(lo, hi): the frames a read of first .. first + n - 1 needs; raises Refused for a range outside the video or r > F - 1."""
    if n < 1 or first < 0 or first > F - n:
        raise Refused("range")
    if cfg["kind"] == GAUSS:
        if cfg["r"] > F - 1:
            raise Refused("r > F - 1")
        return max(0, first - cfg["r"]), min(F - 1, first + n - 1 + cfg["r"])
    return 0, first + n - 1


def check(cfg, count, first, n):
    """The read-out's refusals; the message names the first needed frame with count 0."""
    lo, hi = needed(cfg, len(count), first, n)
    for f in range(lo, hi + 1):
        if count[f] < 1:
            raise Refused("frame %d" % f)
    return lo, hi


def rho(j, n):
    return -j if j < 0 else (2 * (n - 1) - j if j > n - 1 else j)


def gauss(v, w, r, first=0, n=None):
    """PASS along axis 0 of v [F, ...] float32 for frames first .. first + n - 1: every operation a float32 numpy op of its own."""
    F = len(v)
    n = F - first if n is None else n
    out = np.empty((n,) + v.shape[1:], np.float32)
    with np.errstate(all="ignore"):
        for i, f in enumerate(range(first, first + n)):
            acc = w[r] * v[f]
            for d in range(1, r + 1):
                acc = acc + w[r + d] * (v[rho(f - d, F)] + v[rho(f + d, F)])
            out[i] = acc
    return out


def ema(v, alpha, first=0, n=None):
    """m_0 = v_0 (the bits), m_f = alpha m_{f-1} + (1 - alpha) v_f in float32; frames first .. first + n - 1."""
    F = len(v)
    n = F - first if n is None else n
    a = np.float32(alpha)
    b = np.float32(1.0) - a
    out = np.empty((n,) + v.shape[1:], np.float32)
    m = v[0].copy()
    with np.errstate(all="ignore"):
        for f in range(first + n):
            if f:
                m = a * m + b * v[f]
            if f >= first:
                out[f - first].view(np.uint32)[...] = np.ascontiguousarray(m).view(np.uint32)
    return out


def inputs(mode, store, count, lo, hi):
    """v_f for every frame, [F, ...]: the stored map under NEWEST, sum / float32(count) under MEAN (a count of 1: the bits).
    Frames outside lo .. hi are not needed, may have count 0 and are returned as they are stored."""
    v = np.array(store, np.float32, copy=True)
    v[lo:hi + 1] = vr.read_out(mode, v[lo:hi + 1], [int(c) for c in count[lo:hi + 1]])
    return v


def filter_maps(cfg, mode, store, count, first=0, n=None):
    """What a read-out of frames first .. first + n - 1 returns under the setting cfg (parse): store [F, ...] float32 (maps or
    sums), count [F]."""
    store = np.ascontiguousarray(store, np.float32)
    F = len(store)
    n = F - first if n is None else n
    lo, hi = check(cfg, [int(c) for c in count], first, n)
    v = inputs(mode, store, count, lo, hi)
    if cfg["kind"] == GAUSS:
        return gauss(v, cfg["w"], cfg["r"], first, n)
    return ema(v, cfg["alpha"], first, n)
