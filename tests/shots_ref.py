"""numpy replay of include/p3d_hip.h's "Shot boundaries of 8-bit frames" (csrc/shots.hip) and of what a shot table does to the
temporal filter and to the reframe track, written from that text alone: the cell histograms by a bincount over explicit cell, channel
and bin indices, the decision in Python integers, the filters frame by frame.  SIGNAL, DECISION and the track are integers and compare
exactly; the temporal filter is float32 numpy operations in the PASS order and compares bit for bit."""
import numpy as np

import reframe_ref
import temporal_ref as tr

MAX_GRID = 4


# ---- SIGNAL ----
def histograms(frame, gy, gx):
    """HIST of one frame uint8 [H, W, 3] -> int64 [gy, gx, 3, 64]."""
    frame = np.asarray(frame)
    H, W, _ = frame.shape
    assert 1 <= gy <= min(MAX_GRID, H) and 1 <= gx <= min(MAX_GRID, W)
    cy = (np.arange(H, dtype=np.int64) * gy // H)[:, None, None]
    cx = (np.arange(W, dtype=np.int64) * gx // W)[None, :, None]
    ch = np.arange(3, dtype=np.int64)[None, None, :]
    idx = ((cy * gx + cx) * 3 + ch) * 64 + (frame.astype(np.int64) >> 2)
    return np.bincount(idx.ravel(), minlength=gy * gx * 192).reshape(gy, gx, 3, 64)


def distances(frames, gy, gx):
    """DIST: frames uint8 [n, H, W, 3] -> uint32 [n]."""
    frames = np.asarray(frames)
    n, H, W, _ = frames.shape
    assert 1 <= n <= 65535 and H * W <= 2 ** 28
    D = np.zeros(n, np.int64)
    prev = None
    for f in range(n):
        h = histograms(frames[f], gy, gx)
        if f:
            D[f] = np.abs(h - prev).sum()
        prev = h
    assert D.max() <= 6 * H * W
    return D.astype(np.uint32)


# ---- DECISION ----
def candidates(D, P, threshold, window, ratio):
    F = len(D)
    D = [int(d) for d in D]
    cand = [False] * F
    for f in range(1, F):
        near = [D[g] for g in range(max(1, f - window), min(F - 1, f + window) + 1) if g != f]
        N = max(near) if near else 0
        cand[f] = D[f] * 1000 >= threshold * 6 * P and D[f] * 256 >= ratio * N
    return cand


def cuts(D, P, threshold, window, ratio, min_length):
    """CAND and ACCEPT -> starts, a list that begins with 0."""
    assert 1 <= threshold <= 1000 and 0 <= window <= 32 and 256 <= ratio <= 65535 and min_length >= 1
    F = len(D)
    cand = candidates(D, P, threshold, window, ratio)
    starts, last = [0], 0
    for f in range(1, F):
        if cand[f] and f - last >= min_length and F - f >= min_length:
            starts.append(f)
            last = f
    return starts


def shot_of(starts, F, f):
    """(lo, hi) of the shot frame f lies in."""
    starts = list(starts)
    assert starts[0] == 0 and all(a < b for a, b in zip(starts, starts[1:])) and starts[-1] < F
    k = max(i for i, s in enumerate(starts) if s <= f)
    return starts[k], (starts[k + 1] if k + 1 < len(starts) else F) - 1


# ---- the temporal filter under a shot table ----
def refl(j, L):
    """Periodic reflect-101 of any integer j into 0 .. L - 1."""
    if L == 1:
        return 0
    m = j % (2 * L - 2)
    return m if m < L else 2 * L - 2 - m


def gauss_shots(v, w, r, starts, first=0, n=None):
    """GAUSS with rho replaced by rho_s(i) = lo + refl(i - lo, L) of frame f's shot; v [F, ...] float32."""
    F = len(v)
    n = F - first if n is None else n
    out = np.empty((n,) + v.shape[1:], np.float32)
    with np.errstate(all="ignore"):
        for i, f in enumerate(range(first, first + n)):
            lo, hi = shot_of(starts, F, f)
            L = hi - lo + 1
            acc = w[r] * v[f]
            for d in range(1, r + 1):
                acc = acc + w[r + d] * (v[lo + refl(f - d - lo, L)] + v[lo + refl(f + d - lo, L)])
            out[i] = acc
    return out


def ema_shots(v, alpha, starts, first=0, n=None):
    """EMA restarted at every shot: m_lo = v_lo, a copy of the bits."""
    F = len(v)
    n = F - first if n is None else n
    a = np.float32(alpha)
    b = np.float32(1.0) - a
    out = np.empty((n,) + v.shape[1:], np.float32)
    begins = set(int(s) for s in starts)
    m = None
    with np.errstate(all="ignore"):
        for f in range(first + n):
            m = v[f].copy() if f in begins else a * m + b * v[f]
            if f >= first:
                out[f - first].view(np.uint32)[...] = np.ascontiguousarray(m).view(np.uint32)
    return out


def temporal_shots(cfg, v, starts, first=0, n=None):
    """cfg: temporal_ref.parse's; v [F, ...] float32 inputs (every count 1)."""
    v = np.ascontiguousarray(v, np.float32)
    if cfg["kind"] == tr.GAUSS:
        return gauss_shots(v, cfg["w"], cfg["r"], starts, first, n)
    return ema_shots(v, cfg["alpha"], starts, first, n)


# ---- the reframe track under a shot table ----
def smooth_shots(raw, R, starts):
    """SMOOTHED TRACK with c(i) = min(max(i, a), b), [a, b] the frame's shot inside the n frames given."""
    n = len(raw)
    if R == 0:
        return [tuple(int(c) for c in p) for p in raw]
    out = []
    for f in range(n):
        a, b = shot_of(starts, n, f)
        sy = sx = 0
        for k in range(-R, R + 1):
            c = min(max(f + k, a), b)
            sy += int(raw[c][0])
            sx += int(raw[c][1])
        out.append(((2 * sy + (2 * R + 1)) // (2 * (2 * R + 1)), (2 * sx + (2 * R + 1)) // (2 * (2 * R + 1))))
    return out


def reframe_shots(sal, frames, hc, wc, gate, R, starts):
    """reframe_ref.reframe with the track smoothed inside the shots: (track, raw, mass, crop or None)."""
    sal = np.asarray(sal)
    n, H, W = sal.shape
    _, raw, mass, _ = reframe_ref.reframe(sal, None, hc, wc, gate, 0)
    track = np.array(smooth_shots(raw, R, starts), np.int32).reshape(n, 2)
    mass = mass.copy()
    for f, (y, x) in enumerate(track):
        mass[f, 1] = reframe_ref.weights(sal[f, y:y + hc, x:x + wc], gate).sum()
    crop = None
    if frames is not None:
        crop = np.stack([np.asarray(frames)[f, y:y + hc, x:x + wc] for f, (y, x) in enumerate(track)])
    return track, raw, mass, crop


# ---- the inputs of the tests ----
FIXTURE_LENGTHS = (5, 16, 9, 3, 7)
FIXTURE_CUTS = [5, 21, 30, 33]
FIXTURE_RULE = dict(threshold=250, window=2, ratio=512, min_length=3)


def shot_frames(length, seed, H=24, W=40, cell=4):
    """One shot: a random (H / cell) x (W / cell) grid of colours blown up cell x cell, with noise in -2 .. 2 on every frame."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H // cell, W // cell, 3)).astype(np.int64)
    base = np.kron(base, np.ones((cell, cell, 1), np.int64))
    noise = rng.integers(-2, 3, (length, H, W, 3))
    return np.clip(base[None] + noise, 0, 255).astype(np.uint8)


def fixture(lengths=FIXTURE_LENGTHS, H=24, W=40):
    """The planted video: shots of the given lengths, shot k from default_rng(k)."""
    return np.concatenate([shot_frames(n, k, H, W) for k, n in enumerate(lengths)])


def noise_frames(n, H, W, seed=0):
    return np.random.default_rng([seed, n, H, W]).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
