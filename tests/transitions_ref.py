"""numpy replay of include/p3d_hip.h's "Gradual transitions" (csrc/shots.hip), written from that text alone: the three signals of a
frame from shots_ref's cell histograms, the spread in Python integers (with the header's q, r split beside it, for the test of that
identity), the decision in Python integers.  Everything is an integer and compares exactly.  The planted video at the end is built
in integers only."""
import numpy as np

import shots_ref

FIRST, CUT, FADE, DISSOLVE = 0, 1, 2, 3
GRADUAL_DEFAULTS = dict(lag=12, high=250, dip=230, mono=768, mono_min=2)


# ---- SIGNAL ----
def spread_exact(h, P):
    """v of one frame's histograms int [gy, gx, 3, 64], the law as written: S1 * S1 is formed, in Python integers."""
    v = 0
    for c in range(3):
        n = [int(x) for x in np.asarray(h)[:, :, c, :].sum(axis=(0, 1))]
        S1 = sum(b * n[b] for b in range(64))
        S2 = sum(b * b * n[b] for b in range(64))
        v += S2 - S1 * S1 // P
    return v


def square_over(S1, P):
    """floor(S1^2 / P) the way the device forms it: q = S1 / P, r = S1 - q P, no term above 64 bits."""
    q = S1 // P
    r = S1 - q * P
    terms = (q * q * P, 2 * q * r, r * r // P)
    assert all(0 <= t < 2 ** 64 for t in terms) and r * r < 2 ** 64
    return sum(terms)


def signals(frames, gy, gx, lag):
    """frames uint8 [n, H, W, 3] -> D uint32 [n], E uint32 [n], v int64 [n]; lag 0 (E = 0 everywhere) or 2 .. 64."""
    frames = np.asarray(frames)
    n, H, W, _ = frames.shape
    P = H * W
    assert 1 <= n <= 65535 and P <= 2 ** 28 and (lag == 0 or 2 <= lag <= 64)
    hs = [shots_ref.histograms(frames[f], gy, gx) for f in range(n)]
    D, E, v = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for f in range(n):
        if f >= 1:
            D[f] = np.abs(hs[f] - hs[f - 1]).sum()
        if lag and f >= lag:
            E[f] = np.abs(hs[f] - hs[f - lag]).sum()
        v[f] = spread_exact(hs[f], P)
    assert max(D.max(), E.max()) <= 6 * P and 0 <= v.min() and v.max() < 2 ** 40
    return D.astype(np.uint32), E.astype(np.uint32), v


# ---- DECISION ----
def runs(flags):
    """The maximal runs [a, b] of true flags."""
    out, a = [], None
    for f, on in enumerate(list(flags) + [False]):
        if on and a is None:
            a = f
        if not on and a is not None:
            out.append((a, f - 1))
            a = None
    return out


def flags(D, E, v, P, rule, gradual):
    """CAND, MONO, HIGH, FADE, DISS, each a list of F booleans."""
    K, high, dip, mono, mono_min = (gradual[k] for k in ("lag", "high", "dip", "mono", "mono_min"))
    assert (K == 0 or 2 <= K <= 64) and 1 <= high <= 1000 and 1 <= dip <= 256 and 0 <= mono <= 65535 and mono_min >= 0
    F = len(D)
    E, v = [int(e) for e in E], [int(x) for x in v]
    cand = shots_ref.candidates(D, P, rule["threshold"], rule["window"], rule["ratio"])
    is_mono = [v[f] * 256 <= mono * P for f in range(F)]
    is_high = [K > 0 and f >= K and E[f] * 1000 >= high * 6 * P for f in range(F)]
    fade, diss = [False] * F, [False] * F
    if mono_min:
        for a, b in runs(is_mono):
            if b - a + 1 >= mono_min and a >= 1 and b <= F - 2:
                fade[b + 1] = True
    for p, q in runs(is_high):
        n = q - p + 1
        if not (2 * n >= K and n <= 2 * K):
            continue
        if any(cand[g] for g in range(max(1, p - K + 1), q + 1)):
            continue
        if any(is_mono[g] for g in range(max(0, p - K), q + 1)):
            continue
        lo = max(p - K, 0)
        if min(v[lo:q + 1]) * 256 <= dip * min(v[lo], v[q]):
            diss[(p + q - K + 1) >> 1] = True
    return cand, is_mono, is_high, fade, diss


def transitions(D, E, v, P, rule, gradual):
    """KIND and ACCEPT -> (starts, kinds), lists that begin with 0 and FIRST."""
    assert rule["min_length"] >= 1
    F = len(D)
    cand, _, _, fade, diss = flags(D, E, v, P, rule, gradual)
    starts, kinds, last = [0], [FIRST], 0
    for f in range(1, F):
        kind = CUT if cand[f] else FADE if fade[f] else DISSOLVE if diss[f] else None
        if kind is not None and f - last >= rule["min_length"] and F - f >= rule["min_length"]:
            starts.append(f)
            kinds.append(kind)
            last = f
    return starts, kinds


# ---- the planted video ----
FIXTURE_FRAMES = 241
FIXTURE_GRID = (4, 4)
FIXTURE_RULE = shots_ref.FIXTURE_RULE
FIXTURE_STARTS = [0, 24, 48, 77, 126, 188]
FIXTURE_KINDS = [FIRST, DISSOLVE, CUT, FADE, DISSOLVE, CUT]
FIXTURE_OFF_STARTS = [0, 48, 188]


def scene(seed, H, W, shift=0):
    """int64 [H, W, 3]: per channel the mean of two triangle waves |(a y +- b x + phi) mod 510 - 255|; shift moves it along x."""
    rng = np.random.default_rng(seed)
    y = np.arange(H, dtype=np.int64)[:, None]
    x = np.arange(W, dtype=np.int64)[None, :] + shift
    out = np.empty((H, W, 3), np.int64)
    for c in range(3):
        a, b, p0, p1 = (int(k) for k in rng.integers((20, 20, 0, 0), (90, 90, 510, 510)))
        out[:, :, c] = (np.abs((a * y + b * x + p0) % 510 - 255) + np.abs((a * y - b * x + p1) % 510 - 255)) // 2
    return out


def fixture(H=24, W=40):
    """The planted video uint8 [241, H, W, 3]: scenes of 20 frames joined by a dissolve of 8, a hard cut, a fade through 3 black
    frames, a flash, a dissolve of 4, a dissolve of 20, and a hard cut to a scene that pans for 13 frames."""
    noise = np.random.default_rng(1000)
    black = np.zeros((H, W, 3), np.int64)
    frames = []

    def put(img):
        frames.append(np.clip(img + noise.integers(-1, 2, (H, W, 3)), 0, 255).astype(np.uint8))

    def still(img, n=20):
        for _ in range(n):
            put(img)

    def blend(A, B, L):
        for i in range(1, L + 1):
            put(((L + 1 - i) * A + i * B + (L + 1) // 2) // (L + 1))

    s = [scene(k, H, W) for k in range(8)]
    still(s[0]); blend(s[0], s[1], 8); still(s[1])                       # dissolve over frames 20 .. 27
    still(s[2])                                                         # hard cut at 48
    blend(s[2], black, 6); still(black, 3); blend(black, s[3], 6)        # black at 74 .. 76
    still(s[3])
    put(np.full((H, W, 3), 250, np.int64))                              # the flash, frame 103
    still(s[3]); blend(s[3], s[4], 4); still(s[4])                       # dissolve over 124 .. 127
    blend(s[4], s[5], 20); still(s[5])                                   # dissolve over 148 .. 167: too long for K = 12
    still(s[6])                                                         # hard cut at 188
    for t in range(1, 14):
        put(scene(6, H, W, 3 * t))                                      # the pan, frames 208 .. 220
    still(scene(6, H, W, 39))
    out = np.stack(frames)
    assert out.shape == (FIXTURE_FRAMES, H, W, 3)
    return out
