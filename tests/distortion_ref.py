"""The law of include/p3d_hip.h, "Distortion of frames under their 8-bit maps", replayed in numpy (int64 throughout; every bound of
the contract keeps the sums inside it), and the makers of its test inputs.  The SSIM windows are plain slices of the Y planes, not the
cells the kernel sums; nothing is shared with the library."""
import numpy as np

BLOCKS = (0, 8, 16, 32, 64, 128)
RECORD = 20
SSE, WSSE, SW, MAXABS, CHANGED, SALIENT, CHANGED_SALIENT, NW, SQ, SWQ, SWW = 0, 4, 8, 9, 13, 14, 15, 16, 17, 18, 19
C1, C2 = 26634, 235963
assert C1 == round(4096 * 6.5025) and C2 == round(64 * 63 * 58.5225)


def check(sal, ref, test, block, gate, wlaw, n=None, H=None, W=None):
    """LIMITS, CONFIG and the law's range; test is required."""
    if test is None or ref is None:
        raise ValueError("null")
    n, H, W = (sal.shape[0] if n is None else n), (sal.shape[1] if H is None else H), (sal.shape[2] if W is None else W)
    if not 1 <= n <= 65535 or H < 1 or W < 1 or H * W > 2 ** 23:
        raise ValueError("limits")
    if block not in BLOCKS or not 0 <= gate <= 255:
        raise ValueError("config")
    wlaw = np.asarray(wlaw)
    if wlaw.shape != (256,) or wlaw.min() < 0 or wlaw.max() > 255:
        raise ValueError("law")


def luma(f):
    """Y of frames [..., 3] in B, G, R order -> int64 [...]."""
    f = np.asarray(f, np.int64)
    return (29 * f[..., 0] + 150 * f[..., 1] + 77 * f[..., 2] + 128) >> 8


def windows(H, W):
    """The top-left corners' rows and columns."""
    if H < 8 or W < 8:
        return [], []
    return list(range(0, H - 7, 4)), list(range(0, W - 7, 4))


def window_q(a, b):
    """q of one window: a and b are the 8 x 8 Y values (int64) of ref and test -> (q, num, den)."""
    assert a.shape == (8, 8) and b.shape == (8, 8)
    sa, sb = int(a.sum()), int(b.sum())
    saa, sbb, sab = int((a * a).sum()), int((b * b).sum()), int((a * b).sum())
    num = (2 * sa * sb + C1) * (2 * (64 * sab - sa * sb) + C2)
    den = (sa * sa + sb * sb + C1) * (64 * (saa + sbb) - sa * sa - sb * sb + C2)
    assert den > 0 and abs(num) < 2 ** 56 and den < 2 ** 56
    # float() of a Python integer is correctly rounded, and so is the division; * 65536 is exact
    q = int(np.floor(np.float64(float(num)) / np.float64(float(den)) * 65536.0 + 0.5))
    assert -65536 <= q <= 65536
    return q, num, den


def ssim_frame(ya, yb, w):
    """One frame: Y planes of ref and test and the weights, int64 [H, W] -> (NW, SQ, SWQ, SWW, q int64 [rows, cols])."""
    H, W = ya.shape
    rows, cols = windows(H, W)
    q = np.zeros((len(rows), len(cols)), np.int64)
    sq = swq = sww = 0
    for j, y in enumerate(rows):
        for i, x in enumerate(cols):
            q[j, i], _, _ = window_q(ya[y:y + 8, x:x + 8], yb[y:y + 8, x:x + 8])
            ww = int(w[y:y + 8, x:x + 8].sum())
            sq += int(q[j, i]); swq += ww * int(q[j, i]); sww += ww
    return len(rows) * len(cols), sq, swq, sww, q


def block_map(d2, B):
    """One frame: d2 int64 [H, W], the three planes' squared differences summed -> int64 [Hb, Wb], edge blocks partial."""
    H, W = d2.shape
    Hb, Wb = -(-H // B), -(-W // B)
    pad = np.zeros((Hb * B, Wb * B), np.int64)
    pad[:H, :W] = d2
    return pad.reshape(Hb, B, Wb, B).sum(axis=(1, 3))


def distortion(sal, ref, test, wlaw, block=0, gate=0, with_q=False):
    """sal uint8 [n, H, W], ref and test uint8 [n, H, W, 3], wlaw [256] -> (table int64 [n, RECORD], block_sse int64 [n, Hb, Wb] or
    None[, the list of every frame's q])."""
    check(sal, ref, test, block, gate, wlaw)
    sal, ref, test = np.asarray(sal), np.asarray(ref), np.asarray(test)
    assert sal.dtype == np.uint8 and sal.ndim == 3 and ref.dtype == np.uint8 and test.dtype == np.uint8
    assert ref.shape == sal.shape + (3,) and test.shape == ref.shape
    n, H, W = sal.shape
    law = np.asarray(wlaw, np.int64)
    table = np.zeros((n, RECORD), np.int64)
    blocks = np.zeros((n, -(-H // block), -(-W // block)), np.int64) if block else None
    qs = []
    for f in range(n):
        w = law[sal[f]]
        r, t = ref[f].astype(np.int64), test[f].astype(np.int64)
        ya, yb = luma(r), luma(t)
        d = np.concatenate([r - t, (ya - yb)[..., None]], axis=2)      # [H, W, 4]
        d2 = d * d
        table[f, SSE:SSE + 4] = d2.sum(axis=(0, 1))
        table[f, WSSE:WSSE + 4] = (d2 * w[..., None]).sum(axis=(0, 1))
        table[f, SW] = w.sum()
        table[f, MAXABS:MAXABS + 4] = np.abs(d).max(axis=(0, 1))
        changed = (r != t).any(axis=2)
        salient = (sal[f] >= gate) if gate else np.zeros((H, W), bool)
        table[f, CHANGED], table[f, SALIENT], table[f, CHANGED_SALIENT] = changed.sum(), salient.sum(), (changed & salient).sum()
        table[f, NW], table[f, SQ], table[f, SWQ], table[f, SWW], q = ssim_frame(ya, yb, w)
        qs.append(q)
        if block:
            blocks[f] = block_map(d2[..., :3].sum(axis=2), block)
    assert table[:, WSSE:WSSE + 4].max() < 2 ** 47 and abs(table[:, SWQ]).max() < 2 ** 49
    return (table, blocks, qs) if with_q else (table, blocks)


def identity_law():
    return np.arange(256, dtype=np.int32)


def random_frames(n, H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, H, W, 3)).astype(np.uint8)


def random_maps(n, H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, H, W)).astype(np.uint8)


def near(ref, seed, spread=6, share=0.5):
    """A test frame near ref: `share` of the bytes moved by up to +-spread, clipped: differences small enough for SSIM to be high and
    large enough for every sum to be busy."""
    rng = np.random.RandomState(seed)
    step = rng.randint(-spread, spread + 1, ref.shape) * (rng.rand(*ref.shape) < share)
    return np.clip(ref.astype(np.int64) + step, 0, 255).astype(np.uint8)
