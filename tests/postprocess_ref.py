"""numpy replay of the smoothing / normalisation stage of P3DSession.set_postprocess, bit for bit per include/p3d_hip.h:
the radius rule, the taps, the two float32 passes (vectorised over the map, one loop over the tap distance d, every product and
sum a float32 numpy operation, hence rounded on its own), the normalisations and the byte law.  The passes take the taps as an
argument: the kernels are held to the replay with the library's own taps (libm's and numpy's exp may differ in the last place)."""
import numpy as np


def radius(sigma, radius=0):
    """RADIUS: radius > 0 as given; else cv2's rule for float images on the float32 sigma; sigma == 0: no blur."""
    if radius > 0 or sigma == 0:
        return int(radius)
    k = int(np.rint(8.0 * float(np.float32(sigma)) + 1.0)) | 1
    return k // 2


def taps(sigma, r):
    """TAPS: float32(e_k / sum e), e_k = exp(-(k - r)^2 / (2 sigma^2)) in float64 on the float32 sigma, summed in ascending k."""
    s = float(np.float32(sigma))
    d = np.arange(2 * r + 1, dtype=np.float64) - r
    e = np.exp(-(d * d) / (2.0 * (s * s)))
    S = 0.0
    for v in e:
        S += float(v)
    return (e / S).astype(np.float32)


def reflect101(j, n):
    j = np.asarray(j)
    j = np.where(j < 0, -j, j)
    return np.where(j > n - 1, 2 * (n - 1) - j, j)


def blur_pass(m, w, axis):
    """PASS along `axis` of float32 m: acc = w_r s[i]; acc += w_{r+d} (s[rho(i-d)] + s[rho(i+d)]), d = 1..r."""
    m = np.asarray(m, np.float32)
    w = np.asarray(w, np.float32)
    r = (len(w) - 1) // 2
    n = m.shape[axis]
    assert r <= n - 1
    i = np.arange(n)
    acc = w[r] * m
    for d in range(1, r + 1):
        lo = np.take(m, reflect101(i - d, n), axis=axis)
        hi = np.take(m, reflect101(i + d, n), axis=axis)
        acc = acc + w[r + d] * (lo + hi)
        assert acc.dtype == np.float32
    return acc


def blur(m, w):
    """BLUR of float32 maps [..., H, W]: the pass along x, then the pass along y; no taps: the maps as they are."""
    m = np.asarray(m, np.float32)
    if len(w) == 0:
        return m.copy()
    return blur_pass(blur_pass(m, w, -1), w, -2)


def normalise(m, norm):
    """NORM of float32 maps [n, H, W], per map, on a copy."""
    out = np.array(m, np.float32)
    if norm == "none":
        return out
    for k in range(len(out)):
        mn, mx = out[k].min(), out[k].max()
        if norm == "max":
            if mx > 0:
                out[k] = out[k] / mx
        elif norm == "range":
            out[k] = (out[k] - mn) / (mx - mn) if mx > mn else np.float32(0)
        else:
            raise ValueError(norm)
    assert out.dtype == np.float32
    return out


def sat_u8(v):
    """cv2's saturate_cast<uchar>(double): round half to even, clamp; NaN -> 0."""
    r = np.rint(np.asarray(v, np.float64))
    r = np.where(np.isnan(r), 0.0, r)
    return np.clip(r, 0.0, 255.0).astype(np.uint8)


def quantise(m, scale):
    """BYTE: sat_u8((double)fmul(v, scale))."""
    return sat_u8((np.asarray(m, np.float32) * np.float32(scale)).astype(np.float64))


def postprocess(resized, w, norm="none", scale=None):
    """The chain after the float32 resize on maps [n, H, W] -> float32, or uint8 with a scale."""
    out = normalise(blur(resized, w), norm)
    return out if scale is None else quantise(out, scale)
