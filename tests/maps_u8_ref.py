"""float64 restatement of gen_pred.py:154-168's write-out, for the tests of the 8-bit prediction maps (test infrastructure):

    save_image = np.zeros([112, 112]); save_image[:, :] = map * 255.       # float32 product, widened exactly to float64
    save_image = cv2.resize(save_image, dsize=(W, H))                        # INTER_LINEAR on CV_64F
    cv2.imwrite(name, save_image)                                            # converts to CV_8U: saturate_cast<uchar>(double)

OpenCV's CV_64F generic path (resize.cpp: HResizeLinear / VResizeLinear with float32 weights widened to double): the index
and weight tables of the float32 path (oracle/dataflow.py::_coef), horizontal pass then vertical pass, every product and sum
rounded on its own; dsize == ssize is a copy.  saturate_cast<uchar>(double) = cvRound (round half to even) then a clamp to
[0, 255]; NaN and a rounded value outside int32 give 0 (x86: cvtsd2si's integer-indefinite result saturates to 0)."""
import numpy as np

from oracle.dataflow import _coef


def quantise(v):
    """saturate_cast<uchar>(double) of an array of doubles."""
    v = np.asarray(v, dtype=np.float64)
    r = np.rint(v)                                            # round half to even
    with np.errstate(invalid="ignore"):
        inside = (r >= -2.0 ** 31) & (r <= 2.0 ** 31 - 1)     # False for NaN and +-inf
        out = np.where(inside, np.clip(np.where(inside, r, 0.0), 0, 255), 0.0)
    return out.astype(np.uint8)


def resize_f64(src, H, W):
    """cv2.resize(src, (W, H), INTER_LINEAR) of one float64 map [h, w] (values already float64)."""
    src = np.asarray(src, dtype=np.float64)
    h, w = src.shape
    if (h, w) == (H, W):
        return src.copy()
    x0, x1, wx = _coef(W, w)
    y0, y1, wy = _coef(H, h)
    one = np.float32(1)
    ax, bx = (one - wx).astype(np.float64), wx.astype(np.float64)           # float32 weights, widened
    ay, by = (one - wy).astype(np.float64)[:, None], wy.astype(np.float64)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        rows = src[:, x0] * ax[None, :] + src[:, x1] * bx[None, :]
        return rows[y0] * ay + rows[y1] * by


def maps_u8(maps, H, W, scale=255.):
    """[n, h, w] (or [h, w]) float32 -> [n, H, W] (or [H, W]) uint8, the bytes cv2.imwrite would encode."""
    m = np.asarray(maps, dtype=np.float32)
    single = m.ndim == 2
    if single:
        m = m[None]
    with np.errstate(invalid="ignore", over="ignore"):
        src = (m * np.float32(scale)).astype(np.float32).astype(np.float64)
    out = np.stack([quantise(resize_f64(k, H, W)) for k in src])
    return out[0] if single else out
