"""Frame pre-processing of the reference's loader (dataflow.py:187-216 `mapf`, gen_pred.py:117-121) on the GPU:
decoded uint8 frames in, float32 clip tensors out, one fused pass (channel flip, mean subtraction, cv2.INTER_LINEAR
resize, / 255) in csrc/metrics.hip.  Decoding (cv2.imread) and the tensorpack plumbing stay with the caller."""
import ctypes as C

import numpy as np

from ._lib import check, lib

# dataflow.py:194-196: mean_value = [98, 102, 90][::-1] -> per RGB channel
MEAN_RGB = (90.0, 102.0, 98.0)


def mapf_frames(frames_bgr, size=112, mean_rgb=MEAN_RGB, device=0):
    """[n, H0, W0, 3] uint8 BGR (what cv2.imread returns) -> [n, size, size, 3] float32, one clip of the x placeholder."""
    f = np.ascontiguousarray(frames_bgr, dtype=np.uint8)
    if f.ndim == 3:
        f = f[None]
    if f.ndim != 4 or f.shape[3] != 3 or f.size == 0:
        raise ValueError("expected [n, H, W, 3] uint8 frames")
    H, W = (size, size) if np.isscalar(size) else size
    out = np.empty((f.shape[0], H, W, 3), np.float32)
    mean = (C.c_float * 3)(*[float(v) for v in mean_rgb])
    check(lib().p3d_mapf_frames(device, f.ctypes.data_as(C.POINTER(C.c_ubyte)), f.shape[0], f.shape[1], f.shape[2], mean, H, W,
                                out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def mapf_density(maps_grey, size=112, device=0):
    """[n, H0, W0] uint8 density maps (cv2.IMREAD_GRAYSCALE) -> [n, size, size] float32 in [0, 1], the y placeholder."""
    f = np.ascontiguousarray(maps_grey, dtype=np.uint8)
    if f.ndim == 2:
        f = f[None]
    if f.ndim != 3 or f.size == 0:
        raise ValueError("expected [n, H, W] uint8 maps")
    H, W = (size, size) if np.isscalar(size) else size
    out = np.empty((f.shape[0], H, W), np.float32)
    check(lib().p3d_mapf_density(device, f.ctypes.data_as(C.POINTER(C.c_ubyte)), f.shape[0], f.shape[1], f.shape[2], H, W,
                                 out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def resize_linear(maps, size, device=0):
    """cv2.resize(m, (W, H), interpolation=cv2.INTER_LINEAR) of float32 single-channel maps (test.py:170 resizes every
    112x112 prediction to the 1080x960 fixation map): [n, h, w] or [h, w] -> [n, H, W] / [H, W]; size = (H, W) or an int."""
    m = np.ascontiguousarray(maps, dtype=np.float32)
    single = m.ndim == 2
    if single:
        m = m[None]
    if m.ndim != 3 or m.size == 0:
        raise ValueError("expected [n, h, w] or [h, w] float32 maps")
    H, W = (size, size) if np.isscalar(size) else size
    out = np.empty((m.shape[0], H, W), np.float32)
    check(lib().p3d_resize_linear(device, m.ctypes.data_as(C.POINTER(C.c_float)), m.shape[0], m.shape[1], m.shape[2], H, W,
                                  out.ctypes.data_as(C.POINTER(C.c_float))))
    return out[0] if single else out


def resize_linear_u8(maps, size, scale=255., device=0):
    """gen_pred.py:154-168's write-out of float32 maps: uint8(cv2.resize(float64(m * scale), (W, H))) as cv2.imwrite stores it
    (INTER_LINEAR in float64, round half to even, clamp to [0, 255]; NaN and values outside int32 -> 0), csrc/metrics_full.hip.
    [n, h, w] or [h, w] -> [n, H, W] / [H, W] uint8; size = (H, W) or an int; m * scale is a float32 product."""
    m = np.ascontiguousarray(maps, dtype=np.float32)
    single = m.ndim == 2
    if single:
        m = m[None]
    if m.ndim != 3 or m.size == 0:
        raise ValueError("expected [n, h, w] or [h, w] float32 maps")
    H, W = (size, size) if np.isscalar(size) else size
    out = np.empty((m.shape[0], H, W), np.uint8)
    check(lib().p3d_resize_linear_u8(device, m.ctypes.data_as(C.POINTER(C.c_float)), m.shape[0], m.shape[1], m.shape[2], float(scale),
                                     H, W, out.ctypes.data_as(C.POINTER(C.c_ubyte))))
    return out[0] if single else out


def fixations_to_grid(fix_u8, H, W):
    """Full-resolution fixation maps on the training grid: uint8 [n, H0, W0] -> uint8 [n, H, W] of 0 / 255, for the losses with an
    NSS term (P3DSession.upload_fixations).  A grid cell is fixated if any source pixel with byte >= 128 maps to it by
    (r * H // H0, c * W // W0).  Host numpy.  The reference has no counterpart: it uses fixation maps only at 1080x960, to score
    (test.py:167-176), and never trains on them."""
    f = np.asarray(fix_u8)
    if f.ndim == 2:
        f = f[None]
    if f.ndim != 3 or f.dtype != np.uint8 or f.size == 0:
        raise ValueError("expected [n, H0, W0] uint8 fixation maps")
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("grid %r x %r" % (H, W))
    n, H0, W0 = f.shape
    out = np.zeros((n, H, W), np.uint8)
    k, r, c = np.nonzero(f >= 128)
    out[k, r * H // H0, c * W // W0] = 255
    return out
