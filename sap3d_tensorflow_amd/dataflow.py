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


def clip_tuples(frames_per_video, video_length=16, overlap=15, skip_head=11):
    """The clip list of VideoDataset.setup_video_dataset_p3d (dataflow.py:43-52) before its shuffle: (video, first frame) for
    first frames skip_head, skip_head + step, .. with step = video_length - overlap, video by video, a video's list ending at
    the first clip that would leave it (:49-50)."""
    if not overlap < video_length:
        raise ValueError("overlap should be smaller than video_length")          # dataflow.py:42
    step = video_length - overlap
    out = []
    for i, total in enumerate(frames_per_video):
        for j in range(skip_head, int(total), step):
            if j + video_length > total:
                break
            out.append((i, j))
    return out


def split_clips(tuples, props, rng):
    """dataflow.py:56-60: the shuffled list cut at int(n * props) -> (training tuples, validation tuples).  The reference
    shuffles with the unseeded global `random`; here the order is rng.permutation(n) of a numpy Generator (or a seed for
    np.random.default_rng), so a split can be reproduced.  UNPINNED: no run of the reference yields the same split."""
    if not hasattr(rng, "permutation"):
        rng = np.random.default_rng(rng)
    order = rng.permutation(len(tuples))
    shuffled = [tuple(tuples[i]) for i in order]
    n = int(len(shuffled) * props)
    return shuffled[:n], shuffled[n:]


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


def _post_cfg(sigma, radius, norm):
    from . import _lib
    if norm not in _lib.NORMS:
        raise ValueError("normalisation %r: have %s" % (norm, sorted(_lib.NORMS)))
    return _lib.P3dPostprocess(float(sigma), int(radius), _lib.NORMS[norm])


def blur_taps(sigma, radius=0):
    """The weights of the Gaussian of P3DSession.set_postprocess (p3d_blur_taps, host only): float32 [2 r + 1] with
    r = radius, or cv2's rule for float images when radius is 0 (r = (int(rint(8 sigma + 1)) | 1) // 2); w_k = float32(e_k / sum e),
    e_k = exp(-(k - r)^2 / (2 sigma^2)) in float64.  sigma == 0: the empty array (no blur)."""
    from . import _lib
    taps = np.empty(2 * _lib.P3D_BLUR_MAX_RADIUS + 1, np.float32)
    r = C.c_int(0)
    check(lib().p3d_blur_taps(float(sigma), int(radius), taps.ctypes.data_as(C.POINTER(C.c_float)), taps.size, C.byref(r)))
    return taps[:2 * r.value + 1].copy() if r.value > 0 else np.zeros(0, np.float32)


def blur_strip(radius):
    """(columns, rows, LDS bytes) of one block of the blur's vertical pass at this radius (p3d_debug_blur_strip, host only)."""
    c, r, b = C.c_int(0), C.c_int(0), C.c_int(0)
    check(lib().p3d_debug_blur_strip(int(radius), C.byref(c), C.byref(r), C.byref(b)))
    return c.value, r.value, b.value


def gaussian_blur(maps, sigma, radius=0, device=0):
    """The separable Gaussian of include/p3d_hip.h on float32 maps [n, H, W] or [H, W], same shape out: blur_taps' weights, a
    horizontal then a vertical float32 pass with reflect-101 borders (csrc/postprocess.hip).  Needs r <= min(H, W) - 1."""
    m = np.ascontiguousarray(maps, dtype=np.float32)
    single = m.ndim == 2
    if single:
        m = m[None]
    if m.ndim != 3 or m.size == 0:
        raise ValueError("expected [n, H, W] or [H, W] float32 maps")
    out = np.empty_like(m)
    fp = C.POINTER(C.c_float)
    check(lib().p3d_gaussian_blur(device, m.ctypes.data_as(fp), m.shape[0], m.shape[1], m.shape[2], float(sigma), int(radius),
                                  out.ctypes.data_as(fp)))
    return out[0] if single else out


def _temporal_cfg(kind, sigma, radius, alpha):
    from . import _lib
    if kind not in _lib.TEMPORAL_KINDS:
        raise ValueError("temporal kind %r: have %s" % (kind, sorted(_lib.TEMPORAL_KINDS)))
    return _lib.P3dVideoTemporal(_lib.TEMPORAL_KINDS[kind], float(sigma), int(radius), float(alpha))


def temporal_filter(maps, kind, sigma=0., radius=0, alpha=0., first=0, n=None, device=0, shots=None, counts=None, mode="newest", offset=0):
    """The temporal stage of P3DSession.set_video_temporal on supplied maps (p3d_temporal_filter): maps [F, ...] float32, one per
    frame, trailing axes flattened to pixels and every count 1.  kind "gauss": the Gaussian of blur_taps(sigma, radius) along
    the frame axis with reflect-101 at the first and last frame, r in 1 .. 24 and r <= F - 1; "ema": m_f = alpha m_{f-1} +
    (1 - alpha) v_f from m_0 = v_0.  Returns frames first .. first + n - 1 (all by default), [n, ...].  shots: the starts of a shot
    table, ascending from 0 (p3d_temporal_filter_shots): the Gaussian reflects at the ends of every shot, periodically, so any r in
    1 .. 24 is legal, and the moving average restarts at every shot; then counts [F] (with mode "mean": the maps are sums) and offset
    (0 .. 3 floats off a 16-byte boundary, every device buffer between guards) are read as well."""
    m = np.ascontiguousarray(maps, dtype=np.float32)
    if m.ndim < 1 or m.size == 0:
        raise ValueError("expected [F, ...] float32 maps")
    F = m.shape[0]
    n = F - int(first) if n is None else int(n)
    cfg = _temporal_cfg(kind, sigma, radius, alpha)
    out = np.empty((max(n, 0),) + m.shape[1:], np.float32)
    fp = C.POINTER(C.c_float)
    if shots is None:
        check(lib().p3d_temporal_filter(device, C.byref(cfg), m.ctypes.data_as(fp), F, m.size // F, int(first), n, out.ctypes.data_as(fp)))
        return out
    from . import _lib
    st = np.ascontiguousarray(shots, np.int32).ravel()
    cnt = None if counts is None else np.ascontiguousarray(counts, np.int32)
    i32 = C.POINTER(C.c_int32)
    check(lib().p3d_temporal_filter_shots(device, _lib.VIDEO_MODES[mode], C.byref(cfg), m.ctypes.data_as(fp), None if cnt is None else cnt.ctypes.data_as(i32),
                                          F, m.size // F, st.ctypes.data_as(i32), len(st), int(first), n, int(offset), out.ctypes.data_as(fp)))
    return out


def temporal_plan(kind, radius, hw, n):
    """(pixels, consecutive output frames, LDS bytes) of one block of the temporal launch for a read of n frames of hw pixels
    (p3d_debug_video_temporal_plan, host only); kind "gauss" with its effective radius, or "ema"."""
    from . import _lib
    if kind not in ("gauss", "ema"):
        raise ValueError("temporal kind %r: have ['ema', 'gauss']" % (kind,))
    p, f, b = C.c_int(0), C.c_int(0), C.c_int(0)
    check(lib().p3d_debug_video_temporal_plan(_lib.TEMPORAL_KINDS[kind], int(radius), int(hw), int(n), C.byref(p), C.byref(f), C.byref(b)))
    return p.value, f.value, b.value


def temporal_desc(kind, F, hw, first=0, n=None, sigma=0., radius=0, alpha=0., mode="newest"):
    """dict(kernel, flops, bytes): what the temporal launch of a read-out of frames first .. first + n - 1 of F frames of hw pixels
    claims (p3d_debug_video_temporal_desc, host only)."""
    from . import _lib
    if mode not in _lib.VIDEO_MODES:
        raise ValueError("video mode %r: have %s" % (mode, sorted(_lib.VIDEO_MODES)))
    cfg = _temporal_cfg(kind, sigma, radius, alpha)
    n = int(F) - int(first) if n is None else int(n)
    name = C.create_string_buffer(64)
    flops, nbytes = C.c_double(0.), C.c_double(0.)
    check(lib().p3d_debug_video_temporal_desc(_lib.VIDEO_MODES[mode], C.byref(cfg), int(F), int(hw), int(first), n, name, 64, C.byref(flops),
                                              C.byref(nbytes)))
    return dict(kernel=name.value.decode(), flops=flops.value, bytes=nbytes.value)


def _match_cfg(hist_match, nbins=256):
    """(P3dHistMatch, the arrays it points to) of what P3DSession.set_hist_match takes: None / "off", "density", or a table
    (cdf, bin_centers) of float64 [nt] each."""
    from . import _lib
    if hist_match is None or (isinstance(hist_match, str) and hist_match == "off"):
        return _lib.P3dHistMatch(_lib.MATCH_MODES["off"], int(nbins), 0, None, None), ()
    if isinstance(hist_match, str):
        if hist_match != "density":
            raise ValueError("hist_match %r: 'off', 'density' or a table (cdf, bin_centers)" % (hist_match,))
        return _lib.P3dHistMatch(_lib.MATCH_MODES["density"], int(nbins), 0, None, None), ()
    cdf, centres = hist_match
    cdf = np.ascontiguousarray(cdf, dtype=np.float64)
    centres = np.ascontiguousarray(centres, dtype=np.float64)
    if cdf.ndim != 1 or cdf.shape != centres.shape:
        raise ValueError("a table is (cdf, bin_centers), float64 [nt] each")
    dp = C.POINTER(C.c_double)
    return _lib.P3dHistMatch(_lib.MATCH_MODES["table"], int(nbins), cdf.size, cdf.ctypes.data_as(dp), centres.ctypes.data_as(dp)), (cdf, centres)


def load_match_table(path):
    """(cdf, bin_centers), float64 [nt] each, of an .npz that holds `cdf` and `bin_centers` (the --match-hist FILE of the drivers);
    one map's cumulative_distribution output, or tables pooled over a dataset on the host."""
    with np.load(path) as d:
        if "cdf" not in d or "bin_centers" not in d:
            raise ValueError("%s: a match table holds `cdf` and `bin_centers`" % path)
        cdf, centres = np.asarray(d["cdf"], np.float64), np.asarray(d["bin_centers"], np.float64)
    if cdf.ndim != 1 or cdf.shape != centres.shape or cdf.size < 2:
        raise ValueError("%s: cdf and bin_centers are float64 [nt] each, nt >= 2" % path)
    return cdf, centres


def _maps3(maps):
    m = np.ascontiguousarray(maps, dtype=np.float32)
    single = m.ndim == 2
    if single:
        m = m[None]
    if m.ndim != 3 or m.size == 0:
        raise ValueError("expected [n, H, W] or [H, W] float32 maps")
    return m, single


def cumulative_distribution(maps, nbins=256, with_counts=False, device=0):
    """skimage.exposure.cumulative_distribution(map, nbins) of float32 maps [n, H, W] or [H, W] on the GPU (csrc/hist_match.hip;
    the law, np.histogram then cumsum / N in float64, is in include/p3d_hip.h) -> (cdf, bin_centers), float64 [n, nbins] /
    [nbins] each; with_counts: (cdf, bin_centers, counts int64) -- np.histogram(map.astype(float64), nbins)[0]."""
    m, single = _maps3(maps)
    n, nb = m.shape[0], int(nbins)
    if not 2 <= nb <= 1024:
        raise ValueError("nbins must be in [2, 1024]")
    cdf, centres, counts = np.empty((n, nb), np.float64), np.empty((n, nb), np.float64), np.empty((n, nb), np.int64)
    dp = C.POINTER(C.c_double)
    check(lib().p3d_cumulative_distribution(device, m.ctypes.data_as(C.POINTER(C.c_float)), n, m.shape[1], m.shape[2], nb,
                                            counts.ctypes.data_as(C.POINTER(C.c_int64)) if with_counts else None,
                                            cdf.ctypes.data_as(dp), centres.ctypes.data_as(dp)))
    out = (cdf, centres, counts) if with_counts else (cdf, centres)
    return tuple(a[0] for a in out) if single else out


def match_hist(maps, cdf, bin_centers, nbins=256, device=0):
    """The reference's utils/metric_utils.py:56-84 match_hist(image, cdf, bin_centers, nbins) on the GPU: float32 maps [n, H, W] or
    [H, W] remapped so that their histogram follows the target table's -> the same shape, float32.  cdf / bin_centers: float64
    [nt] (one table for every map) or [n, nt] (one per map), finite and non-decreasing."""
    m, single = _maps3(maps)
    c = np.ascontiguousarray(cdf, dtype=np.float64)
    x = np.ascontiguousarray(bin_centers, dtype=np.float64)
    if c.shape != x.shape or c.ndim not in (1, 2) or (c.ndim == 2 and c.shape[0] != m.shape[0]):
        raise ValueError("cdf and bin_centers are float64 [nt], or [n, nt] with one table per map")
    out = np.empty_like(m)
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    check(lib().p3d_match_hist(device, m.ctypes.data_as(fp), m.shape[0], m.shape[1], m.shape[2], int(nbins), c.ctypes.data_as(dp),
                               x.ctypes.data_as(dp), 1 if c.ndim == 1 else c.shape[0], c.shape[-1], out.ctypes.data_as(fp)))
    return out[0] if single else out


def match_hist_maps(maps, targets, nbins=256, device=0):
    """match_hist(map, *cumulative_distribution(target, nbins), nbins) for every map and its own target image (the reference's
    recipe, utils/metric_utils.py:321), both tables built on the device.  maps, targets: float32 [n, H, W] or [H, W]."""
    m, single = _maps3(maps)
    t, _ = _maps3(targets)
    if t.shape != m.shape:
        raise ValueError("targets must have the maps' shape %s" % (m.shape,))
    out = np.empty_like(m)
    fp = C.POINTER(C.c_float)
    check(lib().p3d_match_hist_maps(device, m.ctypes.data_as(fp), t.ctypes.data_as(fp), m.shape[0], m.shape[1], m.shape[2], int(nbins),
                                    out.ctypes.data_as(fp)))
    return out[0] if single else out


def postprocess_maps(maps, size, sigma=0., radius=0, norm="none", scale=None, device=0, hist_match=None, nbins=256, prior=None,
                     prior_mode="off", prior_weight=0.):
    """The output stage of P3DSession.set_postprocess on supplied maps (p3d_postprocess_maps): float32 [n, h, w], [h, w], or
    [n, h, w, c] of which channel 0 is taken -> resize_linear to size = (H, W), gaussian_blur, then each map divided by its
    maximum (norm="max") or brought to its range (norm="range").  -> float32 [n, H, W]; with `scale`, the uint8 images
    saturate_cast(float32(v * scale)) instead.  hist_match: a table (cdf, bin_centers) as P3DSession.set_hist_match takes it --
    every map is matched to it (match_hist with `nbins`) after the blur and before the normalisation.  prior (float32 [H, W]),
    prior_mode ("mul" / "mix") and prior_weight: P3DSession.set_prior_stage's stage, after the blur and before the matching
    (p3d_postprocess_maps_prior)."""
    m = np.ascontiguousarray(maps, dtype=np.float32)
    single = m.ndim == 2
    if single:
        m = m[None]
    if m.ndim not in (3, 4) or m.size == 0:
        raise ValueError("expected [n, h, w], [h, w] or [n, h, w, c] float32 maps")
    H, W = (size, size) if np.isscalar(size) else size
    cfg = _post_cfg(sigma, radius, norm)
    out = np.empty((m.shape[0], H, W), np.float32 if scale is None else np.uint8)
    fp, u8 = C.POINTER(C.c_float), C.POINTER(C.c_ubyte)
    args = (device, m.ctypes.data_as(fp), m.shape[0], m.shape[1], m.shape[2], m.shape[3] if m.ndim == 4 else 1, int(H), int(W), C.byref(cfg))
    outs = (0.0 if scale is None else float(scale), out.ctypes.data_as(fp) if scale is None else None,
            out.ctypes.data_as(u8) if scale is not None else None)
    # the three entry points are supersets of one another: a call takes the lowest that has every argument it was given
    level = 2 if prior is not None or prior_mode != "off" else 1 if hist_match is not None else 0
    if level == 2:
        md = _prior_mode(prior_mode, prior_weight)
        g = None if prior is None else np.ascontiguousarray(prior, dtype=np.float32)
        if g is not None and g.shape != (H, W):
            raise ValueError("the prior is %s, the output %s" % (g.shape, (H, W)))
    mc, keep = _match_cfg(hist_match if hist_match is not None else "off", nbins)
    if level >= 1:
        args += (C.byref(mc),)
    if level == 2:
        args += (g.ctypes.data_as(fp) if g is not None else None, md, float(prior_weight))
    check(getattr(lib(), "p3d_postprocess_maps" + ("", "_match", "_prior")[level])(*(args + outs)))
    return out[0] if single else out


def _u8_maps3(maps):
    m = np.asarray(maps)
    if m.dtype != np.uint8:
        raise ValueError("prior maps are uint8 images")
    m = np.ascontiguousarray(m[None] if m.ndim == 2 else m)
    if m.ndim != 3 or m.size == 0:
        raise ValueError("expected [n, H, W] or [H, W] uint8 maps")
    return m


def _prior_kind(kind):
    from . import _lib
    if kind not in _lib.PRIOR_KINDS:
        raise ValueError("prior kind %r: have %s" % (kind, sorted(_lib.PRIOR_KINDS)))
    return _lib.PRIOR_KINDS[kind]


def _prior_mode(mode, a):
    from . import _lib
    if mode not in _lib.PRIOR_MODES:
        raise ValueError("prior mode %r: have %s" % (mode, sorted(_lib.PRIOR_MODES)))
    if mode != "off" and not 0. <= float(a) <= 1.:
        raise ValueError("the prior weight must be in [0, 1]")
    return _lib.PRIOR_MODES[mode]


def prior_count(maps, kind="fixations", sign=1, counts=None, offset=0, device=0):
    """Test hook (p3d_debug_prior_count): uint8 maps [n, H, W] counted into `counts` (uint32 [H, W]; None: zeros) by
    csrc/prior.hip's prior_count_kernel, the maps `offset` bytes past a 4-byte boundary -> (uint32 [H, W], underflow flag)."""
    m = _u8_maps3(maps)
    n, H, W = m.shape
    cin = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
    if cin is not None and cin.shape != (H, W):
        raise ValueError("counts are uint32 %s" % ((H, W),))
    out, flag = np.empty((H, W), np.uint32), C.c_int(0)
    u32 = C.POINTER(C.c_uint32)
    check(lib().p3d_debug_prior_count(device, _prior_kind(kind), m.ctypes.data_as(C.POINTER(C.c_ubyte)), n, H, W, int(sign),
                                      cin.ctypes.data_as(u32) if cin is not None else None, int(offset), out.ctypes.data_as(u32),
                                      C.byref(flag)))
    return out, bool(flag.value)


def prior_count_plan(n, H, W, offset=0):
    """(four-pixel word lanes, one-pixel byte lanes, map slices) of the count launch on n maps of H x W bytes (host only)."""
    w, s1, sl = C.c_int64(0), C.c_int64(0), C.c_int(0)
    check(lib().p3d_debug_prior_count_plan(int(n), int(H), int(W), int(offset), C.byref(w), C.byref(s1), C.byref(sl)))
    return w.value, s1.value, sl.value


def fixation_prior(maps, kind="fixations", sigma=0., radius=0, device=0):
    """A fixation prior from uint8 maps [n, H, W] on the GPU, without a session: the counts (csrc/prior.hip), float32, the Gaussian
    of gaussian_blur, then / max -> float32 [H, W], 1 at the peak (P3DSession.finish_prior's law, include/p3d_hip.h)."""
    counts, flag = prior_count(maps, kind, device=device)
    if not counts.any():
        raise ValueError("every count is zero")
    return postprocess_maps(counts.astype(np.float32), counts.shape, sigma=sigma, radius=radius, norm="max", device=device)


def apply_prior(maps, prior, mode="mul", a=0., offset=0, device=0):
    """P3DSession.set_prior_stage's stage on supplied maps (p3d_debug_prior_apply): float32 [n, H, W] or [H, W] combined with
    prior float32 [H, W] -- "mul": v * ((1 - a) g + a); "mix": (1 - a) v + a g, in float32 -> the same shape.  offset (test
    hook): the maps start (offset & 3), the prior ((offset >> 2) & 3) floats past a 16-byte boundary on the device."""
    m, single = _maps3(maps)
    g = np.ascontiguousarray(prior, dtype=np.float32)
    if g.shape != m.shape[1:]:
        raise ValueError("the prior is %s, the maps %s" % (g.shape, m.shape[1:]))
    md = _prior_mode(mode, a)
    if mode == "off":
        raise ValueError("apply_prior: mode 'mul' or 'mix'")
    out = np.empty_like(m)
    fp = C.POINTER(C.c_float)
    check(lib().p3d_debug_prior_apply(device, md, float(a), m.ctypes.data_as(fp), m.shape[0], m.shape[1], m.shape[2], g.ctypes.data_as(fp),
                                      int(offset), out.ctypes.data_as(fp)))
    return out[0] if single else out


def fixation_words(H, W):
    """Words per packed fixation map: ceil(H * W / 64) (include/p3d_hip.h, STORE)."""
    return (int(H) * int(W) + 63) // 64


def pack_fixations(maps, offset=0, device=0):
    """Test hook (p3d_debug_fix_pack): uint8 maps [n, H, W] or [H, W] -> uint64 [n, ceil(H W / 64)], bit j of word k set where byte
    64 k + j is >= 128 (csrc/fixpool.hip's fix_pack_kernel); the maps start `offset` bytes past a 16-byte boundary."""
    m = _u8_maps3(maps)
    n, H, W = m.shape
    out = np.empty((n, fixation_words(H, W)), np.uint64)
    check(lib().p3d_debug_fix_pack(device, m.ctypes.data_as(C.POINTER(C.c_ubyte)), n, H, W, int(offset), out.ctypes.data_as(C.POINTER(C.c_uint64))))
    return out


def _pool_ids(words, size, others):
    w = np.ascontiguousarray(words, dtype=np.uint64)
    H, W = (size, size) if np.isscalar(size) else tuple(size)
    if w.ndim != 2 or w.shape[1] != fixation_words(H, W):
        raise ValueError("packed maps are uint64 [capacity, %d] for %d x %d maps" % (fixation_words(H, W), H, W))
    ids = np.ascontiguousarray(others, dtype=np.int32)
    if ids.ndim != 2:
        raise ValueError("others is int [B, M]")
    return w, int(H), int(W), ids


def union_fixations(words, size, others, device=0):
    """Test hook (p3d_debug_fix_union): for every row of others [B, M] (slots of the packed pool `words`, uint64 [capacity, nw]) the
    OR of its maps -> (uni uint64 [B, nw], the exclusive prefix of the words' bit counts uint32 [B, nw], n_other uint32 [B])."""
    w, H, W, ids = _pool_ids(words, size, others)
    B, M = ids.shape
    uni, prefix, n_other = np.empty((B, w.shape[1]), np.uint64), np.empty((B, w.shape[1]), np.uint32), np.empty(B, np.uint32)
    u64, u32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    check(lib().p3d_debug_fix_union(device, w.ctypes.data_as(u64), w.shape[0], H, W, ids.ctypes.data_as(C.POINTER(C.c_int)), B, M,
                                    uni.ctypes.data_as(u64), prefix.ctypes.data_as(u32), n_other.ctypes.data_as(u32)))
    return uni, prefix, n_other


def select_fixations(words, size, others, ranks, n_rows, n_rep, device=0):
    """Test hook (p3d_debug_fix_select): the union of every row of others, then the pixel index of every rank's set bit --
    np.nonzero(other.ravel())[0][ranks].  ranks: int32, [n_rows[b], n_rep] per row, concatenated -> int32 of the same layout."""
    w, H, W, ids = _pool_ids(words, size, others)
    B, M = ids.shape
    r = np.ascontiguousarray(ranks, dtype=np.int32).ravel()
    rows = np.ascontiguousarray(n_rows, dtype=np.int32)
    if rows.shape != (B,) or r.size != int(np.sum(rows.astype(np.int64))) * int(n_rep):
        raise ValueError("ranks hold sum(n_rows) * n_rep entries, n_rows one per row of others")
    out = np.empty(r.size, np.int32)
    ip = C.POINTER(C.c_int)
    check(lib().p3d_debug_fix_select(device, w.ctypes.data_as(C.POINTER(C.c_uint64)), w.shape[0], H, W, ids.ctypes.data_as(ip), B, M,
                                     r.ctypes.data_as(ip), rows.ctypes.data_as(ip), int(n_rep), out.ctypes.data_as(ip)))
    return out


def postprocess_maps_both(maps, size, sigma=0., radius=0, norm="none", scale=255., device=0):
    """postprocess_maps with both outputs of one call -> (float32 [n, H, W], uint8 [n, H, W])."""
    m = np.ascontiguousarray(maps, dtype=np.float32)
    if m.ndim not in (3, 4) or m.size == 0:
        raise ValueError("expected [n, h, w] or [n, h, w, c] float32 maps")
    H, W = (size, size) if np.isscalar(size) else size
    cfg = _post_cfg(sigma, radius, norm)
    f, b = np.empty((m.shape[0], H, W), np.float32), np.empty((m.shape[0], H, W), np.uint8)
    fp, u8 = C.POINTER(C.c_float), C.POINTER(C.c_ubyte)
    check(lib().p3d_postprocess_maps(device, m.ctypes.data_as(fp), m.shape[0], m.shape[1], m.shape[2], m.shape[3] if m.ndim == 4 else 1,
                                     int(H), int(W), C.byref(cfg), float(scale), f.ctypes.data_as(fp), b.ctypes.data_as(u8)))
    return f, b


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


def render_table(colormap="jet", alpha=0.6, opacity="ramp", gate=0):
    """The colour and opacity table of p3d_render (include/p3d_hip.h, "Rendering 8-bit maps") -> uint32 [256], entry v packed
    b | g << 8 | r << 16 | o << 24.  Built here in float64 with x = v / 255 and byte(c) = floor(255 c + 0.5).  The colour maps are
    this project's own, not cv2's: "grey" (v, v, v); "hot" r = clamp(3x), g = clamp(3x - 1), b = clamp(3x - 2); "jet"
    r = clamp(1.5 - |4x - 3|), g = clamp(1.5 - |4x - 2|), b = clamp(1.5 - |4x - 1|), clamp to [0, 1].  opacity "constant":
    o = floor(255 alpha + 0.5) at every level; "ramp": o_v = floor(alpha v + 0.5).  Either is 0 below level `gate`."""
    from ._lib import RENDER_COLORMAPS, RENDER_OPACITIES
    if colormap not in RENDER_COLORMAPS:
        raise ValueError("colormap %r: have %s" % (colormap, list(RENDER_COLORMAPS)))
    if opacity not in RENDER_OPACITIES:
        raise ValueError("opacity %r: have %s" % (opacity, list(RENDER_OPACITIES)))
    alpha, gate = float(alpha), int(gate)
    if not 0. <= alpha <= 1.:
        raise ValueError("alpha is in [0, 1]")
    if not 0 <= gate <= 256:
        raise ValueError("gate is a level, 0 .. 256")
    v = np.arange(256, dtype=np.float64)
    x = v / 255.

    def byte(c):
        return np.floor(255. * np.clip(c, 0., 1.) + 0.5).astype(np.uint32)
    if colormap == "grey":
        r = g = b = np.arange(256, dtype=np.uint32)
    elif colormap == "hot":
        r, g, b = byte(3. * x), byte(3. * x - 1.), byte(3. * x - 2.)
    else:
        r, g, b = byte(1.5 - np.abs(4. * x - 3.)), byte(1.5 - np.abs(4. * x - 2.)), byte(1.5 - np.abs(4. * x - 1.))
    o = np.floor((alpha * v if opacity == "ramp" else np.full(256, 255. * alpha)) + 0.5).astype(np.uint32)
    o[:min(gate, 256)] = 0
    return (b | (g << 8) | (r << 16) | (o << 24)).astype(np.uint32)


def render_cfg(table, contour=None, thickness=1, contour_color=(255, 255, 255)):
    """p3d_render from a uint32 [256] table, a contour level (None or 0: off), its thickness and its colour as (R, G, B)."""
    from ._lib import P3dRender
    t = np.ascontiguousarray(table)
    if t.dtype != np.uint32 or t.shape != (256,):
        raise ValueError("the table is uint32 [256] (dataflow.render_table)")
    rgb = tuple(int(c) for c in contour_color)
    if len(rgb) != 3 or min(rgb) < 0 or max(rgb) > 255:
        raise ValueError("contour_color is (R, G, B) bytes")
    cfg = P3dRender()
    C.memmove(cfg.table, t.ctypes.data, 1024)
    cfg.contour_level = int(contour) if contour else 0
    cfg.contour_thickness = int(thickness)
    cfg.contour_bgr[0], cfg.contour_bgr[1], cfg.contour_bgr[2] = rgb[2], rgb[1], rgb[0]
    return cfg


def render_plan(H, W, n=1, thickness=0, offset=0):
    """Test hook (p3d_debug_render_plan, host only): (rows, cols, pixels) per block of the render launch; cols 0: flat runs."""
    r, c, p = C.c_int(0), C.c_int(0), C.c_int64(0)
    check(lib().p3d_debug_render_plan(int(H), int(W), int(n), int(thickness), int(offset), C.byref(r), C.byref(c), C.byref(p)))
    return r.value, c.value, p.value


def render_overlay(sal, frames, table, contour=None, thickness=1, contour_color=(255, 255, 255), device=0, offset=None):
    """8-bit saliency maps uint8 [n, H, W] or [H, W] laid over frames uint8 [n, H, W, 3] in B, G, R order (None: the plain heat
    map) through `table` (render_table) -> uint8 [n, H, W, 3] (include/p3d_hip.h, "Rendering 8-bit maps"; p3d_render_u8).
    contour: the level whose iso-line is drawn, `thickness` pixels wide (1 .. 4), in contour_color (R, G, B).  offset (0 .. 15):
    the test hook p3d_debug_render_u8, every device buffer between guards and shifted off a 16-byte boundary."""
    s = np.ascontiguousarray(sal)
    if s.dtype != np.uint8 or s.ndim not in (2, 3) or s.size == 0:
        raise ValueError("saliency maps are non-empty uint8 [H, W] or [n, H, W]")
    s3 = s[None] if s.ndim == 2 else s
    f = None
    if frames is not None:
        f = np.ascontiguousarray(frames)
        if f.dtype != np.uint8 or f.shape != s3.shape + (3,) and f.shape != s.shape + (3,):
            raise ValueError("frames are uint8 %s, the maps' shape with three channels" % (s3.shape + (3,),))
    cfg = render_cfg(table, contour, thickness, contour_color)
    n, H, W = s3.shape
    out = np.empty((n, H, W, 3), np.uint8)
    u8 = C.POINTER(C.c_ubyte)
    args = (device, s3.ctypes.data_as(u8), None if f is None else f.ctypes.data_as(u8), n, H, W, C.byref(cfg))
    if offset is None:
        check(lib().p3d_render_u8(*args, out.ctypes.data_as(u8)))
    else:
        check(lib().p3d_debug_render_u8(*args, int(offset), out.ctypes.data_as(u8)))
    return out if s.ndim == 3 else out[0]


def _reframe_shape(sal, crop):
    s = np.ascontiguousarray(sal)
    if s.dtype != np.uint8 or s.ndim not in (2, 3) or s.size == 0:
        raise ValueError("saliency maps are non-empty uint8 [H, W] or [n, H, W]")
    s3 = s[None] if s.ndim == 2 else s
    hc, wc = (int(crop), int(crop)) if np.isscalar(crop) else (int(crop[0]), int(crop[1]))
    return s3, hc, wc


def reframe_track(sal, crop, gate=0, smooth=0):
    """The law of include/p3d_hip.h, "Reframing around 8-bit maps", stated in numpy on the host (integers only): saliency maps uint8
    [n, H, W] (or [H, W]: one frame), crop = (hc, wc), the gate level and the smoothing radius -> (track int32 [n, 2], raw int32
    [n, 2], mass uint32 [n, 3]): the smoothed and the raw (Y, X) of every frame, and M_best, M_smoothed, T.  The n maps are the
    whole world of the smoothing filter."""
    s3, hc, wc = _reframe_shape(sal, crop)
    n, H, W = s3.shape
    gate, R = int(gate), int(smooth)
    if n > 65535 or H * W > 2 ** 23:
        raise ValueError("1 .. 65535 maps of at most 2^23 pixels")
    if not (1 <= hc <= H and 1 <= wc <= W):
        raise ValueError("the window is %d x %d, the map %d x %d" % (hc, wc, H, W))
    if not 0 <= gate <= 255 or not 0 <= R <= 255:
        raise ValueError("the gate is a level 0 .. 255, the smoothing radius 0 .. 255 frames")
    Hp, Wp = H - hc + 1, W - wc + 1
    D = np.abs(2 * np.arange(Hp, dtype=np.int64) - (H - hc))[:, None] + np.abs(2 * np.arange(Wp, dtype=np.int64) - (W - wc))[None, :]
    raw = np.empty((n, 2), np.int64)
    mass = np.empty((n, 3), np.int64)
    tables = []
    for f in range(n):
        w = np.where(s3[f] >= gate, s3[f], 0).astype(np.int64)
        S = np.zeros((H + 1, W + 1), np.int64)
        S[1:, 1:] = w.cumsum(0).cumsum(1)
        M = S[hc:, wc:] - S[:Hp, wc:] - S[hc:, :Wp] + S[:Hp, :Wp]
        best = M.max()
        d = np.where(M == best, D, np.iinfo(np.int64).max)
        y0, x0 = np.unravel_index(np.argmin(d), d.shape)      # the first of the smallest D in row-major order: smallest y0, then x0
        raw[f] = (y0, x0)
        mass[f, 0], mass[f, 2] = best, S[H, W]
        tables.append(M if R else None)
    if R:
        idx = np.clip(np.arange(n)[:, None] + np.arange(-R, R + 1)[None, :], 0, n - 1)
        track = (2 * raw[idx].sum(axis=1) + (2 * R + 1)) // (2 * (2 * R + 1))
        mass[:, 1] = [tables[f][track[f, 0], track[f, 1]] for f in range(n)]
    else:
        track = raw.copy()
        mass[:, 1] = mass[:, 0]
    return track.astype(np.int32), raw.astype(np.int32), mass.astype(np.uint32)


def reframe_crop(frames, track, crop):
    """frames uint8 [n, H, W, 3], a track int [n, 2] of (Y, X) and crop = (hc, wc) -> uint8 [n, hc, wc, 3], frame f's window at its
    track position, not resized (the CROP rule of include/p3d_hip.h, "Reframing around 8-bit maps")."""
    f = np.asarray(frames)
    t = np.asarray(track)
    hc, wc = (int(crop), int(crop)) if np.isscalar(crop) else (int(crop[0]), int(crop[1]))
    if f.dtype != np.uint8 or f.ndim != 4 or f.shape[3] != 3 or t.shape != (f.shape[0], 2):
        raise ValueError("frames are uint8 [n, H, W, 3] and the track [n, 2]")
    if (t < 0).any() or (t[:, 0] + hc > f.shape[1]).any() or (t[:, 1] + wc > f.shape[2]).any():
        raise ValueError("a window of the track leaves the frame")
    return np.stack([f[i, y:y + hc, x:x + wc] for i, (y, x) in enumerate(t)])


def reframe_plan(H, W, crop, n=1):
    """Test hook (p3d_debug_reframe_plan, host only): dict(positions_per_block, search_blocks, maps_per_chunk, scratch_bytes) of the
    reframe launches for n maps of H x W and a window crop = (hc, wc)."""
    hc, wc = (int(crop), int(crop)) if np.isscalar(crop) else (int(crop[0]), int(crop[1]))
    p, b, m, s = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    check(lib().p3d_debug_reframe_plan(int(H), int(W), hc, wc, int(n), C.byref(p), C.byref(b), C.byref(m), C.byref(s)))
    return dict(positions_per_block=p.value, search_blocks=b.value, maps_per_chunk=m.value, scratch_bytes=s.value)


def reframe(sal, frames, crop, gate=0, smooth=0, device=0, offset=None, shots=None):
    """reframe_track and reframe_crop on the device (p3d_reframe_u8): saliency maps uint8 [n, H, W], frames uint8 [n, H, W, 3] in
    B, G, R order or None -> (track, raw, mass, crop or None).  offset (0 .. 15): the test hook p3d_debug_reframe_u8, every device
    buffer between guards and shifted off a 16-byte boundary.  shots: the starts of a shot table over the n frames, ascending from
    0 (p3d_reframe_shots_u8): the track is smoothed inside every shot, whose ends repeat."""
    from ._lib import P3dReframe
    s3, hc, wc = _reframe_shape(sal, crop)
    n, H, W = s3.shape
    f = None
    if frames is not None:
        f = np.ascontiguousarray(frames)
        if f.dtype != np.uint8 or f.shape != s3.shape + (3,):
            raise ValueError("frames are uint8 %s, the maps' shape with three channels" % (s3.shape + (3,),))
    cfg = P3dReframe(hc, wc, int(gate), int(smooth))
    track, raw, mass = np.empty((n, 2), np.int32), np.empty((n, 2), np.int32), np.empty((n, 3), np.uint32)
    out = None if f is None or not (1 <= hc <= H and 1 <= wc <= W) else np.empty((n, hc, wc, 3), np.uint8)
    if f is not None and out is None:
        out = np.empty((1,), np.uint8)                        # (the library refuses the window before it writes)
    u8, i32, u32 = C.POINTER(C.c_ubyte), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    head = (device, s3.ctypes.data_as(u8), None if f is None else f.ctypes.data_as(u8), n, H, W, C.byref(cfg))
    tail = (track.ctypes.data_as(i32), raw.ctypes.data_as(i32), mass.ctypes.data_as(u32), None if out is None else out.ctypes.data_as(u8))
    if shots is not None:
        st = np.ascontiguousarray(shots, np.int32).ravel()
        check(lib().p3d_reframe_shots_u8(*head, st.ctypes.data_as(i32), len(st), -1 if offset is None else int(offset), *tail))
    elif offset is None:
        check(lib().p3d_reframe_u8(*head, *tail))
    else:
        check(lib().p3d_debug_reframe_u8(*head, int(offset), *tail))
    return track, raw, mass, (out if f is not None else None)


def regions_plan(H, W, n=1, max_regions=64, link=False, labels=False):
    """Test hook (p3d_debug_regions_plan, host only): dict(tile_h, tile_w, tiles_per_map, maps_per_chunk, scratch_bytes) of the
    regions launches for n maps of H x W."""
    th, tw, t, m, s = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    check(lib().p3d_debug_regions_plan(int(H), int(W), int(n), int(max_regions), int(bool(link)), int(bool(labels)), C.byref(th), C.byref(tw),
                                       C.byref(t), C.byref(m), C.byref(s)))
    return dict(tile_h=th.value, tile_w=tw.value, tiles_per_map=t.value, maps_per_chunk=m.value, scratch_bytes=s.value)


def regions_cfg(gate, connectivity=8, min_area=1, max_regions=64, link=False):
    """The five ints of include/p3d_hip.h's CONFIG ("Salient regions of 8-bit maps") in the order of the P3D_REGIONS_* indices."""
    from . import _lib
    cfg = (C.c_int * 5)()
    for k, v in ((_lib.P3D_REGIONS_GATE, gate), (_lib.P3D_REGIONS_CONNECTIVITY, connectivity), (_lib.P3D_REGIONS_MIN_AREA, min_area),
                 (_lib.P3D_REGIONS_MAX_REGIONS, max_regions), (_lib.P3D_REGIONS_LINK, bool(link))):
        cfg[k] = int(v)
    return cfg


def regions(sal, gate, connectivity=8, min_area=1, max_regions=None, link=False, shots=None, labels=False, device=0, offset=None):
    """The connected regions of gated saliency maps on the device (p3d_regions_u8; include/p3d_hip.h, "Salient regions of 8-bit
    maps"): maps uint8 [n, H, W] (or [H, W]: one frame) -> (regions int32 [n, K, P3D_REGION_FIELDS], counts int32 [n, 3], labels uint8
    [n, H, W] or None).  K = max_regions (default P3D_REGIONS_MAX).  link: IDs carried from frame to frame by overlap, inside the
    shots of `shots` (starts ascending from 0) where given.  offset (0 .. 15): the test hook p3d_debug_regions_u8, every device
    buffer between guards and the byte buffers shifted off a 16-byte boundary."""
    from . import _lib
    s3, _, _ = _reframe_shape(sal, 1)
    n, H, W = s3.shape
    K = _lib.P3D_REGIONS_MAX if max_regions is None else int(max_regions)
    cfg = regions_cfg(gate, connectivity, min_area, K, link)
    ok = 1 <= K <= _lib.P3D_REGIONS_MAX                      # (the library refuses the rest before it writes)
    rec = np.empty((n, K, _lib.P3D_REGION_FIELDS) if ok else (1,), np.int32)
    counts = np.empty((n, 3), np.int32)
    lab = np.empty((n, H, W), np.uint8) if labels else None
    u8, i32 = C.POINTER(C.c_ubyte), C.POINTER(C.c_int32)
    st = None if shots is None else np.ascontiguousarray(shots, np.int32).ravel()
    head = (device, s3.ctypes.data_as(u8), n, H, W, cfg, None if st is None else st.ctypes.data_as(i32), 0 if st is None else len(st))
    tail = (rec.ctypes.data_as(i32), counts.ctypes.data_as(i32), None if lab is None else lab.ctypes.data_as(u8))
    if offset is None:
        check(lib().p3d_regions_u8(*head, *tail))
    else:
        check(lib().p3d_debug_regions_u8(*head, int(offset), *tail))
    return rec, counts, lab


QPMAP_BLOCKS = (8, 16, 32, 64, 128)


def qp_law(lo, hi, gate=0, gamma=1.0):
    """The table that turns a block's level into its quantiser offset (LAW of include/p3d_hip.h, "QP maps of 8-bit maps") -> int32
    [256].  A host table, built here in float64: level v < gate gives `hi` (the background's offset); otherwise, with
    x = (v - gate) / (255 - gate), entry v = floor(hi - (hi - lo) x^gamma + 0.5) (round half up), so level `gate` gives hi, level 255
    gives lo and the entries never rise with v.  -127 <= lo <= hi <= 127; gate is a level 0 .. 254; gamma is finite and > 0 (below
    1: the offset falls early, above 1: only the most salient blocks reach lo)."""
    lo, hi, gate, gamma = int(lo), int(hi), int(gate), float(gamma)
    if not -127 <= lo <= hi <= 127:
        raise ValueError("-127 <= lo <= hi <= 127")
    if not 0 <= gate <= 254:
        raise ValueError("gate is a level, 0 .. 254")
    if not (np.isfinite(gamma) and gamma > 0.):
        raise ValueError("gamma is finite and > 0")
    v = np.arange(256, dtype=np.float64)
    x = np.clip((v - gate) / (255. - gate), 0., 1.)
    law = np.floor(hi - (hi - lo) * x ** gamma + 0.5).astype(np.int32)
    law[:gate] = hi
    return law


def qpmap_cfg(block=16, peak_weight=128, dilate=0, fall=0, rise=0, balance=True, target=0, lo=-127, hi=127):
    """The nine ints of include/p3d_hip.h's CONFIG ("QP maps of 8-bit maps") in the order of the P3D_QPMAP_* indices."""
    from . import _lib
    cfg = (C.c_int * _lib.P3D_QPMAP_FIELDS)()
    for k, v in ((_lib.P3D_QPMAP_BLOCK, block), (_lib.P3D_QPMAP_PEAK_WEIGHT, peak_weight), (_lib.P3D_QPMAP_DILATE, dilate),
                 (_lib.P3D_QPMAP_FALL, fall), (_lib.P3D_QPMAP_RISE, rise), (_lib.P3D_QPMAP_BALANCE, balance),
                 (_lib.P3D_QPMAP_TARGET, target), (_lib.P3D_QPMAP_LO, lo), (_lib.P3D_QPMAP_HI, hi)):
        cfg[k] = int(v)
    return cfg


def qpmap_plan(H, W, block=16, n=1):
    """Test hook (p3d_debug_qpmap_plan, host only): dict(strip_rows, tile_cols, blocks_per_map, maps_per_chunk, scratch_bytes) of the
    qpmap launches for n maps of H x W."""
    sr, tc, b, m, s = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    check(lib().p3d_debug_qpmap_plan(int(H), int(W), int(block), int(n), C.byref(sr), C.byref(tc), C.byref(b), C.byref(m), C.byref(s)))
    return dict(strip_rows=sr.value, tile_cols=tc.value, blocks_per_map=b.value, maps_per_chunk=m.value, scratch_bytes=s.value)


def _qp_law_array(law):
    t = np.ascontiguousarray(law)
    if t.dtype != np.int32 or t.shape != (256,):
        raise ValueError("the law is int32 [256] (dataflow.qp_law)")
    return t


def qpmap(sal, law, block=16, peak_weight=128, dilate=0, fall=0, rise=0, balance=True, target=0, lo=-127, hi=127, shots=None,
          levels=False, stats=False, device=0, offset=None):
    """Block importance and quantiser offsets of saliency maps on the device (p3d_qpmap_u8; include/p3d_hip.h, "QP maps of 8-bit
    maps"): maps uint8 [n, H, W] (or [H, W]: one frame) and a law int32 [256] (qp_law) -> (qp int32 [n, Hb, Wb], levels uint8
    [n, Hb, Wb] or None, stats int32 [n, 4] or None), Hb = ceil(H / block), Wb = ceil(W / block).  fall / rise limit every block's
    offset from frame to frame, inside the shots of `shots` (starts ascending from 0) where given.  offset (0 .. 15): the test hook
    p3d_debug_qpmap_u8, every device buffer between guards and the byte buffers shifted off a 16-byte boundary."""
    s3, _, _ = _reframe_shape(sal, 1)
    n, H, W = s3.shape
    t = _qp_law_array(law)
    cfg = qpmap_cfg(block, peak_weight, dilate, fall, rise, balance, target, lo, hi)
    B = int(block)
    grid = (n, -(-H // B), -(-W // B)) if B in QPMAP_BLOCKS else (1,)      # (the library refuses the rest before it writes)
    qp = np.empty(grid, np.int32)
    lev = np.empty(grid, np.uint8) if levels else None
    st4 = np.empty((n, 4), np.int32) if stats else None
    u8, i32 = C.POINTER(C.c_ubyte), C.POINTER(C.c_int32)
    st = None if shots is None else np.ascontiguousarray(shots, np.int32).ravel()
    head = (device, s3.ctypes.data_as(u8), n, H, W, cfg, t.ctypes.data_as(i32), None if st is None else st.ctypes.data_as(i32),
            0 if st is None else len(st))
    tail = (qp.ctypes.data_as(i32), None if lev is None else lev.ctypes.data_as(u8), None if st4 is None else st4.ctypes.data_as(i32))
    if offset is None:
        check(lib().p3d_qpmap_u8(*head, *tail))
    else:
        check(lib().p3d_debug_qpmap_u8(*head, int(offset), *tail))
    return qp, lev, st4


def prefilter_law(gate=0, full=0, gamma=1.0, strength=64):
    """The table that turns a block's level into the strength of its low-pass (the law of include/p3d_hip.h, "Pre-filtering frames by
    their 8-bit maps") -> int32 [256], every entry in 0 .. 64.  A host table, built here in float64: level v >= gate gives 0 (the
    frame is left alone where the viewers look); level v <= full gives `strength` (64: the full low-pass); between them, with
    x = (gate - v) / (gate - full) the normalised distance below the gate, entry v = floor(strength x^gamma + 0.5) (round half up), so
    the entries never rise with v.  0 <= full <= gate <= 255 (where the two rules meet the gate wins: gate = full is a step at the gate, gate = 0 leaves every entry 0); gamma is
    finite and > 0 (below 1: the smoothing comes on just under the gate, above 1: only the least salient blocks get all of it);
    strength is 0 .. 64."""
    gate, full, gamma, strength = int(gate), int(full), float(gamma), int(strength)
    if not 0 <= full <= gate <= 255:
        raise ValueError("0 <= full <= gate <= 255")
    if not (np.isfinite(gamma) and gamma > 0.):
        raise ValueError("gamma is finite and > 0")
    if not 0 <= strength <= 64:
        raise ValueError("strength is 0 .. 64")
    v = np.arange(256, dtype=np.float64)
    x = np.clip((gate - v) / max(gate - full, 1), 0., 1.)
    law = np.floor(strength * x ** gamma + 0.5).astype(np.int32)
    law[:full + 1] = strength
    law[gate:] = 0                                         # (the gate wins where the two meet)
    return law


def prefilter_cfg(block=16, peak_weight=128, dilate=0, fall=0, rise=0, radius=4, passes=1):
    """The seven ints of include/p3d_hip.h's CONFIG ("Pre-filtering frames by their 8-bit maps") in the order of the P3D_PREFILTER_*
    indices."""
    from . import _lib
    cfg = (C.c_int * _lib.P3D_PREFILTER_FIELDS)()
    for k, v in ((_lib.P3D_PREFILTER_BLOCK, block), (_lib.P3D_PREFILTER_PEAK_WEIGHT, peak_weight), (_lib.P3D_PREFILTER_DILATE, dilate),
                 (_lib.P3D_PREFILTER_FALL, fall), (_lib.P3D_PREFILTER_RISE, rise), (_lib.P3D_PREFILTER_RADIUS, radius),
                 (_lib.P3D_PREFILTER_PASSES, passes)):
        cfg[k] = int(v)
    return cfg


def prefilter_plan(H, W, block=16, radius=4, passes=1, n=1):
    """Test hook (p3d_debug_prefilter_plan, host only): dict(tile_rows, tile_cols, halo, fused, blocks_per_frame, frames_per_chunk,
    scratch_bytes, mul, shift) of the prefilter launches for n frames of H x W."""
    tr, tc, halo, fused, b, m, sh = (C.c_int(0) for _ in range(7))
    s, mul = C.c_int64(0), C.c_uint32(0)
    check(lib().p3d_debug_prefilter_plan(int(H), int(W), int(block), int(radius), int(passes), int(n), C.byref(tr), C.byref(tc),
                                         C.byref(halo), C.byref(fused), C.byref(b), C.byref(m), C.byref(s), C.byref(mul), C.byref(sh)))
    return dict(tile_rows=tr.value, tile_cols=tc.value, halo=halo.value, fused=bool(fused.value), blocks_per_frame=b.value,
                frames_per_chunk=m.value, scratch_bytes=s.value, mul=mul.value, shift=sh.value)


def _prefilter_law_array(law):
    t = np.ascontiguousarray(law)
    if t.dtype != np.int32 or t.shape != (256,):
        raise ValueError("the law is int32 [256] (dataflow.prefilter_law)")
    return t


def prefilter(sal, frames, law, block=16, peak_weight=128, dilate=0, fall=0, rise=0, radius=4, passes=1, shots=None, grid=False,
              device=0, offset=None):
    """Frames low-pass filtered away from their saliency on the device (p3d_prefilter_u8; include/p3d_hip.h, "Pre-filtering frames by
    their 8-bit maps"): maps uint8 [n, H, W] (or [H, W]: one frame), frames uint8 [n, H, W, 3] in B, G, R order and a law int32 [256]
    (prefilter_law) -> (out uint8 [n, H, W, 3], grid int32 [n, Hb, Wb] or None), Hb = ceil(H / block), Wb = ceil(W / block).  Per
    block a strength 0 .. 64 (the QP maps' level, dilation, law and limiter: fall / rise limit it from frame to frame, inside the
    shots of `shots`, starts ascending from 0, where given), interpolated between block centres into a weight per pixel; `passes`
    rounded box passes of `radius` pixels either way make the low-pass the weight blends in.  offset (0 .. 15): the test hook
    p3d_debug_prefilter_u8, every device buffer between guards and the byte buffers shifted off a 16-byte boundary."""
    s3, _, _ = _reframe_shape(sal, 1)
    n, H, W = s3.shape
    f = np.ascontiguousarray(frames)
    f = f[None] if f.ndim == 3 else f
    if f.dtype != np.uint8 or f.shape != (n, H, W, 3):
        raise ValueError("frames are %s %s, expected uint8 %s" % (f.dtype, f.shape, (n, H, W, 3)))
    t = _prefilter_law_array(law)
    cfg = prefilter_cfg(block, peak_weight, dilate, fall, rise, radius, passes)
    B = int(block)
    out = np.empty((n, H, W, 3), np.uint8)
    g = np.empty((n, -(-H // B), -(-W // B)) if B in QPMAP_BLOCKS else (1,), np.int32) if grid else None
    u8, i32 = C.POINTER(C.c_ubyte), C.POINTER(C.c_int32)
    st = None if shots is None else np.ascontiguousarray(shots, np.int32).ravel()
    head = (device, s3.ctypes.data_as(u8), f.ctypes.data_as(u8), n, H, W, cfg, t.ctypes.data_as(i32),
            None if st is None else st.ctypes.data_as(i32), 0 if st is None else len(st))
    tail = (out.ctypes.data_as(u8), None if g is None else g.ctypes.data_as(i32))
    if offset is None:
        check(lib().p3d_prefilter_u8(*head, *tail))
    else:
        check(lib().p3d_debug_prefilter_u8(*head, int(offset), *tail))
    return out, g


DISTORTION_BLOCKS = (0,) + QPMAP_BLOCKS


def distortion_law(gate=0, gamma=1.0, floor=0):
    """The table that turns a pixel's saliency level into its weight (the weight law of include/p3d_hip.h, "Distortion of frames under
    their 8-bit maps") -> int32 [256], every entry in 0 .. 255.  A host table, built here in float64: level v >= gate gives
    floor(255 (v / 255)^gamma + 0.5) (round half up), which is v itself at gamma = 1, the default w = s; level v < gate gives `floor`.
    gate is 0 .. 255 (0: no level is below it); gamma is finite and > 0; floor is 0 .. 255."""
    gate, gamma, floor = int(gate), float(gamma), int(floor)
    if not 0 <= gate <= 255:
        raise ValueError("gate is 0 .. 255")
    if not (np.isfinite(gamma) and gamma > 0.):
        raise ValueError("gamma is finite and > 0")
    if not 0 <= floor <= 255:
        raise ValueError("floor is 0 .. 255")
    v = np.arange(256, dtype=np.float64)
    law = v.astype(np.int32) if gamma == 1. else np.floor(255. * (v / 255.) ** gamma + 0.5).astype(np.int32)
    law[:gate] = floor
    return law


def distortion_cfg(block=0, gate=0):
    """The two ints of include/p3d_hip.h's CONFIG ("Distortion of frames under their 8-bit maps") in the order of the
    P3D_DISTORTION_* indices."""
    from . import _lib
    cfg = (C.c_int * _lib.P3D_DISTORTION_FIELDS)()
    cfg[_lib.P3D_DISTORTION_BLOCK], cfg[_lib.P3D_DISTORTION_GATE] = int(block), int(gate)
    return cfg


def _distortion_cfg(cfg):
    """cfg as the library takes it, and its block: a distortion_cfg(), or (block, gate), or dict(block=, gate=)."""
    from . import _lib
    if isinstance(cfg, dict):
        cfg = distortion_cfg(**cfg)
    elif not isinstance(cfg, C.Array):
        cfg = distortion_cfg(*cfg)
    return cfg, int(cfg[_lib.P3D_DISTORTION_BLOCK])


def distortion_plan(H, W, block=0, n=1):
    """Test hook (p3d_debug_distortion_plan, host only): dict(tile_rows, tile_cols, blocks_per_frame, window_rows, window_cols,
    scratch_bytes) of the distortion launches for n frames of H x W."""
    tr, tc, b, wr, wc = (C.c_int(0) for _ in range(5))
    s = C.c_int64(0)
    check(lib().p3d_debug_distortion_plan(int(H), int(W), int(block), int(n), C.byref(tr), C.byref(tc), C.byref(b), C.byref(wr),
                                          C.byref(wc), C.byref(s)))
    return dict(tile_rows=tr.value, tile_cols=tc.value, blocks_per_frame=b.value, window_rows=wr.value, window_cols=wc.value,
                scratch_bytes=s.value)


def _distortion_law_array(law):
    t = np.ascontiguousarray(law)
    if t.dtype != np.int32 or t.shape != (256,):
        raise ValueError("the weight law is int32 [256] (dataflow.distortion_law)")
    return t


def _distortion_frames(f, shape, what):
    f = np.ascontiguousarray(f)
    f = f[None] if f.ndim == 3 else f
    if f.dtype != np.uint8 or f.shape != shape:
        raise ValueError("%s frames are %s %s, expected uint8 %s" % (what, f.dtype, f.shape, shape))
    return f


def distortion(sal, ref, test, cfg, law, block_map=None, device=0, offset=None):
    """Test frames compared with reference frames under their saliency on the device (p3d_distortion_u8; include/p3d_hip.h,
    "Distortion of frames under their 8-bit maps"): maps uint8 [n, H, W] (or [H, W]: one frame), ref and test uint8 [n, H, W, 3] in
    B, G, R order, cfg a distortion_cfg() (or (block, gate)) and a weight law int32 [256] (distortion_law) -> (table int64
    [n, P3D_DISTORTION_RECORD], block_sse int64 [n, Hb, Wb] or None).  The table holds integers alone -- squared errors, weighted
    squared errors, the weights' sum, largest differences and counts per plane B, G, R, Y, and SSIM's quantised window sums;
    distortion_report turns it into PSNR and SSIM.  block_map: whether the block map is made (default: when cfg's block is not 0).
    offset (0 .. 15): the test hook p3d_debug_distortion_u8, every device buffer between guards and the byte buffers shifted off a
    16-byte boundary."""
    from . import _lib
    s3, _, _ = _reframe_shape(sal, 1)
    n, H, W = s3.shape
    r, t = _distortion_frames(ref, (n, H, W, 3), "reference"), _distortion_frames(test, (n, H, W, 3), "test")
    w = _distortion_law_array(law)
    cfg, B = _distortion_cfg(cfg)
    table = np.empty((n, _lib.P3D_DISTORTION_RECORD), np.int64)
    want_map = B != 0 if block_map is None else bool(block_map)
    bs = np.empty((n, -(-H // B), -(-W // B)) if B in QPMAP_BLOCKS else (1,), np.int64) if want_map else None
    u8 = _lib._u8p
    head = (device, s3.ctypes.data_as(u8), r.ctypes.data_as(u8), t.ctypes.data_as(u8), n, H, W, cfg, w.ctypes.data_as(_lib._i32p))
    tail = (table.ctypes.data_as(_lib._i64p), None if bs is None else bs.ctypes.data_as(_lib._i64p))
    if offset is None:
        check(lib().p3d_distortion_u8(*head, *tail))
    else:
        check(lib().p3d_debug_distortion_u8(*head, int(offset), *tail))
    return table, bs


def distortion_report(table, pixels):
    """The float64 figures of a distortion table (int64 [n, P3D_DISTORTION_RECORD], or one record) of frames of `pixels` = H * W
    pixels -> dict of float64 arrays: psnr [n, 4] = 10 log10(255^2 pixels / SSE) and wpsnr [n, 4] = 10 log10(255^2 SW / WSSE) per plane
    B, G, R, Y; ssim [n] = SQ / (65536 NW) and wssim [n] = SWQ / (65536 SWW); changed_salient_share [n] = CHANGED_SALIENT /
    SALIENT.  An SSE (or WSSE) of 0 gives +inf; a denominator of 0 (no weight, no window, no salient pixel) gives NaN.  A handful of
    float64 operations on the device's integers, on the host."""
    from . import _lib
    K = _lib.K
    t = np.asarray(table)
    if t.dtype != np.int64 or t.ndim not in (1, 2) or t.shape[-1] != K["P3D_DISTORTION_RECORD"]:
        raise ValueError("the table is int64 [n, %d]" % K["P3D_DISTORTION_RECORD"])
    t = t.reshape(-1, t.shape[-1]).astype(np.float64)          # exact: every entry is below 2^53
    sse, wsse = t[:, K["P3D_DISTORTION_SSE"]:][:, :4], t[:, K["P3D_DISTORTION_WSSE"]:][:, :4]
    sw = t[:, K["P3D_DISTORTION_SW"]][:, None]
    peak = 255. * 255.

    def db(count, err):
        with np.errstate(divide="ignore", invalid="ignore"):
            out = 10. * np.log10(peak * count / err)
        return np.where(count > 0, out, np.nan)          # (0 / 0 is NaN already; count = 0 with an error cannot happen)

    def ratio(num, den):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(den > 0, num / den, np.nan)
    return dict(psnr=db(np.full_like(sse, float(pixels)), sse), wpsnr=db(np.broadcast_to(sw, wsse.shape), wsse),
                ssim=ratio(t[:, K["P3D_DISTORTION_SQ"]], 65536. * t[:, K["P3D_DISTORTION_NW"]]),
                wssim=ratio(t[:, K["P3D_DISTORTION_SWQ"]], 65536. * t[:, K["P3D_DISTORTION_SWW"]]),
                changed_salient_share=ratio(t[:, K["P3D_DISTORTION_CHANGED_SALIENT"]], t[:, K["P3D_DISTORTION_SALIENT"]]))


def _shot_frames(frames):
    f = np.ascontiguousarray(frames)
    if f.dtype != np.uint8 or f.ndim != 4 or f.shape[3] != 3 or f.size == 0:
        raise ValueError("frames are non-empty uint8 [n, H, W, 3] in B, G, R order")
    return f


def shots_cfg(grid=(2, 2), threshold=250, window=2, ratio=512, min_length=3):
    """The six ints of include/p3d_hip.h's CONFIG ("Shot boundaries of 8-bit frames") in the order of the P3D_SHOTS_* indices:
    grid = (gy, gx) cells, threshold in permille of 6 H W, window in frames, ratio in 1 / 256, min_length in frames."""
    from . import _lib
    gy, gx = (int(grid), int(grid)) if np.isscalar(grid) else (int(grid[0]), int(grid[1]))
    cfg = (C.c_int * 6)()
    for k, v in ((_lib.P3D_SHOTS_GRID_Y, gy), (_lib.P3D_SHOTS_GRID_X, gx), (_lib.P3D_SHOTS_THRESHOLD, threshold), (_lib.P3D_SHOTS_WINDOW, window),
                 (_lib.P3D_SHOTS_RATIO, ratio), (_lib.P3D_SHOTS_MIN_LENGTH, min_length)):
        cfg[k] = int(v)
    return cfg


def shot_distances(frames, grid=(2, 2), device=0, offset=None, ballot=0):
    """The cut signal of frames uint8 [n, H, W, 3] on the device (p3d_shot_distances_u8): D uint32 [n], D[0] = 0, D[f] the distance
    of frame f's gy x gx cell histograms from frame f - 1's.  offset (0 .. 15): the test hook p3d_debug_shot_distances_u8, every
    device buffer between guards, the frames shifted off a 16-byte boundary, counted with (ballot=1) or without ballot aggregation."""
    f = _shot_frames(frames)
    n, H, W, _ = f.shape
    gy, gx = (int(grid), int(grid)) if np.isscalar(grid) else (int(grid[0]), int(grid[1]))
    D = np.empty(n, np.uint32)
    u8, u32 = C.POINTER(C.c_ubyte), C.POINTER(C.c_uint32)
    if offset is None:
        check(lib().p3d_shot_distances_u8(device, f.ctypes.data_as(u8), n, H, W, gy, gx, D.ctypes.data_as(u32)))
    else:
        check(lib().p3d_debug_shot_distances_u8(device, f.ctypes.data_as(u8), n, H, W, gy, gx, int(offset), int(ballot), D.ctypes.data_as(u32)))
    return D


def shot_cuts(D, P, threshold=250, window=2, ratio=512, min_length=3, device=0):
    """The cut decision on the device (p3d_shot_cuts): D uint32 [F], P = H * W of the frames it came from -> starts int32
    [n_shots], strictly ascending from 0."""
    d = np.ascontiguousarray(D, np.uint32)
    if d.ndim != 1 or d.size == 0:
        raise ValueError("D is a non-empty vector")
    cfg = shots_cfg((1, 1), threshold, window, ratio, min_length)
    starts, count = np.empty(len(d), np.int32), C.c_int(0)
    check(lib().p3d_shot_cuts(device, d.ctypes.data_as(C.POINTER(C.c_uint32)), len(d), int(P), cfg, starts.ctypes.data_as(C.POINTER(C.c_int32)),
                              len(d), C.byref(count)))
    return starts[:count.value].copy()


def gradual_cfg(lag=12, high=250, dip=230, mono=768, mono_min=2):
    """The five ints of include/p3d_hip.h's CONFIG ("Gradual transitions") in the order of the P3D_GRADUAL_* indices: lag in frames
    (0: dissolves off), high in permille of 6 H W, dip and mono in 1 / 256, mono_min in frames (0: fades off)."""
    from . import _lib
    cfg = (C.c_int * 5)()
    for k, v in ((_lib.P3D_GRADUAL_LAG, lag), (_lib.P3D_GRADUAL_HIGH, high), (_lib.P3D_GRADUAL_DIP, dip), (_lib.P3D_GRADUAL_MONO, mono),
                 (_lib.P3D_GRADUAL_MONO_MIN, mono_min)):
        cfg[k] = int(v)
    return cfg


def shot_signals_u8(frames, grid=(2, 2), lag=12, device=0, offset=None):
    """The signals of gradual transitions of frames uint8 [n, H, W, 3] on the device (p3d_shot_signals_u8): (D, E, v), uint32, uint32
    and int64 [n] -- D as shot_distances, E[f] the distance of frame f's cell histograms from frame f - lag's (0 before frame lag),
    v[f] the spread of the frame's bins.  offset (0 .. 15): the test hook p3d_debug_shot_signals_u8, every device buffer between
    guards, the frames shifted off a 16-byte boundary."""
    f = _shot_frames(frames)
    n, H, W, _ = f.shape
    gy, gx = (int(grid), int(grid)) if np.isscalar(grid) else (int(grid[0]), int(grid[1]))
    D, E, v = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.int64)
    u8, u32, i64 = C.POINTER(C.c_ubyte), C.POINTER(C.c_uint32), C.POINTER(C.c_int64)
    out = (D.ctypes.data_as(u32), E.ctypes.data_as(u32), v.ctypes.data_as(i64))
    if offset is None:
        check(lib().p3d_shot_signals_u8(device, f.ctypes.data_as(u8), n, H, W, gy, gx, int(lag), *out))
    else:
        check(lib().p3d_debug_shot_signals_u8(device, f.ctypes.data_as(u8), n, H, W, gy, gx, int(lag), int(offset), *out))
    return D, E, v


def shot_transitions(D, E, v, P, threshold=250, window=2, ratio=512, min_length=3, lag=12, high=250, dip=230, mono=768, mono_min=2,
                     device=0, cap=None):
    """The decision of gradual transitions on the device (p3d_shot_transitions): D, E uint32 [F] and v int64 [F] of
    shot_signals_u8, P = H * W of their frames -> (starts, kinds, n_shots): int32 [min(cap, n_shots)] each, starts ascending from 0,
    kinds the P3D_SHOT_* of every shot; cap: the room given (all F by default)."""
    d, e = np.ascontiguousarray(D, np.uint32), np.ascontiguousarray(E, np.uint32)
    w = np.ascontiguousarray(v, np.int64)
    if d.ndim != 1 or d.size == 0 or e.shape != d.shape or w.shape != d.shape:
        raise ValueError("D, E and v are non-empty vectors of one length")
    cfg, gcfg = shots_cfg((1, 1), threshold, window, ratio, min_length), gradual_cfg(lag, high, dip, mono, mono_min)
    cap = len(d) if cap is None else int(cap)
    starts, kinds, count = np.empty(max(cap, 1), np.int32), np.empty(max(cap, 1), np.int32), C.c_int(0)
    u32, i32 = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    check(lib().p3d_shot_transitions(device, d.ctypes.data_as(u32), e.ctypes.data_as(u32), w.ctypes.data_as(C.POINTER(C.c_int64)), len(d), int(P),
                                     cfg, gcfg, starts.ctypes.data_as(i32), kinds.ctypes.data_as(i32), cap, C.byref(count)))
    k = min(cap, count.value)
    return starts[:k].copy(), kinds[:k].copy(), count.value


def transitions_plan(H, W, grid=(2, 2), n=1, lag=12):
    """Test hook (p3d_debug_transitions_plan, host only): dict(tables, scratch_bytes) of shot_signals_u8's launches for n frames."""
    gy, gx = (int(grid), int(grid)) if np.isscalar(grid) else (int(grid[0]), int(grid[1]))
    t, s = C.c_int(0), C.c_int64(0)
    check(lib().p3d_debug_transitions_plan(int(H), int(W), gy, gx, int(n), int(lag), C.byref(t), C.byref(s)))
    return dict(tables=t.value, scratch_bytes=s.value)


def transitions_time(frames, grid=(2, 2), lag=12, reps=20, device=0):
    """Measurement hook (p3d_debug_transitions_time): HIP-event ms of `reps` alternating rounds -> (cut_ms, signal_ms), float64
    [reps] each: the cut signal's launches and shot_signals_u8's on the same frames."""
    f = _shot_frames(frames)
    n, H, W, _ = f.shape
    gy, gx = (int(grid), int(grid)) if np.isscalar(grid) else (int(grid[0]), int(grid[1]))
    out = [np.empty(int(reps), np.float64) for _ in range(2)]
    dp = C.POINTER(C.c_double)
    check(lib().p3d_debug_transitions_time(device, f.ctypes.data_as(C.POINTER(C.c_ubyte)), n, H, W, gy, gx, int(lag), int(reps),
                                           *[o.ctypes.data_as(dp) for o in out]))
    return tuple(out)


def shot_window_starts(shot_starts, frames, stride=1, T=16):
    """The window starts of P3DSession.video_predict_shots that cover a video of `frames` frames under the table shot_starts
    (ascending from 0): per shot of L frames from lo, [lo] where L < T -- the one window a short shot takes -- else lo + 0, stride,
    2 stride, ... and a last one at L - T, so that every frame is covered; the shots' lists one after the other.  Host arithmetic."""
    st = [int(s) for s in shot_starts]
    F, stride, T = int(frames), int(stride), int(T)
    if not st or st[0] != 0 or any(b <= a for a, b in zip(st, st[1:])) or st[-1] >= F:
        raise ValueError("shot starts ascend strictly from 0 and stay below the %d frames" % F)
    if stride < 1 or T < 1:
        raise ValueError("stride and T are at least 1")
    out = []
    for lo, end in zip(st, st[1:] + [F]):
        L = end - lo
        if L < T:
            out.append(lo)
            continue
        offs = list(range(0, L - T + 1, stride))
        if offs[-1] != L - T:
            offs.append(L - T)
        out.extend(lo + o for o in offs)
    return out


def shots_plan(H, W, grid=(2, 2), n=1):
    """Test hook (p3d_debug_shots_plan, host only): dict(rows_per_block, blocks_per_frame, frames_per_chunk, scratch_bytes) of the cut
    signal's launches for n frames of H x W."""
    gy, gx = (int(grid), int(grid)) if np.isscalar(grid) else (int(grid[0]), int(grid[1]))
    r, b, c, s = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    check(lib().p3d_debug_shots_plan(int(H), int(W), gy, gx, int(n), C.byref(r), C.byref(b), C.byref(c), C.byref(s)))
    return dict(rows_per_block=r.value, blocks_per_frame=b.value, frames_per_chunk=c.value, scratch_bytes=s.value)


def shots_time(frames, grid=(2, 2), reps=20, device=0):
    """Measurement hook (p3d_debug_shots_time): HIP-event ms of `reps` alternating rounds -> (signal_ms, ballot_ms, copy_ms), float64
    [reps] each: the cut signal without and with ballot aggregation, and a device-to-device copy of the same bytes."""
    f = _shot_frames(frames)
    n, H, W, _ = f.shape
    gy, gx = (int(grid), int(grid)) if np.isscalar(grid) else (int(grid[0]), int(grid[1]))
    out = [np.empty(int(reps), np.float64) for _ in range(3)]
    dp = C.POINTER(C.c_double)
    check(lib().p3d_debug_shots_time(device, f.ctypes.data_as(C.POINTER(C.c_ubyte)), n, H, W, gy, gx, int(reps), *[o.ctypes.data_as(dp) for o in out]))
    return tuple(out)
