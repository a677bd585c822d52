"""The reference's validation metrics (utils/metrics.py) on the GPU: same names, same argument meaning, computed by
libp3dhip (csrc/metrics.hip) in float64 on float32 maps.  `*_batch` variants take [n_maps, H, W] stacks -- one launch
for all the last-frame maps of a validation pass (train.py:249-260).  Maps must share one shape: the reference's
resize-to-match branch (skimage) is not reproduced and raises here."""
import ctypes as C

import numpy as np

from ._lib import check, lib


def _maps(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        raise ValueError("maps of different shape %s / %s: resize them first (the reference's skimage branch is not "
                         "part of this library)" % (a.shape, b.shape))
    if a.ndim < 2 or a.size == 0:
        raise ValueError("expected non-empty [H, W] or [n, H, W] maps")
    return a, b


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _two_map(fn, m1, m2, batched, device):
    a, b = _maps(m1, m2)
    n = a.shape[0] if batched else 1
    out = np.empty(n, np.float64)
    check(fn(device, _fp(a), _fp(b), n, a.size // n, _dp(out)))
    return out if batched else float(out[0])


def CC(saliency_map1, saliency_map2, device=0):
    """Pearson correlation of two maps (utils/metrics.py:227-250)."""
    return _two_map(lib().p3d_metric_cc, saliency_map1, saliency_map2, False, device)


def SIM(saliency_map1, saliency_map2, device=0):
    """Histogram intersection of two maps scaled to [0,1] and to sum 1 (utils/metrics.py:258-287)."""
    return _two_map(lib().p3d_metric_sim, saliency_map1, saliency_map2, False, device)


def NSS(saliency_map, fixation_map, device=0):
    """Mean standardised saliency at fixated pixels, fixation_map > 0.5 (utils/metrics.py:200-224)."""
    return _two_map(lib().p3d_metric_nss, saliency_map, np.asarray(fixation_map, dtype=np.float32), False, device)


def CC_batch(maps1, maps2, device=0):
    return _two_map(lib().p3d_metric_cc, maps1, maps2, True, device)


def SIM_batch(maps1, maps2, device=0):
    return _two_map(lib().p3d_metric_sim, maps1, maps2, True, device)


def NSS_batch(saliency_maps, fixation_maps, device=0):
    return _two_map(lib().p3d_metric_nss, saliency_maps, np.asarray(fixation_maps, dtype=np.float32), True, device)


def KLdiv(saliency_map, fixation_map, device=0):
    """KL divergence of the density `fixation_map` from `saliency_map`, each scaled to sum 1 (utils/metrics.py:338-362 with its
    resize taken as the identity; float64, eps = 2.2204e-16 -- include/p3d_hip.h, KLDIV)."""
    return _two_map(lib().p3d_metric_kldiv, saliency_map, fixation_map, False, device)


def KLdiv_batch(saliency_maps, density_maps, device=0):
    return _two_map(lib().p3d_metric_kldiv, saliency_maps, density_maps, True, device)


def _info_gain(sal, fix, baseline, batched, device):
    a, b = _maps(sal, np.asarray(fix, dtype=np.float32))
    n = a.shape[0] if batched else 1
    base = np.ascontiguousarray(baseline, dtype=np.float32)
    if base.shape != a.shape[-2:] and base.shape != (a.size // n,):
        raise ValueError("the baseline is one map of the maps' shape %s, not %s" % (a.shape[-2:], base.shape))
    out = np.empty(n, np.float64)
    check(lib().p3d_metric_info_gain(device, _fp(a), _fp(b), _fp(base), n, a.size // n, _dp(out)))
    return out if batched else float(out[0])


def InfoGain(saliency_map, fixation_map, baseline_map, device=0):
    """Information gain of `saliency_map` over `baseline_map` at the fixated pixels (fixation_map > 0.5), in bits: the MIT
    saliency benchmark's InfoGain (include/p3d_hip.h, INFO GAIN).  NaN when nothing is fixated or a map is constant."""
    return _info_gain(saliency_map, fixation_map, baseline_map, False, device)


def InfoGain_batch(saliency_maps, fixation_maps, baseline_map, device=0):
    """[n, H, W] maps against ONE baseline [H, W]."""
    return _info_gain(saliency_maps, fixation_maps, baseline_map, True, device)


def eval_extra_flags(extra):
    """P3D_EVAL_* flags of `extra`: a name ("kldiv", "info_gain") or a collection of names."""
    from ._lib import EVAL_EXTRA
    names = [extra] if isinstance(extra, str) else list(extra)
    flags = 0
    for k in names:
        if k not in EVAL_EXTRA:
            raise ValueError("extra metric %r: have %s" % (k, sorted(EVAL_EXTRA)))
        flags |= EVAL_EXTRA[k]
    return flags


def _judd(sal, fix, jitter, batched, device, rng):
    a, b = _maps(sal, np.asarray(fix, dtype=np.float32))
    n = a.shape[0] if batched else 1
    if jitter is True:          # the reference's default: saliency_map += random.rand(*shape) * 1e-7 (utils/metrics.py:62-63)
        jitter = (rng if rng is not None else np.random).random_sample(a.shape) * 1e-7
    jit = None
    if jitter is not None and jitter is not False:
        jit = np.ascontiguousarray(jitter, dtype=np.float32)
        if jit.shape != a.shape:
            raise ValueError("jitter must have the maps' shape")
    out = np.empty(n, np.float64)
    check(lib().p3d_metric_auc_judd(device, _fp(a), _fp(b), _fp(jit) if jit is not None else None, n, a.size // n, _dp(out)))
    return out if batched else float(out[0])


def AUC_Judd(saliency_map, fixation_map, jitter=True, device=0, rng=None):
    """Area under the ROC curve swept over the saliency values at fixated pixels (utils/metrics.py:25-85).  jitter: True
    (draw the reference's 1e-7 noise from numpy), False, or the noise array itself.  NaN when nothing is fixated."""
    return _judd(saliency_map, fixation_map, jitter, False, device, rng)


def AUC_Judd_batch(saliency_maps, fixation_maps, jitter=True, device=0, rng=None):
    return _judd(saliency_maps, fixation_maps, jitter, True, device, rng)


def AUC_Borji(saliency_map, fixation_map, n_rep=100, step_size=0.1, rand_sampler=None, device=0, rng=None, rand_idx=None):
    """utils/metrics.py:88-154.  The random pixel indices come from numpy exactly as in the reference
    (random.randint(0, n_pixels, [n_fix, n_rep]), :139) unless `rand_idx` supplies them; `rand_sampler` (the hook
    AUC_shuffled uses, :145) is not supported."""
    if rand_sampler is not None:
        raise NotImplementedError("rand_sampler (AUC_shuffled) is outside the ported path")
    a, b = _maps(saliency_map, np.asarray(fixation_map, dtype=np.float32))
    n_fix = int(np.count_nonzero(b > 0.5))
    if n_fix == 0:
        return float("nan")                 # 'no fixation to predict' (utils/metrics.py:122-124)
    if rand_idx is None:
        rand_idx = (rng if rng is not None else np.random).randint(0, a.size, [n_fix, n_rep])
    r = np.ascontiguousarray(rand_idx, dtype=np.int32)
    if r.shape != (n_fix, n_rep):
        raise ValueError("rand_idx must be [n_fix, n_rep] = [%d, %d]" % (n_fix, n_rep))
    out = np.empty(n_rep, np.float64)
    check(lib().p3d_metric_auc_borji(device, _fp(a), _fp(b), r.ctypes.data_as(C.POINTER(C.c_int)), a.size, n_fix, n_rep,
                                     float(step_size), _dp(out)))
    return float(np.mean(out))


def AUC_shuffled(saliency_map, fixation_map, other_map, n_rep=100, step_size=0.1, device=0, rng=None, other_idx=None):
    """utils/metrics.py:157-197: AUC_Borji with the random locations drawn from the fixations of OTHER images (other_map:
    the union of M other fixation maps, Borji's M = 10).  The draws restate the Python-2 code: for each of the n_rep splits
    in order, random.permutation(n_other)[:n_fix] (`map` is eager in Python 2), transposed to [min(n_fix, n_other), n_rep]
    rows; with fewer other fixations than n_fix the rows are shorter but the false-positive rate still divides by n_fix
    (:151-152); with none, no sample is drawn and the curve closes at (1, 1).  `other_idx` supplies the pixel indices instead.
    NaN (and no draw) when nothing is fixated."""
    other = np.asarray(other_map) > 0.5
    if other.shape != np.shape(fixation_map):
        raise ValueError("other_map.shape != fixation_map.shape")                            # :186-187
    a, b = _maps(saliency_map, np.asarray(fixation_map, dtype=np.float32))
    n_fix = int(np.count_nonzero(b > 0.5))
    if n_fix == 0:
        return float("nan")                 # AUC_Borji returns before it calls the sampler (:122-124)
    if other_idx is None:
        fixated = np.nonzero(other.ravel())[0]
        src = rng if rng is not None else np.random
        rows = [src.permutation(len(fixated))[:n_fix] for _ in range(n_rep)]                  # :190
        other_idx = fixated[np.asarray(rows, dtype=np.int64).reshape(n_rep, -1).T]            # :191
    r = np.ascontiguousarray(other_idx, dtype=np.int32).reshape(-1, n_rep)
    if r.shape[0] > n_fix:
        raise ValueError("other_idx has more than n_fix = %d rows" % n_fix)
    out = np.empty(n_rep, np.float64)
    check(lib().p3d_metric_auc_shuffled(device, _fp(a), _fp(b), r.ctypes.data_as(C.POINTER(C.c_int)), a.size, n_fix, r.shape[0],
                                        n_rep, float(step_size), _dp(out)))
    return float(np.mean(out))


def eval_draws(fixation, jitter, n_rep, rng=None):
    """The numpy draws of one test.py batch (test.py:166-176), shared by P3DSession.evaluate and evaluate_maps so that their
    order cannot drift apart.  fixation: uint8 [B, H, W].  Per map, in order: AUC_Judd's random.rand(H, W) * 1e-7 (jitter=True,
    utils/metrics.py:64-65), then AUC_Borji's random.randint(0, H*W, [n_fix, n_rep]) (:139); a map without fixation draws
    nothing (:56-59, :122-124).  jitter: True, False / None, or the noise itself (float64 [B, H, W]: no rand draw).
    -> (n_fix int32 [B], noise float64 [B, H, W] or None, the indices int32, concatenated)."""
    src = rng if rng is not None else np.random
    B, H, W = fixation.shape
    n_fix = np.count_nonzero(fixation.reshape(B, -1) >= 128, axis=1).astype(np.int32)        # / 255. > 0.5
    flag = jitter is None or np.isscalar(jitter)
    draw = flag and bool(jitter)
    if draw:
        jit = np.zeros((B, H, W), np.float64)
    elif flag:
        jit = None
    else:
        jit = np.ascontiguousarray(jitter, dtype=np.float64)
        if jit.shape != (B, H, W):
            raise ValueError("jitter must have the fixation maps' shape %s" % ((B, H, W),))
    idx = []
    for b in range(B):
        if n_fix[b] == 0:
            continue
        if draw:
            jit[b] = src.rand(H, W) * 1e-7
        idx.append(src.randint(0, H * W, [int(n_fix[b]), n_rep]).astype(np.int32).ravel())
    idx = np.ascontiguousarray(np.concatenate(idx) if idx else np.zeros(0, np.int32))
    return n_fix, jit, idx


def shuffled_draws(n_fix, n_other, n_rep, rng=None):
    """The numpy draws of shuffled AUC for one batch (include/p3d_hip.h, DRAW ORDER), the one place that makes them: per clip in
    clip order, nothing for a clip with n_fix = 0, else for each of the n_rep splits in order rng.permutation(n_other)[:n_fix]
    (utils/metrics.py:190), transposed to [min(n_fix, n_other), n_rep] (:191).
    -> (ranks int32, the clips' rows concatenated row-major; n_rows int32 [B])."""
    src = rng if rng is not None else np.random
    n_fix = np.asarray(n_fix, dtype=np.int64).ravel()
    n_other = np.asarray(n_other, dtype=np.int64).ravel()
    if n_fix.shape != n_other.shape:
        raise ValueError("one n_fix and one n_other per clip")
    ranks, n_rows = [], np.zeros(len(n_fix), np.int32)
    for b in range(len(n_fix)):
        if n_fix[b] == 0:
            continue
        rows = [src.permutation(int(n_other[b]))[:int(n_fix[b])] for _ in range(n_rep)]
        r = np.asarray(rows, dtype=np.int64).reshape(n_rep, -1).T
        n_rows[b] = r.shape[0]
        ranks.append(np.ascontiguousarray(r, dtype=np.int32).ravel())
    ranks = np.ascontiguousarray(np.concatenate(ranks) if ranks else np.zeros(0, np.int32))
    return ranks, n_rows


def evaluate_maps(maps, density, fixation, size=None, jitter=True, n_rep=100, step_size=0.1, rng=None, device=0, postprocess=None,
                  hist_match=None, nbins=256, extra=None, baseline=None, prior=None, prior_mode="off", prior_weight=0., shuffled=None):
    """Test hook (p3d_debug_eval_maps): P3DSession.evaluate's device pass on supplied maps instead of a session's prediction ->
    [n, 5] float64: CC, SIM, AUC_Judd, AUC_Borji, NSS.  maps: float32 [n, h, w], or [n, h, w, c] of which channel 0 is scored
    (the way the prediction buffer is addressed); density uint8 [n, Hd, Wd]; fixation uint8 [n, H, W] with (H, W) == size
    (default: the fixation maps' own).  The draws are evaluate's (eval_draws).  postprocess: dict(sigma, radius, norm) as
    P3DSession.set_postprocess takes them -- the smoothing / normalisation stage runs between the resize and the metrics
    (p3d_debug_eval_maps_post).  hist_match: "density" or a table (cdf, bin_centers) as P3DSession.set_hist_match takes them, with
    `nbins` -- the histogram-matching stage runs after the blur and before the normalisation (p3d_debug_eval_maps_match).
    extra: "kldiv", "info_gain" or both in a collection, as P3DSession.set_eval_extra's launch (p3d_debug_eval_maps_extra), with
    `baseline` float32 [H, W] for the information gain; the result is then (the [n, 5] array, [n, 2] float64: KL, IG -- NaN for
    the one that is off).  prior (float32 [H, W]), prior_mode and prior_weight: P3DSession.set_prior_stage's stage after the
    blur (p3d_debug_eval_maps_prior); baseline="prior" scores the information gain over that prior, copied on the device.  With
    a prior the result is always the pair.  shuffled: dict(pool=uint8 [capacity, H, W] fixation maps, others=int [n, M] slots of it,
    rng=..., n_rep=100, step_size=0.1[, n_other=...]) -- shuffled AUC of the clean scored map by the armed sequence
    (p3d_debug_eval_maps_shuffled; shuffled_draws draws from `rng` after n_other is known: given, or taken by
    dataflow.union_fixations); the result is then (out, xout, per_rep float64 [n, n_rep]), xout NaN where nothing is on."""
    m = np.ascontiguousarray(maps, dtype=np.float32)
    dens = np.ascontiguousarray(density)
    fix = np.ascontiguousarray(fixation)
    if m.ndim not in (3, 4) or m.size == 0:
        raise ValueError("expected non-empty [n, h, w] or [n, h, w, c] maps")
    if dens.dtype != np.uint8 or fix.dtype != np.uint8:
        raise ValueError("density and fixation maps are uint8 images (cv2.IMREAD_GRAYSCALE)")
    n = m.shape[0]
    if dens.ndim != 3 or dens.shape[0] != n or fix.ndim != 3 or fix.shape[0] != n:
        raise ValueError("expected %d density / fixation maps, [n, H, W]" % n)
    H, W = fix.shape[1:] if size is None else ((size, size) if np.isscalar(size) else tuple(size))
    if fix.shape[1:] != (H, W):
        raise ValueError("fixation maps are %s, not %s" % (fix.shape[1:], (H, W)))
    n_fix, jit, idx = eval_draws(fix, jitter, n_rep, rng)
    out = np.empty((n, 5), np.float64)
    u8 = C.POINTER(C.c_ubyte)
    ip = C.POINTER(C.c_int)
    args = (device, _fp(m), n, m.shape[1], m.shape[2], m.shape[3] if m.ndim == 4 else 1, dens.ctypes.data_as(u8),
            dens.shape[1], dens.shape[2], fix.ctypes.data_as(u8), int(H), int(W),
            _dp(jit) if jit is not None else None, idx.ctypes.data_as(ip), n_fix.ctypes.data_as(ip),
            int(n_rep), float(step_size), _dp(out))
    # the hooks are supersets of one another: a call takes the lowest rung that has every argument it was given
    from . import dataflow
    from .dataflow import _match_cfg, _post_cfg, _prior_mode
    rungs = ("", "_post", "_match", "_extra", "_prior", "_shuffled")
    level = (5 if shuffled is not None else 4 if prior is not None else 3 if extra is not None else 2 if hist_match is not None
             else 1 if postprocess is not None else 0)
    if level == 5:
        pool = np.ascontiguousarray(shuffled["pool"])
        if pool.dtype != np.uint8 or pool.ndim != 3 or pool.shape[1:] != (H, W):
            raise ValueError("the pool is uint8 [capacity, %d, %d]" % (H, W))
        ids = np.ascontiguousarray(shuffled["others"], dtype=np.int32)
        if ids.ndim != 2 or ids.shape[0] != n:
            raise ValueError("others is int [%d, M]" % n)
    flags = eval_extra_flags(extra) if extra is not None else 0
    g = None if prior is None else np.ascontiguousarray(prior, dtype=np.float32)
    if level == 4 and g.shape != (H, W):
        raise ValueError("the prior is %s, the fixation maps %s" % (g.shape, (H, W)))
    base = None
    if level == 4 and isinstance(baseline, str):
        if baseline != "prior":
            raise ValueError("baseline %r: a [H, W] map or 'prior'" % (baseline,))
    elif level >= 3 and baseline is not None:
        base = np.ascontiguousarray(baseline, dtype=np.float32)
        if level != 5 and base.shape != (H, W):         # (the shuffled rung leaves the shapes to the library)
            raise ValueError("the baseline is %s, the fixation maps %s" % (base.shape, (H, W)))
    post = postprocess or {}
    cfg = _post_cfg(post.get("sigma", 0.), post.get("radius", 0), post.get("norm", "none"))
    mc, keep = _match_cfg(hist_match if hist_match is not None else "off", nbins)
    xout = np.full((n, 2), np.nan, np.float64) if level >= 4 else np.empty((n, 2), np.float64)
    if level >= 1:
        args += (C.byref(cfg),)
    if level >= 2:
        args += (C.byref(mc),)
    if level >= 3:
        args += (flags, _fp(base) if base is not None else None, _dp(xout))
    if level >= 4:
        args += (_fp(g) if g is not None else None, _prior_mode(prior_mode, prior_weight), float(prior_weight))
    if level == 5:
        s_rep, s_step = int(shuffled.get("n_rep", 100)), float(shuffled.get("step_size", 0.1))
        n_other = shuffled.get("n_other")
        if n_other is None:
            n_other = dataflow.union_fixations(dataflow.pack_fixations(pool, device=device), (H, W), ids, device=device)[2]
        if "ranks" in shuffled:                 # (tests of the refusals: ranks of the caller's, nothing drawn)
            ranks, n_rows = (np.ascontiguousarray(v, dtype=np.int32) for v in (shuffled["ranks"], shuffled["n_rows"]))
        else:
            ranks, n_rows = shuffled_draws(n_fix, n_other, s_rep, shuffled.get("rng"))
        got_other, per_rep = np.empty(n, np.uint32), np.empty((n, s_rep), np.float64)
        args += (pool.ctypes.data_as(u8), pool.shape[0], ids.ctypes.data_as(ip), ids.shape[1], ranks.ctypes.data_as(ip),
                 n_rows.ctypes.data_as(ip), s_rep, s_step, got_other.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(per_rep))
    check(getattr(lib(), "p3d_debug_eval_maps" + rungs[level])(*args))
    return (out, xout, per_rep) if level == 5 else (out, xout) if level >= 3 else out


def score_flags(columns):
    """The flags of p3d_video_score / p3d_score_maps_u8 for column names of _lib.SCORE_COLUMNS ("matlab": cc, sim, judd), or an
    int that already is such a set."""
    from ._lib import SCORE_COLUMNS, SCORE_MATLAB
    if isinstance(columns, (int, np.integer)):
        return int(columns)
    if isinstance(columns, str):
        columns = (columns,)
    flags = 0
    for c in columns:
        for name in (SCORE_MATLAB if c == "matlab" else (c,)):
            if name not in SCORE_COLUMNS:
                raise ValueError("score column %r: have %s and 'matlab'" % (name, sorted(SCORE_COLUMNS)))
            flags |= SCORE_COLUMNS[name]
    return flags


def score_ties(ties):
    from ._lib import SCORE_TIES
    if ties not in SCORE_TIES:
        raise ValueError("ties %r: have %s" % (ties, sorted(SCORE_TIES)))
    return SCORE_TIES[ties]


def score_plan(n_pix, n=1, offset=0):
    """Test hook (p3d_debug_score_plan, host only): (blocks per map, pixels per block, most products a lane adds) of pass A."""
    b, c, k = C.c_int(0), C.c_int(0), C.c_int64(0)
    check(lib().p3d_debug_score_plan(int(n_pix), int(n), int(offset), C.byref(b), C.byref(c), C.byref(k)))
    return b.value, c.value, k.value


def score_bytes(sal, density, fixation, flags=("cc", "sim", "judd", "kl", "nss"), ties="expected", with_tables=False, device=0, offset=0):
    """8-bit saliency maps scored against 8-bit density and fixation maps (fixated: byte >= 128), all uint8 [n, H, W] or [H, W] of
    one shape -> float64 [n, 5]: CC, SIM, AUC_Judd, KL, NSS, an unselected column NaN (include/p3d_hip.h, "Scoring 8-bit maps";
    p3d_score_maps_u8).  ties: how AUC_Judd treats equal bytes, "reference" (utils/metrics.py with jitter=False) or "expected"
    (the mean over every order of the tied pixels).  fixation may be None when neither judd nor nss is selected.  with_tables
    (the test hook p3d_debug_score_u8, sources `offset` bytes past a 16-byte boundary): also dict(hs, hf, hd uint32 [n, 256],
    sd uint64 [n])."""
    s = np.ascontiguousarray(sal)
    d = np.ascontiguousarray(density)
    x = None if fixation is None else np.ascontiguousarray(fixation)
    for a in (s, d) + (() if x is None else (x,)):
        if a.dtype != np.uint8 or a.shape != s.shape:
            raise ValueError("saliency, density and fixation maps are uint8 arrays of one shape")
    if s.ndim not in (2, 3) or s.size == 0:
        raise ValueError("expected non-empty [H, W] or [n, H, W] maps")
    n = s.shape[0] if s.ndim == 3 else 1
    H, W = s.shape[-2:]
    u8 = C.POINTER(C.c_ubyte)
    out = np.empty((n, 5), np.float64)
    args = (device, s.ctypes.data_as(u8), d.ctypes.data_as(u8), None if x is None else x.ctypes.data_as(u8), n, int(H), int(W),
            score_flags(flags), score_ties(ties))
    if not with_tables:
        check(lib().p3d_score_maps_u8(*args, _dp(out)))
        return out
    t = dict(hs=np.empty((n, 256), np.uint32), hf=np.empty((n, 256), np.uint32), hd=np.empty((n, 256), np.uint32), sd=np.empty(n, np.uint64))
    u32 = C.POINTER(C.c_uint32)
    check(lib().p3d_debug_score_u8(*args, int(offset), t["hs"].ctypes.data_as(u32), t["hf"].ctypes.data_as(u32), t["hd"].ctypes.data_as(u32),
                                   t["sd"].ctypes.data_as(C.POINTER(C.c_uint64)), _dp(out)))
    return out, t


def borji_draws_u8(fixation, n_rep, rng=None):
    """AUC-Borji's draws for byte maps (the draw order of eval_draws without the jitter): fixation uint8 [n, H, W] or [H, W],
    fixated where the byte is >= 128; per map in map order, nothing for a map without fixation, else
    randint(0, H * W, [nf, n_rep]) (utils/metrics.py:139).  -> (idx int32, the maps' rows concatenated; nf int32 [n])."""
    src = rng if rng is not None else np.random
    f = np.asarray(fixation)
    f = f[None] if f.ndim == 2 else f
    nf = np.count_nonzero(f.reshape(f.shape[0], -1) >= 128, axis=1).astype(np.int32)
    n_pix = int(f.shape[1]) * int(f.shape[2])
    idx = [src.randint(0, n_pix, [int(k), int(n_rep)]).astype(np.int32).ravel() for k in nf if k]
    return np.ascontiguousarray(np.concatenate(idx) if idx else np.zeros(0, np.int32)), nf


def score_sweep(sal, fixation, idx, n_rows, step_size=0.1, device=0, with_tables=False, offset=0, n_rep=None):
    """AUC-Borji / shuffled AUC of 8-bit maps from supplied sample locations (include/p3d_hip.h, SPLIT SWEEP; p3d_score_sweep_u8):
    sal, fixation uint8 [n, H, W] or [H, W]; idx int32, map b's [n_rows[b], n_rep] pixel indices row-major, the maps concatenated;
    n_rows int [n], each at most the map's number of fixated pixels; n_rep: the splits, by default idx.size / sum(n_rows).  -> the per-split areas float64 [n, n_rep] (the score is
    np.mean over a row; NaN rows: no fixation, or a flat map).  with_tables (the test hook p3d_debug_score_sweep_u8, sources
    `offset` bytes past a 16-byte boundary): also dict(lev int32 [n, 256], top int32 [n, n_rep])."""
    s = np.ascontiguousarray(sal)
    x = np.ascontiguousarray(fixation)
    if s.dtype != np.uint8 or x.dtype != np.uint8 or s.shape != x.shape:
        raise ValueError("saliency and fixation maps are uint8 arrays of one shape")
    if s.ndim not in (2, 3) or s.size == 0:
        raise ValueError("expected non-empty [H, W] or [n, H, W] maps")
    n = s.shape[0] if s.ndim == 3 else 1
    H, W = s.shape[-2:]
    rows = np.ascontiguousarray(n_rows, dtype=np.int32).ravel()
    if rows.size != n:
        raise ValueError("one row count per map")
    r = np.ascontiguousarray(idx, dtype=np.int32).ravel()
    total = int(rows.astype(np.int64).sum())
    if n_rep is None:            # from idx: sum(n_rows) * n_rep indices; with no row at all, idx of shape [0, n_rep] still says it
        if total > 0 and r.size and r.size % total == 0:
            n_rep = r.size // total
        elif total == 0 and np.ndim(idx) == 2:
            n_rep = int(np.shape(idx)[1])
        else:
            raise ValueError("idx holds sum(n_rows) * n_rep indices")
    n_rep = int(n_rep)
    if r.size != total * n_rep:
        raise ValueError("idx holds sum(n_rows) * n_rep = %d indices, not %d" % (total * n_rep, r.size))
    ip, u8 = C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
    out = np.empty((n, n_rep), np.float64)
    args = (device, s.ctypes.data_as(u8), x.ctypes.data_as(u8), n, int(H), int(W), r.ctypes.data_as(ip) if total else None,
            rows.ctypes.data_as(ip), n_rep, float(step_size))
    if not with_tables:
        check(lib().p3d_score_sweep_u8(*args, _dp(out)))
        return out
    t = dict(lev=np.empty((n, 256), np.int32), top=np.empty((n, n_rep), np.int32))
    check(lib().p3d_debug_score_sweep_u8(*args, int(offset), t["lev"].ctypes.data_as(ip), t["top"].ctypes.data_as(ip), _dp(out)))
    return out, t
