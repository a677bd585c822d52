"""Cases for the full-resolution evaluation on supplied maps (metrics.evaluate_maps / p3d_debug_eval_maps), shared by
tests/test_eval_maps_cpu.py (what the cases claim, no GPU) and tests/test_gpu_eval_maps.py (the kernels of metrics_full.hip
against the float64 oracle).  Every case is seeded; the arrays of a built case are read-only and shared.

Maps.  Independent random maps would give CC and NSS near 0, where a relative tolerance means nothing, so the ground truth
follows the saliency map s (uniform float32 in [0, 1), the scored map at the fixation maps' resolution):
    density byte = clip(rint(255 * (0.6 s + 0.4 u))), u uniform          (CC about 0.83, SIM about 0.86)
    fixations    = n_fix pixels drawn without replacement with probability ~ s + 0.05          (NSS about 0.5)

What each case is for (csrc/metrics_full.hip; SORT_TPB, LCAP and TPB are read from that file):
  batch        eight 96x80 maps in one call, n_fix 0, 1, 2, 1000, 2048, 4096, 4097, 5000: slot and counter offsets of a batch
               (sums of next_pow2(n_fix), + map index), full_sort with more than one element per thread (np2 > SORT_TPB) and
               its pad fill, full_pass_c on both sides of LCAP (thresholds and counters in LDS / in global memory)
  ties         s quantised to 16 levels, n_fix 5000 and 300, no jitter: equal thresholds, pixels equal to thresholds; the levels
               normalise to j/15, so AUC_Borji's thresholds k * 0.1 meet them on the >= edge.  ties_fine: step 0.03
  ties_jitter  the same maps with AUC_Judd's noise supplied
  blocks257    one 1025x1025 map, n_fix 6000: 257 blocks per map, the second trip (j = tid + TPB < nblk) of every fold over
               block partials.  Pass B's "fixations before my block" sum runs j < blockIdx.x <= 256 there: still one trip
  blocks258    one 1027x1027 map, n_fix 6000: 258 blocks, so block 257 takes the second trip of that sum (j = 256), which
               decides its compaction slots; blocks 256 and 257 both hold fixations
  odd          33x47 (n_pix a multiple of nothing, n_fix 2);  row: 1x300
  bytes        fixation bytes from {0, 1, 127, 128, 129, 254, 255} (fixated <=> byte >= 128), every density byte 0..255
  resize       a 24x20 source scored at 96x80;  strided: a 96x80 source as channel 0 of 3, the other channels NaN
  degenerate   every pixel fixated (1 / (n_pix - n_fix) is infinite: AUC_Judd NaN); a map with one NaN pixel (CC, SIM NaN)
"""
import collections
import functools
import os
import re

import numpy as np

from oracle import dataflow as odf
from oracle import evaluation as oev
from oracle import metrics as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# maps [n, h, w] or [n, h, w, c] float32 (channel 0 is scored), density uint8 [n, Hd, Wd], fixation uint8 [n, H, W],
# jitter float64 [n, H, W] or None, n_rep, step; then the case's name and its list of n_fix
Case = collections.namedtuple("Case", "maps density fixation jitter n_rep step name n_fix")

BATCH_N_FIX = (0, 1, 2, 1000, 2048, 4096, 4097, 5000)
FIX_ON = (128, 129, 254, 255)           # dataflow.py:239-241: fixated <=> byte / 255. > 0.5 <=> byte >= 128
FIX_OFF = (0, 1, 127)


def _match(pattern, src, what):
    m = re.search(pattern, src)
    if m is None:
        raise AssertionError("csrc/metrics_full.hip no longer states %s as r'%s': if the kernel file was only reformatted, update "
                             "this pattern; if the rule changed, size the cases of this module for the new one" % (what, pattern))
    return m


@functools.lru_cache(maxsize=None)
def kernel_constants():
    """SORT_TPB, LCAP, TPB and the pixels per block of p3d_full_blocks, as csrc/metrics_full.hip states them (read once)."""
    src = open(os.path.join(ROOT, "sap3d_tensorflow_amd", "csrc", "metrics_full.hip")).read()
    out = {k: int(_match(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % k, src, k).group(1)) for k in ("TPB", "SORT_TPB", "LCAP")}
    m = _match(r"int\s+p3d_full_blocks\(long long n_pix\)\s*\{\s*return \(int\)std::max<long long>\(1,\s*std::min<long long>\("
               r"\(n_pix \+ (\d+)\) / (\d+),\s*(\d+)\)\);\s*\}", src, "p3d_full_blocks' rule ceil(n_pix / 4096)")
    if int(m.group(1)) != int(m.group(2)) - 1:
        raise AssertionError("p3d_full_blocks no longer rounds up: (n_pix + %s) / %s" % (m.group(1), m.group(2)))
    out["BLOCK_PIX"], out["MAX_BLOCKS"] = int(m.group(2)), int(m.group(3))
    return out


def full_blocks(n_pix):
    """p3d_full_blocks: blocks per map."""
    k = kernel_constants()
    return max(1, min(-(-n_pix // k["BLOCK_PIX"]), k["MAX_BLOCKS"]))


def block_range(n_pix, block):
    """[i0, i1): the pixels of one map that block `block` of its full_blocks(n_pix) takes (block_range, metrics_full.hip)."""
    chunk = -(-n_pix // full_blocks(n_pix))
    return block * chunk, min(n_pix, (block + 1) * chunk)


def next_pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def reference_auc_judd_loop(s, f):
    """utils/metrics.py:69-85 literally (np.sum(S >= thresh) per threshold), jitter off, on float32 map s and fixation map f."""
    S = np.asarray(s, np.float32).ravel().astype(np.float64)
    F = np.asarray(f).ravel() > 0.5
    S_fix = S[F]; n_fix = len(S_fix); n_pixels = len(S)
    thresholds = sorted(S_fix, reverse=True)
    tp = np.zeros(len(thresholds) + 2); fp = np.zeros(len(thresholds) + 2)
    tp[-1] = 1; fp[-1] = 1
    for k, thresh in enumerate(thresholds):
        above_th = np.sum(S >= thresh)
        tp[k + 1] = (k + 1) / float(n_fix)
        fp[k + 1] = (above_th - k - 1) / float(n_pixels - n_fix)
    return (getattr(np, "trapezoid", None) or np.trapz)(tp, fp)


# ---- builders ---------------------------------------------------------------------------------------------------------
def _saliency(rng, shape, levels=None):
    s = rng.random(shape).astype(np.float32)
    if levels:
        s = (np.floor(s * levels) / levels).astype(np.float32)      # j / levels exactly; range-normalised: j / (levels - 1)
    return s


def _density(rng, s):
    u = rng.random(s.shape)
    return np.clip(np.rint(255.0 * (0.6 * s.astype(np.float64) + 0.4 * u)), 0, 255).astype(np.uint8)


def _fixated(rng, s, n_fix):
    """Flat indices of n_fix distinct pixels, probability ~ s + 0.05."""
    if n_fix == s.size:
        return np.arange(s.size)
    p = s.ravel().astype(np.float64) + 0.05
    return rng.choice(s.size, n_fix, replace=False, p=p / p.sum())


def _fixation(rng, s, n_fix):
    f = np.zeros(s.shape, np.uint8)
    f.reshape(-1)[_fixated(rng, s, n_fix)] = 255
    return f


def _stack(seed, shape, n_fixes, levels=None):
    rng = np.random.default_rng(seed)
    s = np.stack([_saliency(rng, shape, levels) for _ in n_fixes])
    d = np.stack([_density(rng, m) for m in s])
    f = np.stack([_fixation(rng, m, k) for m, k in zip(s, n_fixes)])
    return s, d, f


def _batch():
    s, d, f = _stack(101, (96, 80), BATCH_N_FIX)
    return s, d, f, None, 5, 0.1


def _ties(step=0.1, jitter=False):
    s, d, f = _stack(102, (96, 80), (5000, 300), levels=16)
    jit = np.random.RandomState(1102).rand(*s.shape) * 1e-7 if jitter else None       # AUC_Judd's random.rand(H, W) * 1e-7
    return s, d, f, jit, 5, step


def _blocks257():
    s, d, f = _stack(104, (1025, 1025), (6000,))
    return s, d, f, None, 5, 0.1


def _blocks258():
    s, d, f = _stack(114, (1027, 1027), (6000,))
    return s, d, f, None, 5, 0.1


def _odd():
    s, d, f = _stack(105, (33, 47), (2,))
    return s, d, f, None, 5, 0.1


def _row():
    s, d, f = _stack(115, (1, 300), (7,))
    return s, d, f, None, 5, 0.1


def _bytes():
    rng = np.random.default_rng(106)
    s = _saliency(rng, (96, 80))
    d = _density(rng, s)
    d.reshape(-1)[rng.permutation(s.size)[:256]] = np.arange(256, dtype=np.uint8)      # every byte value occurs
    on = np.zeros(s.size, bool)
    on[_fixated(rng, s, 700)] = True
    f = np.where(on, np.resize(FIX_ON, s.size), np.resize(FIX_OFF, s.size)).astype(np.uint8).reshape(s.shape)
    return s[None], d[None], f[None], None, 5, 0.1


def _resize():
    rng = np.random.default_rng(107)
    s = _saliency(rng, (24, 20))
    full = odf.resize_linear(s, 96, 80)             # what is scored: ground truth follows it
    return s[None], _density(rng, full)[None], _fixation(rng, full, 400)[None], None, 5, 0.1


def _strided():
    s, d, f = _stack(117, (96, 80), (400,))
    wide = np.full(s.shape + (3,), np.nan, np.float32)
    wide[..., 0] = s
    return wide, d, f, None, 5, 0.1


def _degenerate():
    s, d, f = _stack(108, (96, 80), (96 * 80, 500))
    s = s.copy()
    free = np.flatnonzero(f[1].ravel() == 0)
    s[1].reshape(-1)[free[len(free) // 2]] = np.nan             # one NaN pixel, not fixated
    return s, d, f, None, 5, 0.1


BUILDERS = collections.OrderedDict([
    ("batch", _batch), ("ties", _ties), ("ties_fine", functools.partial(_ties, step=0.03)),
    ("ties_jitter", functools.partial(_ties, jitter=True)), ("blocks257", _blocks257), ("blocks258", _blocks258), ("odd", _odd),
    ("row", _row), ("bytes", _bytes), ("resize", _resize), ("strided", _strided), ("degenerate", _degenerate)])
NAN_PIXEL = ("degenerate", 1)               # (case, map) with a NaN pixel: its AUC columns are not compared
ORACLE_SEED = 21
# NSS with every pixel fixated is the mean of all z-scores, 0 but for rounding, so no relative tolerance applies.  Either side
# sums n = 7680 differences x - mean of magnitude < 1 in float64, with a mean that carries up to n * 2^-53 relative error:
# |sum| <= n * (n * 2^-53 * 0.5 + n * 2^-53), divided by std (0.29) and n: < 5e-12 per side
NSS_ALL_FIXATED_ABS = 1e-11


@functools.lru_cache(maxsize=None)
def case(name):
    maps, dens, fix, jit, n_rep, step = BUILDERS[name]()
    for a in (maps, dens, fix, jit):
        if a is not None:
            a.setflags(write=False)
    n_fix = tuple(int(k) for k in np.count_nonzero(fix.reshape(len(fix), -1) >= 128, axis=1))
    return Case(maps, dens, fix, jit, n_rep, step, name, n_fix)


def scored(c):
    """[n, h, w]: the channel of c.maps that is scored."""
    return c.maps if c.maps.ndim == 3 else c.maps[..., 0]


def scored_size(c):
    return c.fixation.shape[1:]


def jitter_arg(c):
    return c.jitter if c.jitter is not None else False


@functools.lru_cache(maxsize=None)
def oracle_rows(name):
    """([n, 5] float64, numpy's generator state afterwards): oracle.evaluation.test_py_clip_metrics per map, in map order, drawing
    AUC_Borji's indices from RandomState(ORACLE_SEED) -- the stream evaluate_maps is given in the GPU test."""
    c = case(name)
    rng = np.random.RandomState(ORACLE_SEED)
    rows = []
    for b in range(len(c.maps)):
        args = (scored(c)[b], c.density[b], c.fixation[b])
        with np.errstate(all="ignore"):
            if (name, b) != NAN_PIXEL:
                rows.append(oev.test_py_clip_metrics(*args, jitter=c.jitter[b] if c.jitter is not None else False, n_rep=c.n_rep,
                                                     step_size=c.step, rng=rng))
                continue
            # a NaN in the map: the reference draws, then stops in AUC_Borji (np.r_[0:nan:step] raises), and the place of a NaN
            # among sorted thresholds is unspecified: only the columns that are defined, from the same functions
            H, W = scored_size(c)
            rng.randint(0, H * W, [c.n_fix[b], c.n_rep])
            pred = odf.resize_linear(args[0], H, W)
            dens = odf.resize_linear_u8(args[1], H, W) / 255.
            rows.append(np.array([om.CC(pred, dens), om.SIM(pred, dens), np.nan, np.nan, om.NSS(pred, args[2] / 255.)]))
    rows = np.stack(rows)
    rows.setflags(write=False)
    return rows, rng.get_state()
