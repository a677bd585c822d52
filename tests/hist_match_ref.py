"""The numpy replay of the histogram-matching law of include/p3d_hip.h (CDF, INTERP, MATCH), written out step by step: the bin
fix-ups, the integer running sum, searchsorted-right - 1 -- NOT as calls to np.histogram / np.interp, to which
tests/test_hist_match_cpu.py holds it bit for bit.  Everything is float64, one numpy operation per rounding."""
import numpy as np


def values(kind, shape, rng):
    """The input kinds of the tests, float32."""
    if kind == "uniform":
        return rng.random(shape).astype(np.float32)
    if kind == "normal":
        return rng.normal(0.0, 3.0, shape).astype(np.float32)
    if kind == "skewed":
        return (rng.random(shape) ** 8).astype(np.float32)
    if kind == "few":                                       # values exactly on bin edges: both fix-ups
        return (rng.integers(0, 5, shape) / 4).astype(np.float32)
    if kind == "three":                                     # as a target: long runs of equal cdf entries
        return rng.choice(np.array([0.1, 0.5, 0.9], np.float32), shape)
    if kind == "const":
        return np.full(shape, 0.37, np.float32)
    raise ValueError(kind)


KINDS = ("uniform", "normal", "skewed", "few", "const")
# (seed, nb) of edge_values whose maps take the "i += 1" fix-up, and the "i -= 1" one (tests/test_hist_match_cpu.py checks it)
EDGE_CASES = ((5, 7), (40, 100))


def edge_values(seed, nb):
    """float32 [1, L]: the float32 neighbours of the nb + 1 bin edges of a random range -- values a rounding away from an edge,
    where (int)((v - mn) * norm) lands a bin off and the law's two fix-ups decide."""
    rng = np.random.default_rng(seed)
    lo, span = np.float32(rng.normal()), np.float32(rng.random() * 3 + 0.1)
    lv = (lo + span * (np.arange(nb + 1, dtype=np.float64) / nb)).astype(np.float32)
    lv = np.concatenate([lv, np.nextafter(lv, np.float32(9)), np.nextafter(lv, np.float32(-9))])
    return lv[(lv >= lv[0]) & (lv <= lv[nb])][None]


def edges(mn, mx, nb):
    """mn, mx after the +-0.5 rule, the nb + 1 edges, norm."""
    mn, mx = np.float64(mn), np.float64(mx)
    if mn == mx:
        mn, mx = mn - 0.5, mx + 0.5
    step = (mx - mn) / nb
    edge = mn + np.arange(nb + 1, dtype=np.float64) * step
    edge[nb] = mx
    return mn, mx, edge, nb / (mx - mn)


def bins(v, nb):
    """CDF's bin of every value of the float64 array v (one map), and the edges."""
    mn, mx, edge, norm = edges(v.min(), v.max(), nb)
    i = ((v - mn) * norm).astype(np.int64)                  # (int): towards zero, and nothing here is negative
    i[i == nb] = nb - 1
    dec = v < edge[i]
    inc = ~dec & (v >= edge[i + 1]) & (i != nb - 1)
    return i - dec + inc, edge


def cumulative_distribution(a, nb=256):
    """CDF of one map (float32, or the float64 b / 255. of a density) -> (cdf, centre, count int64).  The counts and their
    running sum are integers: no order, no rounding."""
    v = np.asarray(a).astype(np.float64).ravel()
    i, edge = bins(v, nb)
    assert i.min() >= 0 and i.max() < nb
    count = np.bincount(i, minlength=nb).astype(np.int64)
    cdf = np.cumsum(count).astype(np.float64) / np.float64(v.size)
    return cdf, (edge[:-1] + edge[1:]) / 2.0, count


def interp(x, xp, fp):
    """INTERP over the table (xp, fp), xp non-decreasing."""
    x = np.asarray(x, np.float64)
    xp, fp = np.asarray(xp, np.float64), np.asarray(fp, np.float64)
    n = len(xp)
    j = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, n - 2)      # the largest j with xp[j] <= x (the ends: below)
    with np.errstate(all="ignore"):
        slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])
        out = slope * (x - xp[j]) + fp[j]
    out = np.where(x == xp[j], fp[j], out)
    out = np.where(x < xp[0], fp[0], out)
    return np.where(x >= xp[n - 1], fp[n - 1], out)


def match_hist(a, cdf_t, centre_t, nb=256):
    """MATCH of one float32 map against a target table -> float32, the map's shape."""
    a = np.asarray(a, np.float32)
    cdf_s, centre_s, _ = cumulative_distribution(a, nb)
    new = interp(cdf_s, cdf_t, centre_t)
    return interp(a.astype(np.float64), centre_s, new).astype(np.float32)


def match_hist_maps(maps, targets, nb=256):
    """Every map matched to the table of its own target (float32 images, or float64 densities) -> float32 [n, H, W]."""
    return np.stack([match_hist(m, *cumulative_distribution(t, nb)[:2], nb=nb) for m, t in zip(maps, targets)])


def match_table(maps, cdf_t, centre_t, nb=256):
    return np.stack([match_hist(m, cdf_t, centre_t, nb) for m in maps])
