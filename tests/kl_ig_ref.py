"""numpy float64 replay of include/p3d_hip.h's KLDIV and INFO GAIN (p3d_set_eval_extra; full_pass_kl in csrc/metrics_full.hip),
step by step, and the inputs shared by tests/test_kl_ig_cpu.py (what the replay claims, no GPU) and tests/test_gpu_kl_ig.py (the
kernels against it).  The header leaves the order of the sums to the kernels and the tests compare at relative 1e-9; `how`
picks the order in which THIS replay adds ("np": np.sum's pairwise order, "rev": the same over the reversed array, "fsum": the
correctly rounded sum), so that the CPU test can show that the order moves the results by less than 1e-11 on these inputs.

    python tests/kl_ig_ref.py --write-gates      rewrites tests/golden/kl_ig_gates.json with the observed spreads
"""
import functools
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import dataflow as odf          # noqa: E402

import eval_maps_ref as R                   # noqa: E402

GATES = os.path.join(ROOT, "tests", "golden", "kl_ig_gates.json")
EPS = 2.2204e-16            # utils/metrics.py:359, the literal (np.finfo(float).eps is 2.220446049250313e-16)
HOWS = ("np", "rev", "fsum")
ORDER_GATE = 1e-11          # the three orders agree to this, two decades under ...
GPU_GATE = 1e-9             # ... the gate the kernels are held to (tests/test_gpu_eval.py's for CC and NSS)


def total(x, how="np"):
    x = np.asarray(x, np.float64).ravel()
    if how == "np":
        return float(np.sum(x))
    if how == "rev":
        return float(np.sum(x[::-1]))
    if how == "fsum":
        return math.fsum(x.tolist()) if np.isfinite(x).all() else float(np.sum(x))
    raise ValueError(how)


def density_f32(byte):
    """Evaluation's float32 density of resized bytes: float32(v / 255.) (mapf_density_kernel)."""
    return (np.asarray(byte, np.float64) / 255.0).astype(np.float32)


def density(q):
    """density() of csrc/metrics_full.hip on the float32 density q: rint(q * 255) / 255 in double, i.e. byte / 255.."""
    return np.rint(np.asarray(q, np.float32).astype(np.float64) * 255.0) / 255.0


def fixated_bytes(fix):
    return np.asarray(fix) >= 128               # / 255. > 0.5


def kldiv(s, y, how="np"):
    """KLDIV: s the float32 map, y the density in double (density(...) in evaluation, double(float32) at op level)."""
    s = np.asarray(s, np.float32).astype(np.float64).ravel()
    y = np.asarray(y, np.float64).ravel()
    S1, S2 = total(s, how), total(y, how)
    p = s / S1 if np.any(s != 0) else s
    q = y / S2 if np.any(y != 0) else y
    return total(q * np.log(EPS + q / (p + EPS)), how)


def _share(v, how):
    """P of the header: u = (v - min) / (max - min), P = u / U with U = (sum v - n * min) / (max - min)."""
    mn, mx = np.min(v), np.max(v)                         # np.min / np.max propagate NaN; numpy scalars: x / 0 is inf or NaN
    rng = mx - mn
    U = (np.float64(total(v, how)) - np.float64(v.size) * mn) / rng
    return (v - mn) / rng / U


def info_gain(s, fixated, b, how="np"):
    """INFO GAIN: s the float32 map, fixated a bool mask, b the float32 baseline."""
    s = np.asarray(s, np.float32).astype(np.float64).ravel()
    b = np.asarray(b, np.float32).astype(np.float64).ravel()
    f = np.asarray(fixated, bool).ravel()
    F = float(np.count_nonzero(f))
    P, B = _share(s, how), _share(b, how)
    terms = np.log2(EPS + P[f]) - np.log2(EPS + B[f])
    return float(np.float64(total(terms, how)) / np.float64(F))           # 0 / 0 = NaN: no fixation


def rel(a, b):
    return abs(a - b) / max(abs(a), abs(b))


# ---- the shared inputs ---------------------------------------------------------------------------------------------------
# (source h x w, scored H x W): 713 elements are one block with a ragged last stride; 4690 are two blocks by p3d_full_blocks
# (chunks of 2345: the second one ends on another stride than the first begins)
SHAPES = (((7, 9), (23, 31)), ((12, 11), (70, 67)))
ORDINARY, NO_FIX, CONSTANT, HAS_NAN = range(4)


def prior(H, W):
    """A centre prior: float32 [H, W], a Gaussian blob over a floor (visibly not the prediction)."""
    y, x = np.mgrid[0:H, 0:W]
    g = np.exp(-(((y - 0.45 * H) / (0.3 * H)) ** 2 + ((x - 0.55 * W) / (0.3 * W)) ** 2))
    return (0.1 + g).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(k, elem_stride=1):
    """Four maps of SHAPES[k] per call: an ordinary one, one without any fixation, a constant (all-zero) prediction, one holding
    a NaN.  -> dict(maps [4, h, w(, c)] float32, full [4, H, W] float32 (the scored maps: the oracle's float32 resize), density
    uint8 [4, Hd, Wd], dens_bytes uint8 [4, H, W] (its uint8 resize), fixation uint8 [4, H, W], baseline float32 [H, W])."""
    (h, w), (H, W) = SHAPES[k]
    rng = np.random.default_rng(700 + k)
    src = (0.05 + 0.95 * rng.random((4, h, w))).astype(np.float32)
    src[CONSTANT] = 0.0
    src[HAS_NAN, h // 2, w // 3] = np.nan
    full = np.stack([odf.resize_linear(m, H, W) for m in src]).astype(np.float32)
    dens = rng.integers(0, 256, size=(4, h + 4, w + 2), dtype=np.uint8)          # independent of the prediction: KL well above 0
    dens_bytes = np.stack([odf.resize_linear_u8(d, H, W) for d in dens])
    spread = np.where(np.isnan(full), 0.5, full)
    fix = np.stack([R._fixation(rng, spread[b], n) for b, n in ((0, 60), (1, 0), (2, 40), (3, 50))])
    fix[HAS_NAN][np.isnan(full[HAS_NAN])] = 0                                     # the NaN pixels themselves are not fixated
    maps = src
    if elem_stride > 1:
        maps = np.full(src.shape + (elem_stride,), np.nan, np.float32)            # channel 0 is scored, the others are poison
        maps[..., 0] = src
    out = dict(maps=maps, full=full, density=dens, dens_bytes=dens_bytes, fixation=fix, baseline=prior(H, W))
    for a in out.values():
        a.setflags(write=False)
    return out


def replay(c, how="np", full=None):
    """[4, 2]: KL, IG of a case by the law (full: other scored maps than the bare resize, e.g. post-processed ones)."""
    full = c["full"] if full is None else full
    rows = []
    with np.errstate(all="ignore"):
        for b in range(len(full)):
            y = density(density_f32(c["dens_bytes"][b]))
            rows.append([kldiv(full[b], y, how), info_gain(full[b], fixated_bytes(c["fixation"][b]), c["baseline"], how)])
    return np.array(rows, np.float64)


def expected_nan():
    """Where the law gives NaN: [4, 2] bool."""
    out = np.zeros((4, 2), bool)
    out[NO_FIX, 1] = out[CONSTANT, 1] = True
    out[HAS_NAN] = True
    return out


def spreads():
    """{case name: {"kl": ..., "ig": ...}}: the largest relative disagreement of the three summation orders over a case's maps."""
    out = {}
    for k in range(len(SHAPES)):
        c = case(k)
        rows = [replay(c, how) for how in HOWS]
        nan = expected_nan()
        worst = [0.0, 0.0]
        for b in range(4):
            for j in range(2):
                if nan[b, j]:
                    continue
                v = [r[b, j] for r in rows]
                worst[j] = max(worst[j], max(rel(v[0], v[1]), rel(v[0], v[2]), rel(v[1], v[2])))
        out["%dx%d" % SHAPES[k][1]] = {"kl": worst[0], "ig": worst[1]}
    return out


if __name__ == "__main__":
    if "--write-gates" in sys.argv:
        seen = spreads()
        with open(GATES, "w") as f:
            json.dump({"what": "largest relative disagreement of KL and IG between np.sum, reversed np.sum and math.fsum over the "
                               "maps of tests/kl_ig_ref.py's cases; gate %g, the GPU tests' gate %g" % (ORDER_GATE, GPU_GATE),
                       "order_gate": ORDER_GATE, "gpu_gate": GPU_GATE, "spreads": seen}, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(spreads()))
