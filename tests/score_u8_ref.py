"""numpy replay of include/p3d_hip.h's "Scoring 8-bit maps" (p3d_video_score, p3d_score_maps_u8; csrc/score_u8.hip), step by step:
the integer tables, the finals CC / NSS, AUC-Judd under both ties laws, the tables of pass B, and SIM and KL -- and the inputs
shared by tests/test_score_u8_cpu.py (what the replay claims, no GPU) and tests/test_gpu_score_u8.py (the kernels against it).
Everything that follows from the tables alone is replayed operation by operation, the EXPECTED-ties sum in the header's order.  The
header leaves the order of SIM's and KL's sums over the pixels to the kernels and the tests compare at relative 1e-9; `how` picks
the order in which THIS replay adds them ("np", "rev", "fsum", as tests/kl_ig_ref.py), so that the CPU test can show that the order
moves the results by less than 1e-11 on these inputs.

    python tests/score_u8_ref.py --write-gates      rewrites tests/golden/score_u8_gates.json with the observed spreads
"""
import functools
import itertools
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GATES = os.path.join(ROOT, "tests", "golden", "score_u8_gates.json")
EPS = 2.2204e-16            # utils/metrics.py:359, the literal
HOWS = ("np", "rev", "fsum")
ORDER_GATE = 1e-11          # the replay against the oracle, and its three orders among themselves
AUC_GATE = 1e-12            # AUC-Judd against the oracle's sweep / the exhaustive mean
FINAL_GATE = 1e-12          # the kernels' finals (from exact integers) against the replay
GPU_GATE = 1e-9             # the kernels' sums over pixels (SIM, KL) against the replay
CC, SIM, JUDD, KL, NSS = 1, 2, 4, 8, 16
ALL = 31
MATLAB = CC | SIM | JUDD
REFERENCE, EXPECTED = 0, 1
NAN = float("nan")


def total(x, how="np"):
    x = np.asarray(x, np.float64).ravel()
    if how == "np":
        return float(np.sum(x))
    if how == "rev":
        return float(np.sum(x[::-1]))
    if how == "fsum":
        return math.fsum(x.tolist()) if np.isfinite(x).all() else float(np.sum(x))
    raise ValueError(how)


def fixated(x):
    return np.asarray(x) >= 128


# ---- TABLES ------------------------------------------------------------------------------------------------------------------
def tables(s, d, x=None):
    """dict(hs, hf, hd: uint32 [256]; sd: Python int) of one map."""
    s = np.asarray(s, np.uint8).ravel()
    d = np.asarray(d, np.uint8).ravel()
    f = np.zeros(s.shape, bool) if x is None else fixated(x).ravel()
    return dict(hs=np.bincount(s, minlength=256).astype(np.uint32), hf=np.bincount(s[f], minlength=256).astype(np.uint32),
                hd=np.bincount(d, minlength=256).astype(np.uint32), sd=int(np.sum(s.astype(np.int64) * d.astype(np.int64))))


def moments(t):
    """N, S1, S2, D1, D2, nf, F1 as Python ints (exact)."""
    hs, hf, hd = ([int(c) for c in t[k]] for k in ("hs", "hf", "hd"))
    v = range(256)
    return dict(N=sum(hs), S1=sum(i * hs[i] for i in v), S2=sum(i * i * hs[i] for i in v), D1=sum(i * hd[i] for i in v),
                D2=sum(i * i * hd[i] for i in v), nf=sum(hf), F1=sum(i * hf[i] for i in v))


# ---- the finals ----------------------------------------------------------------------------------------------------------------
def cc(t):
    m = moments(t)
    vs, vd = m["N"] * m["S2"] - m["S1"] ** 2, m["N"] * m["D2"] - m["D1"] ** 2
    if vs == 0 or vd == 0:
        return NAN
    return float(m["N"] * t["sd"] - m["S1"] * m["D1"]) / (math.sqrt(float(vs)) * math.sqrt(float(vd)))


def nss(t):
    m = moments(t)
    vs = m["N"] * m["S2"] - m["S1"] ** 2
    if m["nf"] == 0 or vs == 0:
        return NAN
    return float(m["N"] * m["F1"] - m["nf"] * m["S1"]) / (float(m["nf"]) * math.sqrt(float(vs)))


def auc_reference_sweep(t):
    """The law as it is stated: utils/metrics.py:69-85's points from the tables, one by one, and the trapezoid sum in float64."""
    m = moments(t)
    N, nf = m["N"], m["nf"]
    if nf == 0 or nf == N:
        return NAN
    tp, fp = [0.0], [0.0]
    A = k = 0
    for v in range(255, -1, -1):
        A += int(t["hs"][v])
        for _ in range(int(t["hf"][v])):
            k += 1
            tp.append(k / float(nf))
            fp.append((A - k) / float(N - nf))
    tp.append(1.0)
    fp.append(1.0)
    tp, fp = np.array(tp), np.array(fp)
    return float(np.sum((fp[1:] - fp[:-1]) * (tp[1:] + tp[:-1]) / 2.0))


def auc_reference(t):
    """The closed form the kernel takes: I = sum_v hs[v] w_v - nf^2, the score (double)I / (double)(2 (N - nf) nf)."""
    m = moments(t)
    N, nf = m["N"], m["nf"]
    if nf == 0 or nf == N:
        return NAN
    G = total_i = 0
    for v in range(255, -1, -1):
        total_i += int(t["hs"][v]) * (2 * G + 1 if G < nf else 2 * nf)
        G += int(t["hf"][v])
    return float(total_i - nf * nf) / float(2 * (N - nf) * nf)


def butterfly_sum(terms):
    """T of the header: terms[0] = t_255 first; groups of 64 folded by x_i += x_{i xor o}, o = 32 .. 1, then ((w0 + w1) + w2) + w3."""
    x = np.asarray(terms, np.float64).reshape(4, 64).copy()
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[:, idx ^ o]
    return float(((x[0, 0] + x[1, 0]) + x[2, 0]) + x[3, 0])


def auc_expected(t):
    m = moments(t)
    N, nf = m["N"], m["nf"]
    if nf == 0 or nf == N:
        return NAN
    terms, G = [], 0
    n = float(nf)
    for v in range(255, -1, -1):
        hf, mv = int(t["hf"][v]), int(t["hs"][v]) - int(t["hf"][v])
        g, f = float(G), float(hf)
        if mv == 0:
            terms.append(0.0)
        elif G + hf < nf:
            terms.append(float(mv) * (((g + 0.5) + f / 2.0) / n))
        else:
            terms.append(float(mv) * ((((f * (g + 0.5)) / n + (f * (f - 1.0)) / (2.0 * n)) + 1.0) / (f + 1.0)))
        G += hf
    return butterfly_sum(terms) / float(N - nf)


def auc(t, ties):
    return auc_reference(t) if ties == REFERENCE else auc_expected(t)


# ---- the tables of pass B, SIM and KL --------------------------------------------------------------------------------------------
def _share_table(h):
    occ = np.nonzero(h)[0]
    mn, mx = int(occ[0]), int(occ[-1])
    with np.errstate(all="ignore"):
        u = (np.arange(256) - mn).astype(np.float64) / np.float64(mx - mn)
        U = np.float64(0.0)
        for v in occ:                                     # ascending, occupied bins only
            U = U + np.float64(int(h[v])) * u[v]
        return u / U


def pass_b_tables(t):
    """us, ud, ps, pd: float64 [256] each."""
    m = moments(t)
    v = np.arange(256, dtype=np.float64)
    ps = v / np.float64(m["S1"]) if m["S1"] else np.zeros(256)
    pd = v / np.float64(m["D1"]) if m["D1"] else np.zeros(256)
    return _share_table(t["hs"]), _share_table(t["hd"]), ps, pd


def sim(s, d, t, how="np"):
    us, ud, _, _ = pass_b_tables(t)
    return total(np.minimum(us[np.asarray(s).ravel()], ud[np.asarray(d).ravel()]), how)


def kl(s, d, t, how="np"):
    _, _, ps, pd = pass_b_tables(t)
    p, q = ps[np.asarray(s).ravel()], pd[np.asarray(d).ravel()]
    with np.errstate(all="ignore"):
        return total(q * np.log(EPS + q / (p + EPS)), how)


def score(s, d, x, flags=ALL, ties=EXPECTED, how="np"):
    """[5]: CC, SIM, AUC_Judd, KL, NSS of one map; an unselected column NaN."""
    t = tables(s, d, x)
    return np.array([cc(t) if flags & CC else NAN, sim(s, d, t, how) if flags & SIM else NAN, auc(t, ties) if flags & JUDD else NAN,
                     kl(s, d, t, how) if flags & KL else NAN, nss(t) if flags & NSS else NAN], np.float64)


def score_maps(sal, density, fixation, flags=ALL, ties=EXPECTED, how="np"):
    return np.stack([score(sal[i], density[i], None if fixation is None else fixation[i], flags, ties, how) for i in range(len(sal))])


def rel(a, b):
    if a == b:
        return 0.0
    return abs(a - b) / max(abs(a), abs(b))


# ---- the exhaustive law behind EXPECTED ties (small maps only) ---------------------------------------------------------------------
def judd_sweep_f64(S, F):
    """utils/metrics.py:69-85 in float64 on a map with pairwise distinct values."""
    S, F = np.asarray(S, np.float64).ravel(), np.asarray(F, bool).ravel()
    Sf = np.sort(S[F])[::-1]
    nf, N = len(Sf), len(S)
    tp, fp = np.zeros(nf + 2), np.zeros(nf + 2)
    tp[-1] = fp[-1] = 1.0
    for k, th in enumerate(Sf):
        above = int(np.sum(S >= th))
        tp[k + 1] = (k + 1) / float(nf)
        fp[k + 1] = (above - k - 1) / float(N - nf)
    return float(np.sum((fp[1:] - fp[:-1]) * (tp[1:] + tp[:-1]) / 2.0))


def auc_exhaustive(s, x):
    """The mean of the sweep over EVERY order of the pixels inside the tied levels: all permutations of the map's pixels, each
    adding distinct offsets below one grey level."""
    s = np.asarray(s, np.uint8).ravel()
    F = fixated(x).ravel()
    n = len(s)
    if n > 9:
        raise ValueError("exhaustive: at most 9 pixels")
    acc = []
    for perm in itertools.permutations(range(n)):
        acc.append(judd_sweep_f64(s.astype(np.float64) + np.array(perm, np.float64) / (2.0 * n), F))
    return math.fsum(acc) / len(acc)


# ---- the shared inputs ---------------------------------------------------------------------------------------------------------
def blobs(rng, n, H, W, noise=0.04):
    """uint8 [n, H, W]: a few Gaussian blobs plus noise, scaled to bytes -- skewed, as saliency and density maps are."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n, H, W), np.uint8)
    for i in range(n):
        m = np.zeros((H, W))
        for _ in range(3):
            cy, cx, sg = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.08, 0.25) * max(H, W)
            m += rng.uniform(0.3, 1.0) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * sg * sg))
        m = np.clip(m / m.max() + noise * rng.standard_normal((H, W)), 0.0, 1.0)
        out[i] = np.rint(255.0 * m ** 3)
    return out


def fixations(rng, like, n_fix):
    """uint8 [H, W]: n_fix pixels drawn with the map's values as weights, stored as 255, on a floor of 0."""
    w = like.astype(np.float64).ravel() + 1.0
    idx = rng.choice(w.size, size=min(n_fix, w.size), replace=False, p=w / w.sum())
    f = np.zeros(w.size, np.uint8)
    f[idx] = 255
    return f.reshape(like.shape)


SHAPES = ((3, 5), (7, 19), (16, 16), (64, 65), (263, 251))        # 263 x 251 = 66 013 pixels: three blocks of pass A


@functools.lru_cache(maxsize=None)
def case(H, W, n=5):
    """dict(sal, den, fix: uint8 [n, H, W]) of ordinary maps: blobs, and 3 .. N / 4 fixations drawn where the density is high."""
    rng = np.random.default_rng(1000 * H + W)
    sal, den = blobs(rng, n, H, W), blobs(rng, n, H, W, noise=0.01)
    fix = np.stack([fixations(rng, den[i], max(3, min(324, (H * W) // (4 + 3 * i)))) for i in range(n)])
    out = dict(sal=sal, den=den, fix=fix)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def edge_case(H, W):
    """The contents the kernels can go wrong on, one map each -> dict(sal, den, fix: uint8 [8, H, W], names)."""
    rng = np.random.default_rng(77 + H * W)
    N = H * W
    base = case(H, W, 1)
    ramp = (np.arange(N) % 256).astype(np.uint8).reshape(H, W)
    two = np.where(rng.random((H, W)) < 0.5, 0, 255).astype(np.uint8)
    fx = base["fix"][0]
    rows = [
        ("constant saliency", np.full((H, W), 37, np.uint8), base["den"][0], fx),
        ("arange % 256", ramp, ramp[::-1, ::-1].copy(), fx),
        ("only 0 and 255", two, np.where(rng.random((H, W)) < 0.3, 255, 0).astype(np.uint8), fx),
        ("no fixation", base["sal"][0], base["den"][0], np.zeros((H, W), np.uint8)),
        ("every pixel fixated", base["sal"][0], base["den"][0], np.full((H, W), 200, np.uint8)),
        ("fixation bytes 127 / 128", base["sal"][0], base["den"][0], np.where(rng.random((H, W)) < 0.5, 127, 128).astype(np.uint8)),
        ("all-zero saliency", np.zeros((H, W), np.uint8), base["den"][0], fx),
        ("all-zero density", base["sal"][0], np.zeros((H, W), np.uint8), fx),
    ]
    out = dict(sal=np.stack([r[1] for r in rows]), den=np.stack([r[2] for r in rows]), fix=np.stack([r[3] for r in rows]))
    for a in out.values():
        a.setflags(write=False)
    out["names"] = tuple(r[0] for r in rows)
    return out


def spreads():
    """{shape: {column: ...}}: the largest relative disagreement of SIM and KL between the three summation orders over a case."""
    out = {}
    for H, W in SHAPES:
        c = case(H, W)
        rows = [score_maps(c["sal"], c["den"], c["fix"], SIM | KL, EXPECTED, how) for how in HOWS]
        worst = {"sim": 0.0, "kl": 0.0}
        for name, j in (("sim", 1), ("kl", 3)):
            for b in range(len(c["sal"])):
                v = [r[b, j] for r in rows]
                worst[name] = max(worst[name], rel(v[0], v[1]), rel(v[0], v[2]), rel(v[1], v[2]))
        out["%dx%d" % (H, W)] = worst
    return out


if __name__ == "__main__":
    if "--write-gates" in sys.argv:
        seen = spreads()
        with open(GATES, "w") as f:
            json.dump({"what": "largest relative disagreement of SIM and KL between np.sum, reversed np.sum and math.fsum over the maps "
                               "of tests/score_u8_ref.py's cases; gate %g, the GPU tests' gate %g" % (ORDER_GATE, GPU_GATE),
                       "order_gate": ORDER_GATE, "gpu_gate": GPU_GATE, "spreads": seen}, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(spreads()))
