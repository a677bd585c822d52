"""numpy replay of include/p3d_hip.h's SPLIT SWEEP (p3d_score_sweep_u8, p3d_video_score_auc; csrc/score_auc_u8.hip): AUC-Borji and
shuffled AUC of 8-bit maps from integer counts per byte level -- the tables, lev[256], every split's top byte and the area summed
in the header's order -- and the inputs shared by tests/test_score_auc_ref_cpu.py (the replay against oracle.metrics.AUC_Borji and
oracle.evaluation.AUC_shuffled, no GPU) and tests/test_gpu_score_auc.py (the kernels against the replay, bit for bit).

    python tests/score_auc_ref.py --write-gates      rewrites tests/golden/score_auc_gates.json with the worst observed difference
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

GATES = os.path.join(ROOT, "tests", "golden", "score_auc_gates.json")
# the replay against the oracle, per split: np.trapz sums the same non-negative terms in its own order; at most 1026 terms of three
# roundings each, the area <= 1: 1026 * 3 * 2^-53 = 3.4e-13
ORACLE_GATE = 1e-12
MAX_KMAX = 1024
NAN = float("nan")
SHAPES = ((3, 5), (7, 19), (16, 16), (64, 65), (263, 251))
STEPS = (0.1, 0.05, 0.3, 1.0 / 1024, 1.0)


def kmax_of(step):
    step = float(step)
    if not step > 0.0:
        raise ValueError("the step must be positive")
    k = int(math.ceil(1.0 / step))
    if k > MAX_KMAX:
        raise ValueError("the step gives more than %d thresholds" % MAX_KMAX)
    return k


def tables(s, x):
    """dict(hs, hf: int64 [256]; nf, lo, hi, maxfix) of one map; lo / hi / maxfix are -1 where nothing is counted."""
    s = np.asarray(s, np.uint8).ravel()
    f = np.asarray(x).ravel() >= 128
    hs = np.bincount(s, minlength=256).astype(np.int64)
    hf = np.bincount(s[f], minlength=256).astype(np.int64)
    occ, occf = np.nonzero(hs)[0], np.nonzero(hf)[0]
    return dict(hs=hs, hf=hf, nf=int(hf.sum()), lo=int(occ[0]), hi=int(occ[-1]), maxfix=int(occf[-1]) if len(occf) else -1)


def levels(t, step):
    """lev int32 [256]: the number of k < kmax with (double)k * step <= u_v; all 0 on a flat map (hi = lo), where nothing is swept."""
    kmax = kmax_of(step)
    lev = np.zeros(256, np.int32)
    if t["hi"] == t["lo"]:
        return lev
    tk = np.arange(kmax, dtype=np.float64) * np.float64(step)
    span = np.float64(t["hi"] - t["lo"])
    for v in range(256):
        u = np.float64(v - t["lo"]) / span
        lev[v] = int(np.count_nonzero(tk <= u))
    return lev


def sweep_split(t, lev, b, step):
    """One split: b the gathered bytes [n_rows] -> (top, area)."""
    step = float(step)
    b = np.asarray(b, np.int64).ravel()
    top = max(t["maxfix"], int(b.max())) if len(b) else t["maxfix"]
    if t["nf"] == 0 or t["hi"] == t["lo"]:
        return top, NAN
    nf = float(t["nf"])
    u_top = float(top - t["lo"]) / float(t["hi"] - t["lo"])
    K = 0 if u_top == 0.0 else int(math.ceil(u_top / step))
    lb = lev[b]
    px = py = area = 0.0
    for k in range(K - 1, -1, -1):
        ctp = int(t["hf"][lev > k].sum())
        cfp = int(np.count_nonzero(lb > k))
        x, y = float(cfp) / nf, float(ctp) / nf
        area += (x - px) * (y + py) * 0.5
        px, py = x, y
    area += (1.0 - px) * (1.0 + py) * 0.5
    return top, area


def sweep(s, x, idx, step=0.1):
    """One map: idx int [n_rows, n_rep] pixel indices -> dict(per_rep float64 [n_rep], top int32 [n_rep], lev int32 [256], nf)."""
    s = np.asarray(s, np.uint8)
    idx = np.asarray(idx, np.int64)
    t = tables(s, x)
    lev = levels(t, step)
    flat = s.ravel()
    n_rep = idx.shape[1]
    per, top = np.empty(n_rep, np.float64), np.empty(n_rep, np.int32)
    for rep in range(n_rep):
        top[rep], per[rep] = sweep_split(t, lev, flat[idx[:, rep]], step)
    return dict(per_rep=per, top=top, lev=lev, nf=t["nf"])


def sweep_maps(sal, fix, idx, n_rows, n_rep, step=0.1):
    """n maps; idx the maps' rows concatenated (row-major [n_rows[b], n_rep] each) -> dict(per_rep [n, n_rep], top [n, n_rep],
    lev [n, 256])."""
    idx = np.asarray(idx, np.int64).ravel()
    per, top, lev, at = [], [], [], 0
    for b in range(len(sal)):
        m = int(n_rows[b]) * n_rep
        r = sweep(sal[b], fix[b], idx[at:at + m].reshape(int(n_rows[b]), n_rep), step)
        at += m
        per.append(r["per_rep"]); top.append(r["top"]); lev.append(r["lev"])
    return dict(per_rep=np.stack(per), top=np.stack(top), lev=np.stack(lev))


def n_fix(fix):
    fix = np.asarray(fix)
    return np.count_nonzero(fix.reshape(fix.shape[0], -1) >= 128, axis=1).astype(np.int32)


def borji_draws(fix, n_rep, rng):
    """utils/metrics.py:139 per map with fixations, in map order -> (idx int32 concatenated, n_rows int32 [n] = nf)."""
    fix = np.asarray(fix)
    nf = n_fix(fix)
    N = fix[0].size
    idx = [rng.randint(0, N, [int(k), n_rep]).astype(np.int32).ravel() for k in nf if k]
    return np.ascontiguousarray(np.concatenate(idx) if idx else np.zeros(0, np.int32)), nf


# ---- the shared inputs ---------------------------------------------------------------------------------------------------------
def _blob(rng, H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    m = np.zeros((H, W))
    for _ in range(3):
        cy, cx, sg = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.08, 0.25) * max(H, W)
        m += rng.uniform(0.3, 1.0) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * sg * sg))
    m = np.clip(m / m.max() + 0.04 * rng.standard_normal((H, W)), 0.0, 1.0)
    return np.rint(255.0 * m ** 2).astype(np.uint8)


def _fix(rng, H, W, k):
    f = np.zeros(H * W, np.uint8)
    f[rng.choice(H * W, size=min(k, H * W), replace=False)] = 255
    return f.reshape(H, W)


CONTENTS = ("blobs", "multiples of 51", "two levels")


@functools.lru_cache(maxsize=None)
def case(H, W, content="blobs", n_fix_want=None, seed=0):
    """(sal, fix) uint8 [H, W] of one ordinary map."""
    rng = np.random.RandomState(7919 * H + 31 * W + 1009 * CONTENTS.index(content) + seed)
    N = H * W
    sal = _blob(rng, H, W)
    if content == "multiples of 51":                    # u_v lands exactly on thresholds of steps 0.1, 0.05, 1.0
        sal = (np.rint(sal / 51.0) * 51).astype(np.uint8)
        sal.ravel()[:2] = (0, 255)
    elif content == "two levels":
        sal = np.where(rng.rand(H, W) < 0.4, 200, 40).astype(np.uint8)
        sal.ravel()[:2] = (40, 200)
    fix = _fix(rng, H, W, n_fix_want if n_fix_want is not None else max(2, min(300, N // 5)))
    sal.setflags(write=False); fix.setflags(write=False)
    return sal, fix


def worst_against_oracle():
    """The largest per-split |replay - oracle| over the gate's cases, and how many there were."""
    from oracle import evaluation as oe
    from oracle import metrics as om
    worst, cases = 0.0, 0
    for H, W in SHAPES:
        for content in CONTENTS:
            sal, fix = case(H, W, content)
            N, nf = H * W, int(np.count_nonzero(fix >= 128))
            rng = np.random.RandomState(H * W + len(content))
            other = _fix(rng, H, W, max(1, nf // 2)) >= 128         # fewer other fixations than nf: shorter rows
            for step in STEPS:
                n_rep = 5
                idx = rng.randint(0, N, [nf, n_rep])
                _, want = om.AUC_Borji(sal.astype(np.float64), fix / 255.0, idx, step)
                got = sweep(sal, fix, idx, step)["per_rep"]
                worst = max(worst, float(np.abs(got - want).max()))
                cases += 1
                pool = np.nonzero(other.ravel())[0]
                for rows in (min(nf, len(pool)), 0):
                    ranks = np.stack([rng.permutation(len(pool))[:rows] for _ in range(n_rep)]).reshape(n_rep, -1).T
                    oidx = pool[ranks].reshape(rows, n_rep)
                    _, want = oe.AUC_shuffled(sal.astype(np.float64), fix / 255.0, other, n_rep, step, other_idx=oidx)
                    got = sweep(sal, fix, oidx, step)["per_rep"]
                    worst = max(worst, float(np.abs(got - want).max()))
                    cases += 1
    return worst, cases


def write_gates():
    worst, cases = worst_against_oracle()
    with open(GATES, "w") as f:
        json.dump({"what": "largest per-split absolute difference between tests/score_auc_ref.py's replay of the SPLIT SWEEP and "
                           "oracle.metrics.AUC_Borji / oracle.evaluation.AUC_shuffled over the cases of worst_against_oracle(); "
                           "gate %g" % ORACLE_GATE,
                   "oracle_gate": ORACLE_GATE, "cases": cases, "worst": worst}, f, indent=1, sort_keys=True)
        f.write("\n")
    return worst, cases


if __name__ == "__main__":
    print(json.dumps(write_gates() if "--write-gates" in sys.argv else worst_against_oracle()))
