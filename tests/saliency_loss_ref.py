"""Float64 restatement of the per-map saliency loss P3D_LOSS_SALIENCY (include/p3d_hip.h), map by map: its value and its
analytic gradient, for the CPU and GPU tests.  Test infrastructure, like map_loss_ref.py, which supplies KL and CC.

A map is one [H, W] frame of N elements; s the predicted saliency, y the target, f the fixation bytes (fixated <=> >= 128).
    L = sum over maps of w_kld KL + w_cc (1 - CC) + w_nss (-NSS) + w_sim (1 - SIM)
    NSS = (S_f / F - sbar) / sigma, sigma = sqrt(A / N), A = sum (s - sbar)^2, F the fixated count, S_f = sum_{fixated} s
          (utils/metrics.py:200-224); undefined (NaN, adds 0) when F = 0 or A = 0
    dNSS/ds_i = (f_i / F - 1 / N) / sigma - NSS (s_i - sbar) / A
    SIM = sum min(p', q'), u = (s - lo_s) / (hi_s - lo_s), U = sum u, p' = u / U, q' likewise from y
          (utils/metrics.py:258-287); undefined (NaN, adds 0) when hi_s = lo_s or hi_y = lo_y
    dSIM/ds_i = ([p'_i < q'_i] - sum_j [p'_j < q'_j] p'_j) / ((hi_s - lo_s) U), the range lo_s, hi_s held fixed
    dL/dlogits_i = dL/ds_i s_i (1 - s_i)."""
import numpy as np

import map_loss_ref as klcc

sigmoid32 = klcc.sigmoid32
THRESHOLD = 128


def nss_sim(s, y, f, rng_s=None):
    """NSS and SIM of one map with their gradients and the magnitudes the GPU bounds scale by.  rng_s = (lo_s, hi_s) freezes
    the range SIM normalises s by (for finite differences: the gradient holds it fixed)."""
    s = np.asarray(s, np.float64).ravel()
    y = np.asarray(y, np.float64).ravel()
    fx = np.asarray(f).ravel() >= THRESHOLD
    n = s.size
    S = s.sum()
    sbar = S / n
    ds = s - sbar
    A = float((ds * ds).sum())
    F = int(fx.sum())
    out = dict(F=F, A=A)
    # NSS
    out["nss_defined"] = F > 0 and A > 0
    if out["nss_defined"]:
        sigma = np.sqrt(A / n)
        Sf = float(s[fx].sum())
        nss = (Sf / F - sbar) / sigma
        out["nss"] = float(nss)
        out["dnss"] = (fx / F - 1.0 / n) / sigma - nss * ds / A
        # |terms| the value and the gradient are formed from: S_f / F and sbar before they cancel, over sigma
        out["nss_mag"] = float((abs(Sf) / F + abs(sbar)) / sigma)
        out["dnss_mag"] = (fx / F + 1.0 / n) / sigma + abs(nss) * np.abs(ds) / A
    else:
        out["nss"] = float("nan")
        out["dnss"] = np.zeros(n)
        out["nss_mag"] = 0.0
        out["dnss_mag"] = np.zeros(n)
    # SIM
    lo_s, hi_s = (float(s.min()), float(s.max())) if rng_s is None else rng_s
    lo_y, hi_y = float(y.min()), float(y.max())
    out["sim_defined"] = hi_s > lo_s and hi_y > lo_y
    out["range_s"] = (lo_s, hi_s)
    if out["sim_defined"]:
        u = (s - lo_s) / (hi_s - lo_s)
        w = (y - lo_y) / (hi_y - lo_y)
        U, W = u.sum(), w.sum()
        pp, qp = u / U, w / W
        below = pp < qp
        G = float(pp[below].sum())
        out["sim"] = float(np.minimum(pp, qp).sum())
        out["dsim"] = (below - G) / ((hi_s - lo_s) * U)
        out["pq"] = (pp, qp)
        # the kernel forms (hi - lo) U as S - N lo: a difference of sums of N terms, each within N eps64 of its magnitude
        out["amp_s"] = float((np.abs(s).sum() + n * abs(lo_s)) / ((hi_s - lo_s) * U))
        out["amp_y"] = float((np.abs(y).sum() + n * abs(lo_y)) / ((hi_y - lo_y) * W))
        out["dsim_mag"] = (below + G) / ((hi_s - lo_s) * U)
        out["Ds"] = float((hi_s - lo_s) * U)
    else:
        out["sim"] = float("nan")
        out["dsim"] = np.zeros(n)
        out["pq"] = None
        out["amp_s"] = out["amp_y"] = 0.0
        out["Ds"] = float("nan")
        out["dsim_mag"] = np.zeros(n)
    return out


def one_map(s, y, f, kld_weight=1.0, cc_weight=1.0, nss_weight=1.0, sim_weight=0.0, rng_s=None):
    """One map.  Returns map_loss_ref.one_map's dict under the four weights, plus nss, sim (NaN when undefined) and the parts
    of nss_sim."""
    r = klcc.one_map(s, y, kld_weight, cc_weight)
    e = nss_sim(s, y, f, rng_s)
    loss, dlds = r["loss"], r["dlds"]
    if nss_weight > 0 and e["nss_defined"]:
        loss = loss - nss_weight * e["nss"]
        dlds = dlds - nss_weight * e["dnss"]
    if sim_weight > 0 and e["sim_defined"]:
        loss = loss + sim_weight * (1.0 - e["sim"])
        dlds = dlds - sim_weight * e["dsim"]
    out = dict(r)
    out.update(e)
    out.update(loss=loss, dlds=dlds, klcc_loss=r["loss"], klcc_dlds=r["dlds"],
               termmag=r["termmag"] + nss_weight * e["dnss_mag"] + sim_weight * e["dsim_mag"])
    return out


def saliency_loss(s, y, f, maps, kld_weight=1.0, cc_weight=1.0, nss_weight=1.0, sim_weight=0.0):
    """`maps` maps of s.size // maps elements each (s the float32 saliency, y the float32 target, f the bytes).  Returns (loss,
    per_map [maps, 4] = KL, CC, NSS, SIM, dlogits (float64), per-map dicts of one_map)."""
    s32 = np.asarray(s, np.float32).reshape(maps, -1)
    y64 = np.asarray(y, np.float32).astype(np.float64).reshape(maps, -1)
    fb = np.asarray(f).reshape(maps, -1)
    rows = [one_map(s32[m].astype(np.float64), y64[m], fb[m], kld_weight, cc_weight, nss_weight, sim_weight) for m in range(maps)]
    s64 = s32.astype(np.float64)
    dl = np.stack([r["dlds"] for r in rows]) * (s64 * (1.0 - s64))
    per_map = np.array([[r["kl"], r["cc"], r["nss"], r["sim"]] for r in rows], np.float64).reshape(maps, 4)
    return float(sum(r["loss"] for r in rows)), per_map, dl.ravel(), rows


def loss_of_s(s, y, f, maps, weights, ranges):
    """The float64 loss alone as a function of s (float64), with every map's SIM range frozen at ranges[m] = (lo_s, hi_s) --
    for finite differences of the gradient the contract defines."""
    s = np.asarray(s, np.float64).reshape(maps, -1)
    y = np.asarray(y, np.float64).reshape(maps, -1)
    fb = np.asarray(f).reshape(maps, -1)
    return float(sum(one_map(s[m], y[m], fb[m], *weights, rng_s=ranges[m])["loss"] for m in range(maps)))
