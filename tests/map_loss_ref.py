"""Float64 restatement of the per-map saliency loss P3D_LOSS_KLD_CC (include/p3d_hip.h), map by map: its value and its
analytic gradient, for the CPU and GPU tests.  Test infrastructure, like reg_ref.py.

A map is one [H, W] frame; s is the predicted saliency (the stored pred, or sigmoid of a raw head's output), y the target.
    S = sum s, Y = sum y;  p = s / S if S > 0 else s;  q = y / Y if Y > 0 else y           (the reference's `if map.any()`)
    KL = sum q log(eps + q / (p + eps)), eps = 2.2204e-16                                (utils/metrics.py:338-361)
    CC = C / sqrt(A B) from the centred sums A = sum (s - sbar)^2, B = sum (y - ybar)^2, C = sum (s - sbar)(y - ybar);
         undefined (NaN, adds 0 to the loss and the gradient) when A = 0 or B = 0        (utils/metrics.py:227-250)
    L = sum over maps of w_kld KL + w_cc (1 - CC)
    g_i = -q_i^2 / ((p_i + eps)(eps (p_i + eps) + q_i));  dKL/ds_i = (g_i - sum_j g_j p_j) / S  (S > 0), else g_i
    dCC/ds_i = (y_i - ybar) / sqrt(A B) - CC (s_i - sbar) / A
    dL/ds_i = w_kld dKL/ds_i - w_cc dCC/ds_i;   dL/dlogits_i = dL/ds_i s_i (1 - s_i)."""
import numpy as np

EPS = 2.2204e-16


def sigmoid32(z):
    """1/(1+exp(-z)) in float32, as the heads form it (exactly 0 once exp(-z) overflows)."""
    z = np.asarray(z, np.float32)
    with np.errstate(over="ignore"):
        return (np.float32(1) / (np.float32(1) + np.exp(-z))).astype(np.float32)


def one_map(s, y, kld_weight=1.0, cc_weight=1.0):
    """One map (any shape; s and y float64).  Returns a dict: loss, kl, cc (NaN when undefined), the gradient dlds, and the
    magnitudes the GPU tests scale their bounds by (termmag: |dKL| and |dCC| parts per element; kl_mag: sum |q log(..)|)."""
    s = np.asarray(s, np.float64).ravel()
    y = np.asarray(y, np.float64).ravel()
    n = s.size
    S, Y = s.sum(), y.sum()
    p = s / S if S > 0 else s
    q = y / Y if Y > 0 else y
    kl_terms = q * np.log(EPS + q / (p + EPS))
    kl = float(kl_terms.sum())
    ds, dy = s - S / n, y - Y / n
    A, B, C = float((ds * ds).sum()), float((dy * dy).sum()), float((ds * dy).sum())
    defined = A > 0 and B > 0
    cc = C / (np.sqrt(A) * np.sqrt(B)) if defined else float("nan")
    pe = p + EPS
    g = -(q * q) / (pe * (EPS * pe + q))
    gp = float((g * p).sum())
    dkl = (g - gp) / S if S > 0 else g
    kl_mag = np.abs(g) + abs(gp) + np.abs(g * p).sum()
    kl_mag = kl_mag / S if S > 0 else kl_mag
    if defined:
        rab = 1.0 / (np.sqrt(A) * np.sqrt(B))
        dcc = dy * rab - cc * ds / A
        cc_mag = np.abs(dy) * rab + abs(cc) * np.abs(ds) / A
    else:
        dcc = np.zeros(n)
        cc_mag = np.zeros(n)
    loss = kld_weight * kl + (cc_weight * (1.0 - cc) if defined else 0.0)
    return dict(loss=loss, kl=kl, cc=cc, dlds=kld_weight * dkl - cc_weight * dcc, defined=defined,
                termmag=kld_weight * kl_mag + cc_weight * cc_mag, kl_mag=float(np.abs(kl_terms).sum()),
                S=S, Y=Y, A=A, B=B)


def map_loss(s, y, maps, kld_weight=1.0, cc_weight=1.0):
    """`maps` maps of s.size // maps elements each (s the float32 saliency, y the target).  Returns (loss, per_map [maps, 2]
    = KL, CC, dlogits (float64), per-map dicts of one_map)."""
    s32 = np.asarray(s, np.float32).reshape(maps, -1)
    y64 = np.asarray(y, np.float32).astype(np.float64).reshape(maps, -1)
    rows = [one_map(s32[m].astype(np.float64), y64[m], kld_weight, cc_weight) for m in range(maps)]
    s64 = s32.astype(np.float64)
    dl = np.stack([r["dlds"] for r in rows]) * (s64 * (1.0 - s64))
    per_map = np.array([[r["kl"], r["cc"]] for r in rows], np.float64).reshape(maps, 2)
    return float(sum(r["loss"] for r in rows)), per_map, dl.ravel(), rows


def loss_of_s(s, y, maps, kld_weight=1.0, cc_weight=1.0):
    """The float64 loss alone, as a function of s (float64) -- for finite differences."""
    s = np.asarray(s, np.float64).reshape(maps, -1)
    y = np.asarray(y, np.float64).reshape(maps, -1)
    return float(sum(one_map(s[m], y[m], kld_weight, cc_weight)["loss"] for m in range(maps)))
