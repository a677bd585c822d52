"""The laws of the fused-BatchNorm launches (csrc/conv_igemm2.hip, igemm_epilogue.h, conv_wgrad2.hip) in float64 numpy.

Independent of oracle/: tests/test_fused_bn_ref_cpu.py ties these laws to the oracle's tape, tests/test_gpu_fused_ops.py holds
the kernels to them.  All convs are SAME, stride 1 (the fused bottleneck convs), tensors [N, D, H, W, C], filters
[kd, kh, kw, Cin, Cout]."""
import numpy as np

EPS = 1e-3            # tf.layers.batch_normalization
MOVING_WEIGHT = 0.01  # 1 - momentum 0.99
FOLD_MAX = 32         # P3D_FOLD_MAX: more partials go through a finalize launch

f64 = lambda a: np.asarray(a, np.float64)


# ---- convs ---------------------------------------------------------------------------------------------------------------
def _taps(k):
    """(tap index triple, offset triple) of a SAME stride-1 conv: output o reads input o + offset."""
    pb = [(kk - 1) // 2 for kk in k]
    return [((a, b, c), (a - pb[0], b - pb[1], c - pb[2])) for a in range(k[0]) for b in range(k[1]) for c in range(k[2])]


def _shifted(x, off):
    """s[n, d, h, w] = x[n, d + off0, h + off1, w + off2], zero outside."""
    out = np.zeros_like(x)
    src, dst = [slice(None)], [slice(None)]
    for a in range(3):
        n, o = x.shape[1 + a], off[a]
        lo, hi = max(0, -o), min(n, n - o)
        if hi <= lo:
            return out
        dst.append(slice(lo, hi)); src.append(slice(lo + o, hi + o))
    out[tuple(dst)] = x[tuple(src)]
    return out


def conv(x, w):
    x, w = f64(x), f64(w)
    y = np.zeros(x.shape[:4] + (w.shape[4],))
    for t, off in _taps(w.shape[:3]):
        y += _shifted(x, off) @ w[t]
    return y


def conv_input_grad(dy, w):
    dy, w = f64(dy), f64(w)
    dx = np.zeros(dy.shape[:4] + (w.shape[3],))
    for t, off in _taps(w.shape[:3]):
        dx += _shifted(dy @ w[t].T, tuple(-o for o in off))
    return dx


def conv_filter_grad(x, dy, kshape):
    x, dy = f64(x), f64(dy)
    dw = np.zeros(tuple(kshape[:3]) + (x.shape[4], dy.shape[4]))
    for t, off in _taps(kshape):
        dw[t] = _shifted(x, off).reshape(-1, x.shape[4]).T @ dy.reshape(-1, dy.shape[4])
    return dw


# ---- forward fold ----------------------------------------------------------------------------------------------------------
def partials_of(y, bounds):
    """(sum, sum of squares) per channel over the row ranges bounds[i] .. bounds[i + 1] of y [M, C], rounded to float32 as a
    producer's epilogue leaves them: [nparts, C, 2]."""
    y = f64(y)
    return np.stack([np.stack([y[a:b].sum(0), (y[a:b] ** 2).sum(0)], -1) for a, b in zip(bounds[:-1], bounds[1:])]).astype(np.float32)


def fold(partials, M, gamma, beta):
    """mean, var (clamped at 0), inv, scale, shift from [nparts, C, 2] partials over M rows; `terms`: the sum of the magnitudes
    of the terms of each expression (the scale of its rounding error)."""
    p = f64(partials)
    s1, s2 = p[:, :, 0].sum(0), p[:, :, 1].sum(0)
    mean = s1 / M
    raw = s2 / M - mean * mean
    var = np.maximum(raw, 0.0)
    inv = 1.0 / np.sqrt(var + EPS)
    scale = f64(gamma) * inv
    shift = f64(beta) - mean * scale
    terms = {"mean": np.abs(mean), "invstd": np.abs(inv), "scale": np.abs(scale), "shift": np.abs(f64(beta)) + np.abs(mean * scale)}
    return {"mean": mean, "var": var, "raw_var": raw, "invstd": inv, "scale": scale, "shift": shift, "terms": terms}


def moving_update(moving, batch):
    return f64(moving) - (f64(moving) - f64(batch)) * MOVING_WEIGHT


# ---- operand transforms ----------------------------------------------------------------------------------------------------
def relu_operand(x, scale, shift, x2=None, scale2=None, shift2=None):
    """RELU1 / RELU2 (and xt = 1 / 2): relu(s1 x + t1) [+ relu(s2 x2 + t2)]; the conv pads the RESULT with zeros."""
    a = np.maximum(f64(scale) * f64(x) + f64(shift), 0.0)
    if x2 is not None:
        a = a + np.maximum(f64(scale2) * f64(x2) + f64(shift2), 0.0)
    return a


def grad_operand(g, y, k1, k2, k3):
    """GRAD (and dyt): k1 g + k2 y + k3; padding is zero."""
    return f64(k1) * f64(g) + f64(k2) * f64(y) + f64(k3)


# ---- gate and gradient fold ------------------------------------------------------------------------------------------------
def gate_mask(y, scale, shift):
    return f64(scale) * f64(y) + f64(shift) > 0


def gate(v, y, scale, shift):
    return np.where(gate_mask(y, scale, shift), f64(v), 0.0)


def gate_partials(g, y, mean, invstd, bm):
    """(sum g, sum g*xhat) per channel and per tile row of bm rows of g, y [M, C]: ([ntiles, C, 2], the sums of |term|)."""
    g, y = f64(g), f64(y)
    gx = g * (y - f64(mean)) * f64(invstd)
    n = -(-g.shape[0] // bm)
    sums = np.stack([np.stack([g[i * bm:(i + 1) * bm].sum(0), gx[i * bm:(i + 1) * bm].sum(0)], -1) for i in range(n)])
    mags = np.stack([np.stack([np.abs(g[i * bm:(i + 1) * bm]).sum(0), np.abs(gx[i * bm:(i + 1) * bm]).sum(0)], -1) for i in range(n)])
    return sums, mags


def grad_fold(partials, M, gamma, mean, invstd):
    p = f64(partials)
    sg, sgx = p[:, :, 0].sum(0), p[:, :, 1].sum(0)
    k1 = f64(gamma) * f64(invstd)
    k2 = -k1 * f64(invstd) * sgx / M
    k3 = -k1 * sg / M - k2 * f64(mean)
    terms = {"k1": np.abs(k1), "k2": np.abs(k2), "k3": np.abs(k1 * sg / M) + np.abs(k2 * f64(mean)), "dgamma": np.abs(sgx), "dbeta": np.abs(sg)}
    return {"k1": k1, "k2": k2, "k3": k3, "dgamma": sgx, "dbeta": sg, "terms": terms}


def half(a):
    """What the fp16 option makes of an operand fragment: rounded to float16 (round to nearest even), as float64."""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float64)
