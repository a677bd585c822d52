"""Plain numpy restatements of the self-attention block's kernels (utils/network.py:183-191; tests/test_gpu_attention.py):
softmax over rows forward and backward, the core  o = softmax(g f^T) h  with its four gradients, and the mixing
z = r * gamma + x  with the block's dropout given as a keep mask.

Every function takes `dtype`: float64 is the expected result, float32 the SAME formula as the noise yardstick -- a kernel passes
within 5 x the float32 restatement's own distance from float64 on the same inputs, plus a floor (rule(), below).  The builders
make the inputs of the score regimes the GPU tests run; tests/test_attention_ref_cpu.py establishes, without a GPU, that every
builder lands in its regime and that the gradients here are the gradients of the forward formulas."""
import numpy as np

f64 = np.float64
TILE = 32            # keys per tile of the kernels that keep the scores on chip (attention_flash.hip)
FLOOR = 2e-5         # tests/test_gpu_ops.py's tolerance: fp32 sums of up to a few thousand terms
FLOOR_DS = 1e-4      # dg, df: ds = p (dp - <p, dp>) cancels (tests/test_gpu_ops.py::test_attention_core_forward_and_grads)


# ---- the tolerance rule -------------------------------------------------------------------------------------------------------
def rel_err(got, want, scale=None):
    want = np.asarray(want, f64)
    scale = max(np.abs(want).max(), 1e-30) if scale is None else scale
    return float(np.abs(np.asarray(got, f64) - want).max() / scale)


def bound(want32, want64, floor, scale=None):
    """5 x the float32 restatement's distance from float64 + floor, relative to the result's maximum magnitude."""
    return 5.0 * rel_err(want32, want64, scale) + floor


def rule(got, want64, want32, floor=FLOOR, scale=None, what="", factor=1.0):
    err, lim = rel_err(got, want64, scale), factor * bound(want32, want64, floor, scale)
    print("%s err %.3e bound %.3e" % (what, err, lim))
    assert np.all(np.isfinite(np.asarray(got))), what
    assert err <= lim, (what, err, lim)
    return err, lim


# ---- softmax rows -------------------------------------------------------------------------------------------------------------
def softmax_rows(s, dtype=f64):
    s = np.asarray(s, dtype)
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True, dtype=dtype)


def softmax_rows_bwd(beta, dbeta, dtype=f64):
    """ds = beta (dbeta - <beta, dbeta>), utils/network.py:184 differentiated."""
    b, d = np.asarray(beta, dtype), np.asarray(dbeta, dtype)
    return b * (d - (b * d).sum(-1, keepdims=True, dtype=dtype))


SOFTMAX_REGIMES = [(kind, off) for off in (0.0, 1e4, -1e4) for kind in ("normal", "flat", "onehot")]


def softmax_input(rng, rows, cols, rotate=0):
    """[rows, cols] float32 scores; row i is of regime SOFTMAX_REGIMES[(i + rotate) % 9]: normal scores, a flat row, or a row whose
    spread is 200 (one score 200 above the others), each plain and with +1e4 / -1e4 added IN FLOAT32 (the expected result is
    computed from these float32 values).  Returns (scores, regime index per row)."""
    s = (rng.standard_normal((rows, cols)) * 2).astype(np.float32)
    which = (np.arange(rows) + rotate) % len(SOFTMAX_REGIMES)
    for i in range(rows):
        kind, off = SOFTMAX_REGIMES[which[i]]
        if kind == "flat":
            s[i] = np.float32(0.37)
        elif kind == "onehot":
            s[i, int(rng.integers(cols))] += np.float32(200.0)
        s[i] = s[i] + np.float32(off)
    return s, which


# ---- the core -----------------------------------------------------------------------------------------------------------------
def scores(g, f, dtype=f64):
    return np.asarray(g, dtype) @ np.asarray(f, dtype).transpose(0, 2, 1)


def core(g, f, h, d_o=None, dtype=f64):
    """o = softmax(g f^T) h for g [B, Ng, ci], f [B, Nf, ci], h [B, Nf, ch]; with d_o also (dg, df, dh)."""
    g, f, h = (np.asarray(a, dtype) for a in (g, f, h))
    p = softmax_rows(scores(g, f, dtype), dtype)
    o = p @ h
    if d_o is None:
        return o
    d = np.asarray(d_o, dtype)
    ds = softmax_rows_bwd(p, d @ h.transpose(0, 2, 1), dtype)
    return o, ds @ f, ds.transpose(0, 2, 1) @ g, p.transpose(0, 2, 1) @ d


def core_scales(g, f, h, d_o):
    """What the errors of (o, dg, df, dh) are relative to: the expected result's maximum magnitude.  Where dg or df is zero
    throughout (one key: the map is 1 and its gradient vanishes; g = 0: df = ds^T g) that magnitude says nothing about the
    sums that cancel to it, and the scale is the maximum of the same product without the cancellation, (p |dp|) |f| and
    (p |dp|)^T |g| -- what the 1e-4 floor of dg and df is about (an fp32 rounding of dp is 1e-7 of |dp|, not of the difference)."""
    g, f, h, d = (np.asarray(a, f64) for a in (g, f, h, d_o))
    want = core(g, f, h, d)
    p = softmax_rows(scores(g, f))
    raw = p * np.abs(d @ h.transpose(0, 2, 1))
    alt = (None, raw @ np.abs(f), raw.transpose(0, 2, 1) @ np.abs(g), None)
    out = []
    for w, a in zip(want, alt):
        m = np.abs(w).max()
        out.append(max(m if m > 0 or a is None else np.abs(a).max(), 1e-30))
    return out


CORE_REGIMES = ["units", "flat", "rising", "falling", "offset"]


def core_input(regime, B, ng, nf, ch, seed=0):
    """(g, f, h, d_o) float32 of one score regime:
    units    scores of a few units: the map is neither flat nor one-hot;
    flat     g = 0: every map row is 1 / nf and o the mean of h's rows;
    rising   steep, keys ordered so that a query's maximum rises in every tile of 32 keys: the running maximum of the kernels that
             keep the scores on chip moves, and the accumulator is rescaled, on every tile;
    falling  the same keys reversed: the first tile holds every row's maximum, no later tile rescales;
    offset   `units` with one channel pair set to g[..., 0] = f[..., 0] = 10: every score carries a common offset of 100."""
    rng = np.random.default_rng([seed, B, ng, nf, ch, CORE_REGIMES.index(regime)])
    ci = ch // 8
    rnd = lambda *s: rng.standard_normal(s).astype(np.float32)
    amp = np.float32((2.0 / np.sqrt(ci)) ** 0.5)
    g, f = rnd(B, ng, ci) * amp, rnd(B, nf, ci) * amp * 2
    h, d_o = rnd(B, nf, ch), rnd(B, ng, ch)
    if regime == "flat":
        g[:] = 0
    elif regime in ("rising", "falling"):
        # channel 0 carries a ramp over the keys, half a unit per key and 16 per tile; the other channels add about 0.04
        g *= np.float32(0.1)
        f *= np.float32(0.1)
        ramp = np.arange(nf, dtype=np.float32) * np.float32(0.5)
        g[..., 0] = 1
        f[..., 0] = ramp if regime == "rising" else ramp[::-1]
    elif regime == "offset":
        g[..., 0] = 10
        f[..., 0] = 10
    return g, f, h, d_o


# (B, ng, nf, ch) of tests/test_gpu_attention.py; every regime of every case is established in tests/test_attention_ref_cpu.py
CORE_CASES = [
    (2, 300, 77, 32),        # ATTN_CASES of tests/test_gpu_ops.py
    (1, 129, 33, 64),
    (2, 128, 64, 128),
    (1, 50, 200, 256),
    (3, 5, 3, 32),
    (2, 49, 49, 256),        # the 1x7x7 site (x_4_0 at 16x112x112): 49 keys, padded to 52
    (2, 40, 6, 32),          # 6 keys, padded to 8
    (2, 37, 1, 64),          # one key: the map is 1
    (2, 1, 70, 128),         # one query
    (1, 130, 4101, 32),      # more than 4096 keys: the softmax re-reads its rows
    (1, 8, 1024, 32),        # few queries over many keys: the beta h product is K-sliced
]
STORED_ONLY_CASES = [(1, 49, 49, 512), (2, 33, 20, 96)]


def tile_maxima(s):
    """[..., ceil(nf / TILE)] maxima of the score rows over tiles of TILE keys."""
    nf = s.shape[-1]
    return np.stack([s[..., k:k + TILE].max(-1) for k in range(0, nf, TILE)], -1)


def rises_in_every_tile(s):
    m = tile_maxima(s)
    return bool(np.all(np.diff(m, axis=-1) > 0))


def first_tile_holds_the_maximum(s):
    return bool(np.all(s.argmax(-1) < TILE))


def mean_peak(g, f):
    return float(softmax_rows(scores(g, f)).max(-1).mean())


# ---- the mixing ---------------------------------------------------------------------------------------------------------------
def mix(r, x, gamma, keep=None, drop_rate=0.0, dtype=f64):
    """z = (r * gamma + x) * keep / (1 - drop_rate); keep = None: no dropout."""
    z = np.asarray(r, dtype) * dtype(gamma) + np.asarray(x, dtype)
    if keep is not None:
        z = z * (np.asarray(keep, dtype) * (dtype(1) / (dtype(1) - dtype(drop_rate))))
    return z


def mix_bwd(dz, r, gamma, keep=None, drop_rate=0.0, dx_prior=None, dgamma_prior=0.0, dtype=f64):
    """(dr, dx, dgamma) of mix(): dz' = dz * keep / (1 - drop_rate); dr = dz' gamma; dx = dz' (+ prior); dgamma = prior + <dz', r>."""
    d = np.asarray(dz, dtype)
    if keep is not None:
        d = d * (np.asarray(keep, dtype) * (dtype(1) / (dtype(1) - dtype(drop_rate))))
    dx = d if dx_prior is None else d + np.asarray(dx_prior, dtype)
    return d * dtype(gamma), dx, dtype(dgamma_prior) + (d * np.asarray(r, dtype)).sum(dtype=dtype)
