"""Float64 / float32 reference for the regularisation option (P3DSession.set_regularization), composed from the oracle's
graph builders without the library's tags.

The reference's two collections (left out of its loss: train.py:161, gn/train_p3d_gn_dataset.py:188-189):
  * 'weightdecay_losses': get_conv_weight adds wd * tf.nn.l2_loss(var) for every kernel it creates with wd != 0
    (p3d.py:10-16, wd = 0.001 on the BatchNorm nets; gn/p3d_gn.py:54-60, wd = 0.0005 on the GroupNorm nets); the convS /
    convT biases pass wd = 0.  wd_loss = tf.reduce_mean over the collection.
  * REGULARIZATION_LOSSES under scope 'P3D': kernel_regularizer=l2_reg(), 0.0005 * tf.nn.l2_loss (gn/p3d_gn.py:11-21,538),
    on the conv3d_layers / deconv3d_layers kernels and the 'results' conv of the decoder-block head.
The sets are recorded by wrapping oracle.p3d.get_conv_weight (and the name oracle.p3d_gn binds), oracle.p3d_gn's
conv3d_layers / deconv3d_layers and the layers_conv3d call that builds 'results', then building the graph once."""
import numpy as np

from oracle import p3d, p3d_gn

BN_STRUCTURES = ("unet", "concat", "unet++nonsa", "unet++ds")
GN_HEADS = {"gn_p3d": "p3d", "gn_p3d_concat": "concat", "gn_p3d_decoder": "decoder"}
WD_SCALE = {"bn": 0.001, "gn": 0.0005}
L2_SCALE = 0.0005


def recorded_sets(structure, cfg, monkeypatch, input_shape=(1, 16, 32, 32, 3)):
    """(weight-decay names, l2 names, every trainable name in creation order) of one graph build."""
    wd_names, l2_names = [], []
    orig_gcw = p3d.get_conv_weight

    def gcw(g, name, kshape, wd=0.001):
        v = orig_gcw(g, name, kshape, wd)
        if wd != 0 and g.prefix + name not in wd_names:
            wd_names.append(g.prefix + name)
        return v

    def l2_wrap(fn):
        def wrapped(g, x, filters, kernel, strides, name):
            out = fn(g, x, filters, kernel, strides, name)
            if g.prefix == "P3D/":
                l2_names.append(g.prefix + name + "/kernel")
            return out
        return wrapped

    orig_lc = p3d_gn.layers_conv3d

    def layers_conv3d(g, x, filters, kernel, strides, name=None):
        out = orig_lc(g, x, filters, kernel, strides, name=name)
        if name == "results" and g.prefix == "P3D/":
            l2_names.append(g.prefix + "results/kernel")
        return out

    monkeypatch.setattr(p3d, "get_conv_weight", gcw)
    monkeypatch.setattr(p3d_gn, "get_conv_weight", gcw)
    monkeypatch.setattr(p3d_gn, "conv3d_layers", l2_wrap(p3d_gn.conv3d_layers))
    monkeypatch.setattr(p3d_gn, "deconv3d_layers", l2_wrap(p3d_gn.deconv3d_layers))
    monkeypatch.setattr(p3d_gn, "layers_conv3d", layers_conv3d)
    if structure in GN_HEADS:
        params = p3d_gn.init_params(1, cfg, input_shape=input_shape, head=GN_HEADS[structure])
    else:
        params = p3d.init_params(1, structure, cfg, input_shape=input_shape)
    monkeypatch.undo()
    return wd_names, l2_names, list(params)


def coefficients(wd_names, l2_names, terms, wd=None, l2=None, gn=False):
    """{name: float32 coefficient} of the enabled terms: scale / K per variable, formed in float64, rounded once."""
    wd = wd if wd else WD_SCALE["gn" if gn else "bn"]
    l2 = l2 if l2 else L2_SCALE
    c = {}
    if "weightdecay" in terms:
        for n in wd_names:
            c[n] = c.get(n, 0.0) + wd / len(wd_names)
    if "l2" in terms:
        for n in l2_names:
            c[n] = c.get(n, 0.0) + l2 / len(l2_names)
    return {n: np.float32(v) for n, v in c.items()}


def term64(params, coef):
    """sum over the variables of 0.5 * c * sum(w^2), in float64 with the float32 coefficients the library applies."""
    return float(sum(0.5 * float(c) * np.sum(np.asarray(params[n], np.float64) ** 2) for n, c in coef.items()))


def grad64(params, coef):
    """d term / d w = c * w, float64."""
    return {n: float(c) * np.asarray(params[n], np.float64) for n, c in coef.items()}


def decayed_grad32(g, c, w):
    """The kernel's g' = fadd(g, fmul(c, w)) in float32, each operation rounded."""
    g, w = np.asarray(g, np.float32), np.asarray(w, np.float32)
    return (g + np.float32(c) * w).astype(np.float32)


def fma32(a, b, c):
    """Correctly rounded float32 fma(a, b, c): the float64 product is exact, the float64 sum is rounded to odd (exact for the
    one rounding to float32 that follows, 53 >= 24 + 2 bits)."""
    a, b, c = (np.asarray(t, np.float32).astype(np.float64) for t in (a, b, c))
    x = a * b
    s = x + c
    bb = s - x
    e = (x - (s - bb)) + (c - bb)                       # exact error of the sum (TwoSum)
    s = np.array(s, np.float64, copy=True, ndmin=1)
    e = np.broadcast_to(e, s.shape)
    fix = (e != 0) & ((s.view(np.uint64) & 1) == 0)
    s[fix] = np.nextafter(s[fix], np.where(e[fix] > 0, np.inf, -np.inf))
    return s.astype(np.float32)


def adam32(p, m, v, g, lr_t, b1, b2, eps, whole):
    """adam_kernel's float32 arithmetic per element: whole = the element's 4-group lies whole in the launch range (m, v as
    single fmas), else the scalar tail form (nothing fused)."""
    f = np.float32
    p, m, v, g = (np.asarray(t, f).copy() for t in (p, m, v, g))
    a1, a2 = f(1) - f(b1), f(1) - f(b2)
    whole = np.broadcast_to(np.asarray(whole, bool), p.shape)
    mw = fma32(np.full(p.shape, f(b1)), m, a1 * g)
    vw = fma32(np.full(p.shape, f(b2)), v, (a2 * g) * g)
    mt = f(b1) * m + a1 * g
    vt = f(b2) * v + (a2 * g) * g
    m2 = np.where(whole, mw, mt).astype(f)
    v2 = np.where(whole, vw, vt).astype(f)
    p2 = (p - (f(lr_t) * m2) / (np.sqrt(v2) + f(eps))).astype(f)
    return p2, m2, v2
