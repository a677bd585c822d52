"""The per-map saliency loss P3D_LOSS_KLD_CC (map_loss.hip): w_kld KL + w_cc (1 - CC) per [H, W] map, at op level through
p3d_debug_map_loss against the float64 restatement in map_loss_ref.py, across batch shards, and in whole networks against
an oracle composed here (the float64 graph of oracle.p3d / oracle.p3d_gn and a float64 map-loss tape op).  Every op-level
call runs twice and must be bit-equal run to run.

Bounds at op level, per map of N elements (eps64, eps32 the float64 / float32 machine epsilons):
* Sigmoid heads (through_sigmoid): the kernel reads the same float32 s as the reference, so the two differ only by float64
  rounding.  S, Y, A, B, C are sums of N terms (relative error <= N eps64 of their magnitude); p and q inherit it, and each
  log term adds a few roundings, so KL_m is within 8 N eps64 (sum |q log(.)| + 1) (the 1: the relative error of p and q
  times sum q = 1).  CC = C / sqrt(A B) with sum |ds dy| <= sqrt(A B) (Cauchy-Schwarz): within 16 N eps64.  Each dlogit
  is one float32 rounding of a float64 value (eps32 of it) plus a cancellation floor of 8 N eps64 times the magnitudes of
  the terms it was formed from (|g_i| + |sum g p| + sum |g p|, over S, and |y - ybar| / sqrt(A B) + |CC| |s - sbar| / A,
  weighted), times s (1 - s).
* Raw heads: the kernel forms s = 1/(1+expf(-z)) on the device, which may differ from numpy's float32 form by a few ulps:
  delta_i <= 4 eps32 s_i.  To first order that moves KL_m by sum |dKL/ds_i| delta_i and CC_m by sum |dCC/ds_i| delta_i
  (taken twice, for the second order), and a dlogit by |dL/ds_i| delta_i (through s (1 - s)) plus s (1 - s) times the change
  of dL/ds_i: 16 eps32 (1 + sum |s - sbar| s / A) of its term magnitudes (p, q, S shift by a few eps32 relative; A by
  8 eps32 sum |s - sbar| s / A).
* The total folds the weighted map terms in map order: within the sum of the maps' bounds plus (maps + 2) eps64 of the sum
  of |terms|."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_loss_ref as ref      # noqa: E402
from oracle import nn, p3d, p3d_gn      # noqa: E402
from oracle.p3d import Graph            # noqa: E402
from sap3d_tensorflow_amd import ops    # noqa: E402
from test_gpu_loss import (GN_HEADS, PARITY, SIGMOID_HEADS, STRUCTURES, _check_grads, _parity_case, bits_equal,  # noqa: E402
                           make_session)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)
TINY32 = float(np.finfo(np.float32).tiny)
SIZES = [(7, 9), (112, 112), (224, 224)]
WEIGHTS = [(1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.25, 2.5)]


def blocks_per_map(n):
    return max(1, min(256, -(-n // 2048)))


def map_loss_twice(z, p, y, maps, ts, offset, kw, cw, loss0=0.0):
    a = ops.map_loss(z, p, y, maps, z.size // maps, ts, offset, kw, cw, loss0)
    b = ops.map_loss(z, p, y, maps, z.size // maps, ts, offset, kw, cw, loss0)
    assert a[0] == b[0] and bits_equal(a[1], b[1]) and bits_equal(a[2], b[2]) and a[3] == b[3], "run-to-run difference"
    return a


def check_map_loss(z, y, maps, ts, offset, kw, cw, loss0=0.0):
    """Runs the hook on logits z (pred = their float32 sigmoid) and targets y, checks it against map_loss_ref within the
    module's bounds, and returns (loss, dlogits, per_map)."""
    z = np.asarray(z, np.float32).ravel()
    y = np.asarray(y, np.float32).ravel()
    s = ref.sigmoid32(z)
    n = z.size // maps
    loss, dl, per, info = map_loss_twice(z, s, y, maps, ts, offset, kw, cw, loss0)
    assert info == (3, blocks_per_map(n), 1 if offset == 0 and n % 4 == 0 else 2), (info, n, offset)
    assert np.isfinite(loss) and np.all(np.isfinite(dl))
    s64 = s.astype(np.float64).reshape(maps, n)
    y64 = y.astype(np.float64).reshape(maps, n)
    delta = np.zeros_like(s64) if ts else 4 * EPS32 * s64
    dl = dl.reshape(maps, n)
    want_total, bound_total, mag_total = 0.0, 0.0, abs(loss0)
    for m in range(maps):
        r = ref.one_map(s64[m], y64[m], kw, cw)
        rk = ref.one_map(s64[m], y64[m], 1.0, 0.0)
        rc = ref.one_map(s64[m], y64[m], 0.0, 1.0)
        b_kl = 8 * n * EPS64 * (rk["kl_mag"] + 1) + 2 * float((np.abs(rk["dlds"]) * delta[m]).sum())
        b_cc = 16 * n * EPS64 + 2 * float((np.abs(rc["dlds"]) * delta[m]).sum())
        assert abs(per[m, 0] - r["kl"]) <= b_kl, (m, per[m, 0], r["kl"], b_kl)
        if r["defined"]:
            assert abs(per[m, 1] - r["cc"]) <= b_cc, (m, per[m, 1], r["cc"], b_cc)
        else:
            assert np.isnan(per[m, 1]), (m, per[m, 1])
        want_total += r["loss"]
        mag_total += abs(r["loss"])
        bound_total += kw * b_kl + (cw * b_cc if r["defined"] else 0.0)
        # dlogits
        sig = s64[m] * (1 - s64[m])
        want = r["dlds"] * sig
        rel = 8 * n * EPS64
        if not ts:
            ds = s64[m] - s64[m].mean()
            rel += 16 * EPS32 * (1 + (float((np.abs(ds) * s64[m]).sum()) / r["A"] if r["defined"] else 0.0))
        tol = EPS32 * np.abs(want) + rel * r["termmag"] * sig + np.abs(r["dlds"]) * delta[m] + TINY32
        bad = np.abs(dl[m] - want) > tol
        assert not bad.any(), (m, np.flatnonzero(bad)[:5], dl[m][bad][:5], want[bad][:5])
    assert abs(loss - (loss0 + want_total)) <= bound_total + (maps + 2) * EPS64 * mag_total, (loss, loss0 + want_total)
    return loss, dl.ravel(), per


def random_maps(maps, h, w, seed):
    rng = np.random.default_rng(seed)
    z = rng.normal(0, 2, (maps, h, w)).astype(np.float32)
    # a smooth blob plus noise, like a density map
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = rng.uniform(0, h, (maps, 1, 1)), rng.uniform(0, w, (maps, 1, 1))
    y = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * (0.2 * max(h, w)) ** 2)) * 0.8 + 0.2 * rng.random((maps, h, w))
    return z, y.astype(np.float32)


@pytest.mark.parametrize("maps", [1, 3, 128])
@pytest.mark.parametrize("hw", SIZES, ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("ts", [1, 0])
def test_op_level(maps, hw, offset, ts):
    z, y = random_maps(maps, hw[0], hw[1], seed=maps * 7 + hw[0] + offset * 3 + ts)
    weights = WEIGHTS if maps < 128 else [(1.0, 1.0), WEIGHTS[-1]]
    for kw, cw in weights:
        check_map_loss(z, y, maps, ts, offset, kw, cw)


def test_adds_to_the_loss():
    z, y = random_maps(3, 7, 9, 1)
    l0, d0, p0 = check_map_loss(z, y, 3, 1, 0, 1.0, 1.0)
    l1, d1, p1 = check_map_loss(z, y, 3, 1, 0, 1.0, 1.0, loss0=123.25)
    assert l1 == 123.25 + l0 and bits_equal(d0, d1) and bits_equal(p0, p1)


def test_maps_do_not_depend_on_the_alignment():
    """The quads are visited in the same order on the float4 and the scalar path: a map's results are the same bits."""
    z, y = random_maps(3, 112, 112, 2)
    runs = [map_loss_twice(z.ravel(), ref.sigmoid32(z.ravel()), y.ravel(), 3, 1, off, 1.0, 1.0) for off in (0, 1, 2, 3)]
    assert [r[3][2] for r in runs] == [1, 2, 2, 2]
    for r in runs[1:]:
        assert r[0] == runs[0][0] and bits_equal(r[1], runs[0][1]) and bits_equal(r[2], runs[0][2])


# ---- edge maps -----------------------------------------------------------------------------------------------------------
def edge_maps(h=7, w=9):
    rng = np.random.default_rng(11)
    n = h * w
    zs, ys = [], []
    zs.append(rng.normal(0, 2, n)); ys.append(np.zeros(n))                             # Y = 0
    zs.append(np.full(n, 0.7)); ys.append(rng.random(n))                               # constant prediction: no CC
    one = np.zeros(n); one[n // 3] = 0.9
    zs.append(rng.normal(0, 2, n)); ys.append(one)                                     # one nonzero target pixel
    zs.append(np.full(n, -200.0) - rng.random(n)); ys.append(rng.random(n))            # s exactly 0: S = 0
    zs.append(rng.normal(0, 2, n)); ys.append((rng.random(n) < 0.4).astype(float))     # targets of exactly 0 and 1
    zs.append(np.full(n, -200.0)); ys.append(np.zeros(n))                              # both sums 0
    return np.stack(zs).astype(np.float32), np.stack(ys).astype(np.float32)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("ts", [1, 0])
@pytest.mark.parametrize("hw", [(7, 9), (16, 16)], ids=lambda v: "%dx%d" % v)
def test_edge_maps(offset, ts, hw):
    z, y = edge_maps(*hw)
    n = hw[0] * hw[1]
    assert np.all(ref.sigmoid32(z[3]) == 0) and np.all(ref.sigmoid32(z[5]) == 0)
    for kw, cw in WEIGHTS:
        loss, dl, per = check_map_loss(z, y, z.shape[0], ts, offset, kw, cw)
        dl = dl.reshape(-1, n)
        assert np.isnan(per[0, 1]) and np.isnan(per[1, 1]) and np.isnan(per[5, 1])     # B = 0, A = 0, both
        assert per[0, 0] == 0 and per[5, 0] == 0
        assert np.all(dl[3] == 0) and np.all(dl[5] == 0)          # s = 0: zero dlogits through the sigmoid
        if cw and not kw:
            assert np.all(dl[1] == 0)        # a map without CC adds nothing to the CC gradient (and its KL term is off)


# ---- batch shards ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(7, 9), (112, 112)], ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("ts", [1, 0])
def test_shards_are_bit_identical(hw, ts):
    z, y = random_maps(16, hw[0], hw[1], 21)
    z, y = z.reshape(16, -1), y.reshape(16, -1)
    s = ref.sigmoid32(z)
    full = map_loss_twice(z.ravel(), s.ravel(), y.ravel(), 16, ts, 0, 1.0, 1.0)
    lo = map_loss_twice(z[:8].ravel(), s[:8].ravel(), y[:8].ravel(), 8, ts, 0, 1.0, 1.0)
    hi = map_loss_twice(z[8:].ravel(), s[8:].ravel(), y[8:].ravel(), 8, ts, 0, 1.0, 1.0)
    assert bits_equal(full[2], np.concatenate([lo[2], hi[2]]))
    assert bits_equal(full[1], np.concatenate([lo[1], hi[1]]))
    terms = per_map_terms(full[2], 1.0, 1.0)
    assert abs(full[0] - (lo[0] + hi[0])) <= 18 * EPS64 * float(np.abs(terms).sum()), (full[0], lo[0] + hi[0])


def per_map_terms(per, kw, cw):
    cc = per[:, 1]
    return kw * per[:, 0] + np.where(np.isnan(cc), 0.0, cw * (1 - np.nan_to_num(cc)))


# ---- whole networks against float64 ------------------------------------------------------------------------------------
def map_loss_op(tape, pred, y, raw, kw=1.0, cw=1.0):
    """The per-map loss on the network's output [B, T, H, W]: s = pred on a sigmoid head (the oracle's sigmoid backward then
    multiplies by s (1 - s)), sigmoid(output) on a raw one, the op applying the sigmoid and its derivative itself."""
    v = pred.data
    maps = y.shape[0] * y.shape[1]
    v64 = v.astype(np.float64).reshape(maps, -1)
    s = 1 / (1 + np.exp(-v64)) if raw else v64
    y64 = np.asarray(y, np.float64).reshape(maps, -1)
    rows = [ref.one_map(s[m], y64[m], kw, cw) for m in range(maps)]
    dd = np.stack([r["dlds"] for r in rows])
    if raw:
        dd = dd * s * (1 - s)
    out = nn.Var(np.asarray(sum(r["loss"] for r in rows), dtype=v.dtype))

    def bwd():
        pred.acc((out.grad * dd.reshape(v.shape)).astype(v.dtype))
    tape.record(bwd)
    return out


def oracle_map_loss(structure, params, x, y, cfg, dtype):
    g = Graph(params, dtype=dtype, create=False)
    X = nn.Var(x.astype(dtype))
    if structure in GN_HEADS:
        pred = p3d_gn.HEADS[GN_HEADS[structure]](g, X, 0.0, x.shape[0], True, cfg, None)
    else:
        pred = p3d.STRUCTURES[structure](g, X, 0.0, x.shape[0], True, cfg, None)
    loss = map_loss_op(g.tape, nn.reshape(g.tape, pred, y.shape), y, structure not in SIGMOID_HEADS)
    g.tape.backward(loss)
    return float(loss.data), {n: v.grad for n, v in g.trainable.items()}


@pytest.mark.parametrize("structure,ci", PARITY)
def test_kld_cc_network_matches_float64(structure, ci):
    cfg, shape, p64, p32, x, y = _parity_case(structure, ci)
    s = make_session(cfg, shape, p32, structure)
    _, pred_sl1 = s.backward(x, y, 0.0)
    s.set_loss("kld_cc")
    loss, pred = s.backward(x, y, 0.0)
    assert bits_equal(pred, pred_sl1)                   # the forward pass does not depend on the loss
    l64, g64 = oracle_map_loss(structure, p64, x.astype(np.float64), y.astype(np.float64), cfg, np.float64)
    _, g32 = oracle_map_loss(structure, dict(p32), x, y, cfg, np.float32)
    assert np.isfinite(loss) and abs(loss - l64) <= 1e-5 * abs(l64), (loss, l64)
    _check_grads(s, g64, g32)
    s.close()


@pytest.mark.parametrize("structure,cfg,shape", STRUCTURES)
def test_train_step_on_every_structure(structure, cfg, shape):
    from sap3d_tensorflow_amd import P3DSession
    x, y = p3d.synthetic_clip(0, shape + (3,)), p3d.synthetic_target(3, shape)
    s = P3DSession(structure, batch=shape[0], frames=shape[1], height=shape[2], width=shape[3], base=cfg.base, blocks=cfg.blocks,
                   seed=1)
    s.set_loss("kld_cc", cc_weight=0.5)
    before = {n: s.get_param(n) for n, _, tr in s.variables() if tr}
    loss = s.train_step(x, y, dropout=0.5, seed=3)
    assert np.isfinite(loss)
    changed = [n for n, v in before.items() if not bits_equal(s.get_param(n), v)]
    assert changed and all(np.all(np.isfinite(s.get_param(n))) for n in before)
    s.close()


# ---- the default is untouched --------------------------------------------------------------------------------------------
def test_default_loss_is_untouched():
    from test_gpu_net import SMALL, randomise_norm_params
    cfg, shape = SMALL[0]
    p32 = {k: v.astype(np.float32) for k, v in randomise_norm_params(p3d.init_params(1, "unet", cfg, dtype=np.float64)).items()}
    x, y = p3d.synthetic_clip(0, shape + (3,)), p3d.synthetic_target(3, shape)
    outs = []
    for switches in ([], ["smooth_l1", "kld_cc", "smooth_l1"]):
        s = make_session(cfg, shape, p32)
        for name in switches:
            s.set_loss(name)
        loss, pred = s.backward(x, y, 0.0)
        outs.append((np.float32(loss), pred, {n: s.get_grad(n) for n, _, tr in s.variables() if tr}))
        s.close()
    loss, pred, grads = outs[1]
    assert loss.tobytes() == outs[0][0].tobytes() and bits_equal(pred, outs[0][1])
    assert all(bits_equal(g, outs[0][2][n]) for n, g in grads.items())
    # the launch list: the Smooth-L1 launch is replaced by the three map-loss launches, nothing else changes
    s = make_session(cfg, shape, p32)
    s.upload(x, y)
    s.schedule()
    base = s.schedule()
    s.set_loss("kld_cc")
    kld = s.schedule()
    s.close()
    i = [k for k, line in enumerate(base) if "smooth_l1_kernel" in line]
    assert len(i) == 1, i
    i = i[0]
    assert len(kld) == len(base) + 2
    assert kld[:i] == base[:i] and kld[i + 3:] == base[i + 1:]
    assert kld[i:i + 3] == [base[i].replace("smooth_l1_kernel", k)
                            for k in ("map_loss_sums_kernel", "map_loss_terms_kernel", "map_loss_grad_kernel")]


# ---- captured step ---------------------------------------------------------------------------------------------------------
def test_captured_step_gives_the_eager_trajectory():
    """P3D_GRAPH=1: kld_cc steps, then a weight change (which drops the captured step), give the eager trajectory bit for
    bit."""
    script = (
        "import sys, hashlib, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "from oracle import p3d\n"
        "from sap3d_tensorflow_amd import P3DSession\n"
        "shape = (2, 16, 48, 48)\n"
        "s = P3DSession('unet', batch=2, frames=16, height=48, width=48, base=16, blocks=(2, 2, 3), seed=3)\n"
        "s.set_adam(1e-3)\n"
        "s.upload(p3d.synthetic_clip(0, shape + (3,)), p3d.synthetic_target(3, shape))\n"
        "losses = []\n"
        "for cw, k in ((1.0, 3), (0.5, 2)):\n"
        "    s.set_loss('kld_cc', cc_weight=cw)\n"
        "    for i in range(k):\n"
        "        s.train_step_device(0.5, seed=50 + len(losses))\n"
        "        losses.append(np.float32(s.last_loss()).tobytes().hex())\n"
        "h = hashlib.sha256()\n"
        "for n, _, _ in s.variables():\n"
        "    h.update(s.get_param(n).tobytes())\n"
        "print('RESULT', ' '.join(losses), h.hexdigest())\n"
        "s.close()\n" % ROOT)
    outs = []
    for graph in ("0", "1"):
        env = dict(os.environ, P3D_GRAPH=graph)
        r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")]
        assert line, r.stdout[-2000:]
        outs.append(line[0])
        if graph == "1":
            assert "capture failed" not in r.stderr, r.stderr[-2000:]
    assert outs[0] == outs[1]
    losses = [np.frombuffer(bytes.fromhex(v), np.float32)[0] for v in outs[0].split()[1:6]]
    assert np.all(np.isfinite(losses))


# ---- the driver --------------------------------------------------------------------------------------------------------
def test_train_driver_with_kld_cc(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "drivers", "train.py"), "--loss", "kld_cc", "--cc-weight", "0.5",
                        "--batch", "2", "--imagesize", "32", "32", "--steps", "2", "--plotiter", "1", "--validiter", "100",
                        "--saveiter", "100"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    losses = [float(v) for v in re.findall(r"Training Loss (\S+)", r.stdout)]
    assert len(losses) == 2 and np.all(np.isfinite(losses)), r.stdout[-3000:]
