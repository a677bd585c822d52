"""The loss option beside Smooth-L1 (p3d_set_loss; BASELINE.json configs[2]): sigmoid cross-entropy on the head's logits
(sigmoid_ce_kernel) and the L1 sum (l1_loss_kernel), at op level through p3d_debug_loss and in whole networks.  Neither has
a reference counterpart to compare with, so both are held to float64 here: at op level element by element, in the network
through an oracle composed in this file (the graph of oracle.p3d / oracle.p3d_gn, its reshape, and a float64 loss op).
Every op-level call runs twice and must be bit-equal run to run.

Sigmoid cross-entropy.  Each float32 term max(z,0) - z y + log1p(exp(-|z|)) is within a few roundings of its value; its
magnitude is |max(z,0)| + |z y| + log1p(exp(-|z|)), and the double sum over n terms adds n eps64 of the magnitude sum, so the
loss is held to 2 eps32 mag + n eps64 mag.  The gradient sigmoid(z) - y is, on a sigmoid head, the stored pred minus y (one
rounding: compared bit for bit); on a raw head the kernel evaluates 1/(1+expf(-z)) as the head does, a few ulps of sigmoid
plus the rounding of the difference: 4 eps32 (sigmoid + |y|).
L1.  |p - y| rounds once: the Smooth-L1 bound.  The gradient sign(p - y), times p (1 - p) through the sigmoid, is compared
bit for bit with the same float32 operations in the same order."""
import hashlib
import os
import re
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import nn, p3d, p3d_gn      # noqa: E402
from oracle.p3d import Graph            # noqa: E402
from sap3d_tensorflow_amd import ops    # noqa: E402
from test_gpu_net import GN_SMALL, SMALL, _gn_params, grads_vs_oracles, make_session, randomise_norm_params  # noqa: E402
from test_loss_cpu import bce64, sigmoid64      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)
LENGTHS = [1, 3, 4, 5, 1021, 4096, 1024 * 256 * 4 + 12]
SIGMOID_HEADS = ("unet", "unet++nonsa", "unet++ds")
GN_HEADS = {"gn_p3d": "p3d", "gn_p3d_concat": "concat", "gn_p3d_decoder": "decoder"}


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def sigmoid32(z):
    """The head's pred = 1/(1+exp(-z)) in float32 (exactly 0 once exp(-z) overflows)."""
    z = np.asarray(z, np.float32)
    with np.errstate(over="ignore"):
        return (np.float32(1) / (np.float32(1) + np.exp(-z))).astype(np.float32)


def loss_twice(kind, z, p, y, through_sigmoid, offset, loss0=0.0):
    a = ops.loss(kind, z, p, y, through_sigmoid, offset, loss0)
    b = ops.loss(kind, z, p, y, through_sigmoid, offset, loss0)
    assert a[0] == b[0] and bits_equal(a[1], b[1]) and a[2] == b[2], "run-to-run difference"
    return a


def check_info(info, n, offset):
    assert info[0] == (1 if offset == 0 and n % 4 == 0 else 2), (n, offset, info)
    assert info[1] == min(1024, -(-n // 256)), info


# ---- sigmoid cross-entropy at op level -----------------------------------------------------------------------------------
def check_bce(z, y, through_sigmoid, offset, loss0=0.0):
    z, y = np.asarray(z, np.float32), np.asarray(y, np.float32)
    p = sigmoid32(z) if through_sigmoid else z           # what a sigmoid / raw head stores as pred
    n = z.size
    loss, dl, info = loss_twice("bce", z, p, y, through_sigmoid, offset, loss0)
    check_info(info, n, offset)
    z64, y64 = z.astype(np.float64), y.astype(np.float64)
    want = float(bce64(z64, y64).sum())
    mag = float((np.abs(np.maximum(z64, 0)) + np.abs(z64 * y64) + np.log1p(np.exp(-np.abs(z64)))).sum())
    assert np.isfinite(loss)
    assert abs(loss - (loss0 + want)) <= 2 * EPS32 * mag + n * EPS64 * (mag + abs(loss0)), (n, offset, loss, loss0 + want)
    if through_sigmoid:
        assert bits_equal(dl, (p - y).astype(np.float32)), (n, offset)
    else:
        s = sigmoid64(z64)
        # (+ the smallest normal: a sigmoid below it may come out of the division flushed)
        assert np.all(np.abs(dl - (s - y64)) <= 4 * EPS32 * (s + np.abs(y64)) + np.finfo(np.float32).tiny), (n, offset)
    return loss, dl


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("through_sigmoid", [True, False])
def test_bce_lengths(n, offset, through_sigmoid):
    rng = np.random.default_rng(n + offset)
    check_bce(rng.normal(0, 3, n), rng.random(n), through_sigmoid, offset)


def test_bce_edges():
    zs = np.array([0, 1e-8, -1e-8, 15, -15, 17, -17, 88, -88, 89, -89, 100, -100, 1e4, -1e4], np.float32)
    ys = np.array([0, 1, 0.5, 0.37], np.float32)
    z, y = np.repeat(zs, ys.size), np.tile(ys, zs.size)
    for through_sigmoid in (True, False):
        for offset in (0, 1, 2, 3):
            loss, dl = check_bce(z, y, through_sigmoid, offset)
            zero = z == 0
            assert bits_equal(dl[zero], (np.float32(0.5) - y[zero]).astype(np.float32))
            if not through_sigmoid:
                # saturated logits: sigmoid(z) is exactly 1 (exp(-z) below half an ulp of 1) or exactly 0 (exp(-z) overflows)
                one, nil = z >= 17, z <= -89
                assert bits_equal(dl[one], (np.float32(1) - y[one]).astype(np.float32))
                assert bits_equal(dl[nil], (np.float32(0) - y[nil]).astype(np.float32))      # (+0 at y = 0)
    # z = 0: log 2 per element, whatever y is
    n = 1000
    loss, dl = check_bce(np.zeros(n), np.random.default_rng(1).random(n), False, 0)
    assert abs(loss - n * np.log(2)) <= n * 2 * EPS32 * np.log(2)


# ---- L1 at op level --------------------------------------------------------------------------------------------------------
def check_l1(z, p, y, through_sigmoid, offset, loss0=0.0):
    z, p, y = (np.asarray(a, np.float32) for a in (z, p, y))
    n = p.size
    loss, dl, info = loss_twice("l1", z, p, y, through_sigmoid, offset, loss0)
    check_info(info, n, offset)
    d = p - y                                             # float32, as the kernel forms it
    g = np.sign(d).astype(np.float32)
    if through_sigmoid:
        g = g * (p * (np.float32(1) - p))
    assert bits_equal(dl, g.astype(np.float32)), (n, offset)
    d64 = p.astype(np.float64) - y
    mag = float(np.abs(d64).sum())
    assert abs(loss - (loss0 + mag)) <= 2 * EPS32 * mag + n * EPS64 * (mag + abs(loss0)), (n, offset, loss, loss0 + mag)
    return loss, dl


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("through_sigmoid", [True, False])
def test_l1_lengths(n, offset, through_sigmoid):
    rng = np.random.default_rng(n + offset + 7)
    y = rng.random(n).astype(np.float32)
    z = rng.normal(0, 3, n).astype(np.float32)
    p = sigmoid32(z) if through_sigmoid else (y + rng.normal(0, 1.5, n)).astype(np.float32)
    p[::97] = y[::97]                                     # d = 0: gradient 0
    if not through_sigmoid:
        z = p
    loss, dl = check_l1(z, p, y, through_sigmoid, offset)
    assert np.all(dl[::97] == 0)


# ---- both add to the incoming loss -------------------------------------------------------------------------------------
def test_losses_add_to_the_loss():
    rng = np.random.default_rng(4)
    z = rng.normal(0, 3, 5000).astype(np.float32)
    p, y = sigmoid32(z), rng.random(5000).astype(np.float32)
    l0, d0 = check_bce(z, y, True, 0)
    l1, d1 = check_bce(z, y, True, 0, loss0=123.25)
    assert l1 == 123.25 + l0 and bits_equal(d0, d1)
    l0, d0 = check_l1(z, p, y, True, 0)
    l1, d1 = check_l1(z, p, y, True, 0, loss0=123.25)
    assert l1 == 123.25 + l0 and bits_equal(d0, d1)


def test_unknown_loss_kind_is_an_error():
    from sap3d_tensorflow_amd import P3dError
    one = np.ones(4, np.float32)
    with pytest.raises(P3dError):
        ops.loss(3, one, one, one)


# ---- whole networks against float64 --------------------------------------------------------------------------------------
def loss_op(tape, pred, y, kind, on_probs, sign_of=None):
    """The loss on the network's output: BCE on probabilities (sigmoid heads; the oracle's sigmoid backward then multiplies
    by p (1 - p)) or on logits (raw heads), or L1 (whose sign, where given, is taken from sign_of: the HIP pass's own
    float32 p - y, so that both are differentiated on the same branch)."""
    v = pred.data
    y = np.asarray(y, v.dtype)
    if kind == "bce" and on_probs:
        per = -(y * np.log(v) + (1 - y) * np.log(1 - v))
        dd = (v - y) / (v * (1 - v))
    elif kind == "bce":
        per = np.maximum(v, 0) - v * y + np.log1p(np.exp(-np.abs(v)))
        dd = sigmoid64(v).astype(v.dtype) - y
    else:
        per = np.abs(v - y)
        dd = np.sign(v - y if sign_of is None else sign_of).astype(v.dtype)
    out = nn.Var(np.asarray(per.sum(dtype=np.float64), dtype=v.dtype))

    def bwd():
        pred.acc((out.grad * dd).astype(v.dtype))
    tape.record(bwd)
    return out


def oracle_loss(structure, params, x, y, cfg, dtype, kind="bce", sign_of=None):
    g = Graph(params, dtype=dtype, create=False)
    X = nn.Var(x.astype(dtype))
    if structure in GN_HEADS:
        pred = p3d_gn.HEADS[GN_HEADS[structure]](g, X, 0.0, x.shape[0], True, cfg, None)
    else:
        pred = p3d.STRUCTURES[structure](g, X, 0.0, x.shape[0], True, cfg, None)
    loss = loss_op(g.tape, nn.reshape(g.tape, pred, y.shape), y, kind, structure in SIGMOID_HEADS, sign_of)
    g.tape.backward(loss)
    return float(loss.data), pred.data, OrderedDict((n, v.grad) for n, v in g.trainable.items())


# the cases whose Smooth-L1 gradient gate is measured at 0.0 (tests/golden/measured_gates.json)
PARITY = [("unet", 0), ("unet", 1), ("concat", 0), ("concat", 1), ("gn_p3d", 1)]


def _parity_case(structure, ci):
    if structure in GN_HEADS:
        cfg, shape = GN_SMALL[ci]
        p64 = _gn_params(cfg, np.float64, GN_HEADS[structure])
    else:
        cfg, shape = SMALL[ci]
        p64 = randomise_norm_params(p3d.init_params(1, structure, cfg, dtype=np.float64))
    p32 = {k: v.astype(np.float32) for k, v in p64.items()}
    x = p3d.synthetic_clip(0, shape + (3,))
    y = p3d.synthetic_target(3, shape)
    return cfg, shape, p64, p32, x, y


def _check_grads(s, g64, g32):
    errs, errs32 = grads_vs_oracles(s, g64, g32)
    bad = {n: (e, errs32[n]) for n, e in errs.items() if not e <= 5 * errs32[n] + 2e-3}
    assert not bad, bad


@pytest.mark.parametrize("structure,ci", PARITY)
def test_bce_network_matches_float64(structure, ci):
    cfg, shape, p64, p32, x, y = _parity_case(structure, ci)
    s = make_session(cfg, shape, p32, structure)
    _, pred_sl1 = s.backward(x, y, 0.0)
    s.set_loss("bce")
    loss, pred = s.backward(x, y, 0.0)
    assert bits_equal(pred, pred_sl1)                   # the forward pass does not depend on the loss
    l64, _, g64 = oracle_loss(structure, p64, x.astype(np.float64), y.astype(np.float64), cfg, np.float64)
    _, _, g32 = oracle_loss(structure, dict(p32), x, y, cfg, np.float32)
    assert abs(loss - l64) <= 1e-5 * abs(l64), (loss, l64)
    _check_grads(s, g64, g32)
    s.close()


def test_l1_network_matches_float64():
    cfg, shape, p64, p32, x, y = _parity_case("unet", 0)
    s = make_session(cfg, shape, p32, "unet")
    s.set_loss("l1")
    loss, pred = s.backward(x, y, 0.0)
    sign = pred.reshape(y.shape) - y.astype(np.float32)      # the kernel's own float32 p - y
    l64, pr64, g64 = oracle_loss("unet", p64, x.astype(np.float64), y.astype(np.float64), cfg, np.float64, "l1", sign)
    _, _, g32 = oracle_loss("unet", dict(p32), x, y, cfg, np.float32, "l1", sign)
    assert np.abs(pred - pr64).max() < 1e-4
    assert abs(loss - l64) <= 1e-5 * abs(l64), (loss, l64)
    _check_grads(s, g64, g32)
    s.close()


# ---- every structure -------------------------------------------------------------------------------------------------
STRUCTURES = [
    ("unet", p3d.NetConfig(base=16, blocks=(2, 2, 3)), (2, 16, 48, 48)),
    ("concat", p3d.NetConfig(base=16, blocks=(1, 2, 2)), (2, 16, 32, 32)),
    ("unet++nonsa", p3d.NetConfig(base=16, blocks=(1, 1, 2)), (2, 16, 32, 32)),
    ("unet++ds", p3d.NetConfig(base=16, blocks=(1, 1, 2)), (2, 16, 32, 32)),
    ("gn_p3d", p3d.NetConfig(base=16, blocks=(1, 2, 2)), (2, 16, 32, 32)),
    ("gn_p3d_concat", p3d.NetConfig(base=16, blocks=(1, 1, 2)), (2, 16, 32, 32)),
    ("gn_p3d_decoder", p3d.NetConfig(base=16, blocks=(1, 1, 2)), (2, 16, 32, 32)),
]


def _session(structure, cfg, shape, loss="bce"):
    from sap3d_tensorflow_amd import P3DSession
    s = P3DSession(structure, batch=shape[0], frames=shape[1], height=shape[2], width=shape[3], base=cfg.base, blocks=cfg.blocks,
                   seed=1)
    s.set_loss(loss)
    return s


@pytest.mark.parametrize("structure,cfg,shape", STRUCTURES)
def test_bce_on_every_structure(structure, cfg, shape):
    x, y = p3d.synthetic_clip(0, shape + (3,)), p3d.synthetic_target(3, shape)
    s = _session(structure, cfg, shape)
    loss, _ = s.backward(x, y, 0.0)
    z = s.activation("logits").astype(np.float64).reshape(y.shape)
    want = float(bce64(z, y).sum())
    mag = float((np.abs(np.maximum(z, 0)) + np.abs(z * y) + np.log1p(np.exp(-np.abs(z)))).sum())
    assert abs(loss - want) <= EPS32 * abs(want) + 2 * EPS32 * mag + z.size * EPS64 * mag, (loss, want)
    for n, _, tr in s.variables():
        if tr:
            assert np.all(np.isfinite(s.get_grad(n))), n
    buckets, n_train, stale = s.bucket_audit(1 << 16, dropout=0.5, seed=3)
    assert stale == 0 and len(buckets) >= 2
    s.close()
    runs = []
    for _ in range(2):
        s = _session(structure, cfg, shape)
        losses = [np.float32(s.train_step(x, y, dropout=0.5, seed=10 + i)).tobytes() for i in range(3)]
        h = hashlib.sha256()
        for n, _, _ in s.variables():
            h.update(s.get_param(n).tobytes())
        runs.append((losses, h.hexdigest()))
        assert all(np.isfinite(np.frombuffer(b, np.float32)[0]) for b in losses)
        s.close()
    assert runs[0] == runs[1]


# ---- the default is untouched --------------------------------------------------------------------------------------------
def test_default_loss_is_untouched():
    cfg, shape = SMALL[0]
    p32 = {k: v.astype(np.float32) for k, v in randomise_norm_params(p3d.init_params(1, "unet", cfg, dtype=np.float64)).items()}
    x, y = p3d.synthetic_clip(0, shape + (3,)), p3d.synthetic_target(3, shape)
    outs = []
    for switches in ([], ["smooth_l1"], ["smooth_l1", "bce", "smooth_l1"]):
        s = make_session(cfg, shape, p32)
        for name in switches:
            s.set_loss(name)
        loss, pred = s.backward(x, y, 0.0)
        outs.append((np.float32(loss), pred, {n: s.get_grad(n) for n, _, tr in s.variables() if tr}))
        s.close()
    for loss, pred, grads in outs[1:]:
        assert loss.tobytes() == outs[0][0].tobytes() and bits_equal(pred, outs[0][1])
        assert all(bits_equal(g, outs[0][2][n]) for n, g in grads.items())
    # the launch list: only the loss launch differs
    s = make_session(cfg, shape, p32)
    s.upload(x, y)
    s.schedule()                                        # (a first step, so that both traced steps follow one)
    base = s.schedule()
    s.set_loss("bce")
    bce = s.schedule()
    s.close()
    assert len(base) == len(bce)
    diff = [(a, b) for a, b in zip(base, bce) if a != b]
    assert len(diff) == 1, diff
    a, b = diff[0]
    assert "smooth_l1_kernel" in a and b == a.replace("smooth_l1_kernel", "sigmoid_ce_kernel"), diff


# ---- captured step ---------------------------------------------------------------------------------------------------------
def test_captured_step_follows_the_loss_switch():
    """P3D_GRAPH=1: a switch drops the captured step; the next step captures the new loss.  Both processes (eager and
    captured) must give the same trajectory bit for bit."""
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
        "for name, k in (('bce', 4), ('smooth_l1', 2)):\n"
        "    s.set_loss(name)\n"
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
    losses = [np.frombuffer(bytes.fromhex(v), np.float32)[0] for v in outs[0].split()[1:7]]
    # BCE and Smooth-L1 of the same maps differ: the switch back took effect
    assert np.all(np.isfinite(losses)) and abs(losses[4] - losses[3]) > 0.1 * abs(losses[3])


# ---- the driver --------------------------------------------------------------------------------------------------------
def test_train_driver_with_bce(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "drivers", "train.py"), "--loss", "bce", "--batch", "2",
                        "--imagesize", "32", "32", "--steps", "2", "--plotiter", "1", "--validiter", "100", "--saveiter", "100"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    losses = [float(v) for v in re.findall(r"Training Loss (\S+)", r.stdout)]
    assert len(losses) == 2 and np.all(np.isfinite(losses)), r.stdout[-3000:]
