"""The Momentum / SGD optimisers (P3DSession.set_optimizer) and the optimiser state in checkpoints, on the GPU: the kernels at
op level against the bit-exact float32 replays of opt_ref.py, whole steps, three Nesterov steps against the float64 oracle,
the default path, resuming from a checkpoint, data parallelism, the captured step, the refusals and the driver."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from oracle import p3d          # noqa: E402
import opt_ref                  # noqa: E402
import reg_ref                  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(HERE)
EPS64 = np.finfo(np.float64).eps
B1, B2, EPS = 0.9, 0.999, 1e-8
KINDS = {"momentum": ("momentum", False), "nesterov": ("momentum", True), "sgd": ("sgd", False)}


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _inputs(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 0.1).astype(np.float32)
    a = (rng.standard_normal(n) * 0.01).astype(np.float32)
    return p, g, a


# ---- op level ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4097, 2 ** 20 + 3])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("lr_on_device", [False, True])
def test_optimizer_op(n, offset, kind, lr_on_device):
    """Offsets 1-3 start the range mid-16-byte line: the kernel takes those head elements one by one and the rest as float4
    groups; the arithmetic has no fused form, so every element must match the replay whatever its place."""
    from sap3d_tensorflow_amd import ops
    name, nesterov = KINDS[kind]
    p, g, a = _inputs(n, n * 5 + offset)
    lr, mom = 3e-3, 0.9
    got_p, got_a = ops.optimizer(name, p, g, a, lr=lr, momentum=mom, use_nesterov=nesterov, lr_on_device=lr_on_device,
                                 offset=offset)
    want_p, want_a = opt_ref.update32(kind, p, a, g, lr, mom)
    assert _bits_equal(got_p, want_p)
    assert _bits_equal(got_a, want_a)


def _tiles(n, shift):
    """[0, n) cut at offsets `shift` and shift + 1 modulo 4, coefficient 0 beside non-zero ones, and every 8192."""
    k1, k2 = (n // 3) // 4 * 4 + shift, ((2 * n) // 3) // 4 * 4 + shift + 1
    cuts = sorted({0, n} | {k for k in (k1, k2) if 0 < k < n} | set(range(8192 + shift, n, 8192)))
    coefs = [np.float32(0.37), np.float32(0.0), np.float32(1.3e-3), np.float32(0.0), np.float32(2.5e-5)]
    return [(b - a, coefs[i % len(coefs)]) for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4097, 3 * 8192 + 517])
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("update,lr_on_device", [(True, False), (True, True), (False, False)])
def test_optimizer_decay_op(n, shift, kind, update, lr_on_device):
    from sap3d_tensorflow_amd import ops
    name, nesterov = KINDS[kind]
    p, g, a = _inputs(n, n * 11 + shift)
    tiles = _tiles(n, shift)
    lr, mom = 3e-3, 0.9
    g2, p2, a2, term = ops.optimizer_decay(name, p, g, a, tiles, lr=lr, momentum=mom, use_nesterov=nesterov,
                                           lr_on_device=lr_on_device, update=update)
    c = np.concatenate([np.full(k, cf, np.float32) for k, cf in tiles])
    want_g = np.where(c != 0, reg_ref.decayed_grad32(g, c, p), g).astype(np.float32)
    assert _bits_equal(g2, want_g)
    if update:
        want_p, want_a = opt_ref.update32(kind, p, a, want_g, lr, mom)
        assert _bits_equal(p2, want_p) and _bits_equal(a2, want_a)
        # coefficient-0 tiles: the plain kernel's bits
        q_p, q_a = ops.optimizer(name, p, g, a, lr=lr, momentum=mom, use_nesterov=nesterov)
        z = c == 0
        assert _bits_equal(p2[z], q_p[z]) and _bits_equal(a2[z], q_a[z])
    else:
        assert _bits_equal(p2, p) and _bits_equal(a2, a)
    want_term = math.fsum(0.5 * float(cf) * float(x) ** 2 for cf, x in zip(c.astype(np.float64), p.astype(np.float64)))
    assert abs(term - want_term) <= n * EPS64 * max(abs(want_term), 1e-300)


# ---- whole steps -----------------------------------------------------------------------------------------------------------
CFG = p3d.NetConfig(base=16, blocks=(1, 2, 2))
SHAPE = (1, 16, 32, 32)


def _params(structure, cfg=CFG, seed=1):
    if structure.startswith("gn_"):
        from oracle import p3d_gn
        return {k: np.asarray(v, np.float32) for k, v in p3d_gn.init_params(seed, cfg, head=reg_ref.GN_HEADS[structure]).items()}
    return {k: np.asarray(v, np.float32) for k, v in p3d.init_params(seed, structure, cfg).items()}


def _session(structure="unet", cfg=CFG, shape=SHAPE, params=None, seed=1):
    from sap3d_tensorflow_amd import P3DSession
    B, T, H, W = shape
    s = P3DSession(structure, batch=B, frames=T, height=H, width=W, base=cfg.base, blocks=cfg.blocks, seed=seed)
    if params is not None:
        s.load(params)
    return s


def _data(shape=SHAPE):
    return p3d.synthetic_clip(0, shape + (3,)), p3d.synthetic_target(3, shape)


def test_adam_and_momentum_sessions_share_losses_and_gradients():
    params = _params("unet")
    x, y = _data()
    a, m = _session(params=params), _session(params=params)
    m.set_optimizer("momentum", lr=1e-3, momentum=0.9, use_nesterov=True)
    la, pa = a.backward(x, y, 0.0)
    lm, pm = m.backward(x, y, 0.0)
    assert la == lm and _bits_equal(pa, pm)
    for n, _, tr in a.variables():
        if tr:
            assert _bits_equal(a.get_grad(n), m.get_grad(n)), n
    a.close()
    m.close()


@pytest.mark.parametrize("structure,kind,decay", [("unet", "momentum", False), ("unet", "nesterov", False), ("unet", "sgd", False),
                                                  ("unet", "momentum", True), ("gn_p3d", "nesterov", True)])
def test_one_step_is_the_replay_of_its_gradient(structure, kind, decay):
    """After one train_step from zero slots every parameter is the replay of the gradient the step used (with a term on, the
    decayed gradient the fused launch writes back)."""
    name, nesterov = KINDS[kind]
    params = _params(structure)
    x, y = _data()
    s = _session(structure, params=params)
    lr, mom = 2e-3, 0.9
    s.set_optimizer(name, lr=lr, momentum=mom, use_nesterov=nesterov)
    if decay:
        s.set_regularization(("weightdecay",))
    s.train_step(x, y, dropout=0.0)
    assert s.optimizer_step() == 1
    for n, _, tr in s.variables():
        if not tr:
            continue
        g = s.get_grad(n)
        want_p, want_a = opt_ref.update32(kind, params[n], np.zeros_like(g), g, lr, mom)
        assert _bits_equal(s.get_param(n), want_p), n
        if name == "momentum":
            assert _bits_equal(s.get_slot(n, 0), want_a), n
    if decay:
        coef_any = [n for n, _, tr in s.variables() if tr and s.param_regularization(n)[0] != 0]
        assert coef_any
    s.close()


# ---- against float64 -------------------------------------------------------------------------------------------------------
def test_three_nesterov_steps_against_float64():
    """Three Momentum (Nesterov) steps at dropout 0 on test_gpu_net.SMALL[0] against the float64 update composed with the
    float64 oracle's gradients.  Each float64 gradient is taken at the session's own parameters of that step, so the two
    sides do not drift apart through the net's sensitivity to its parameters; what remains is the float32 gradients' error
    and the float32 update.  The tolerance comes from the session's own gradients: e = their largest relative L2 distance to
    the float64 ones over the three steps.  Every update is lr times a positive combination of the gradients, so the summed
    update may differ by e relative; we allow 2 e of its norm, plus the float32 storage of the parameters (each step rounds
    every parameter once, at most u |p|, u = 2^-24).  The losses are the forwards' (1e-4)."""
    from test_gpu_net import SMALL, make_session, randomise_norm_params
    cfg, shape = SMALL[0]
    p64 = randomise_norm_params(p3d.init_params(1, "unet", cfg, dtype=np.float64))
    p32 = {k: v.astype(np.float32) for k, v in p64.items()}
    x, y = _data(shape)
    s = make_session(cfg, shape, p32)
    lr, mom = 1e-3, 0.9
    s.set_optimizer("momentum", lr=lr, momentum=mom, use_nesterov=True)
    names = [n for n, _, tr in s.variables() if tr]
    cur = {n: p32[n].astype(np.float64) for n in names}
    acc = {n: np.zeros_like(cur[n]) for n in names}
    errs = []
    for k in range(3):
        at = {n: s.get_param(n).astype(np.float64) for n, _, _ in s.variables()}
        l32 = s.train_step(x, y, dropout=0.0)
        l64, _, g64, _ = p3d.loss_and_grads(at, x.astype(np.float64), y.astype(np.float64), 0.0, True, "unet", cfg, np.float64)
        assert abs(l32 - l64) <= 1e-4 * abs(l64), (k, l32, l64)
        d = np.concatenate([(s.get_grad(n).astype(np.float64) - g64[n]).ravel() for n in names])
        errs.append(np.linalg.norm(d) / np.linalg.norm(np.concatenate([g64[n].ravel() for n in names])))
        assert errs[-1] < 2e-2, errs       # (the float32 step's gradients: smoke() allows 2e-2 on the last deconv's)
        for n in names:
            cur[n], acc[n] = opt_ref.momentum64(cur[n], acc[n], g64[n], lr, mom, nesterov=True)
    e = max(errs)
    d32 = np.concatenate([(s.get_param(n).astype(np.float64) - p32[n]).ravel() for n in names])
    d64 = np.concatenate([(cur[n] - p32[n]).ravel() for n in names])
    p_norm = np.linalg.norm(np.concatenate([p32[n].ravel() for n in names]).astype(np.float64))
    err, tol = np.linalg.norm(d32 - d64), 2 * e * np.linalg.norm(d64) + 3 * 2.0 ** -24 * p_norm
    print("three nesterov steps: update error %.3g of %.3g (tolerance %.3g; gradient rel-L2 %s)"
          % (err, np.linalg.norm(d64), tol, ", ".join("%.3g" % v for v in errs)))
    assert err <= tol, (err, tol, errs)
    s.close()


# ---- the default path ------------------------------------------------------------------------------------------------------
def test_default_path_untouched():
    params = _params("unet")
    x, y = _data()
    fresh, toggled = _session(params=params), _session(params=params)
    toggled.set_optimizer("momentum", lr=1e-4, momentum=0.9)
    toggled.set_optimizer("adam", lr=1e-4)
    la, pa = fresh.backward(x, y, 0.0)
    lb, pb = toggled.backward(x, y, 0.0)
    assert la == lb and _bits_equal(pa, pb)
    for n, _, tr in fresh.variables():
        if tr:
            assert _bits_equal(fresh.get_grad(n), toggled.get_grad(n)), n
    for s in (fresh, toggled):
        s.upload(x, y)
        s.train_step_device(0.5, seed=0)
        s.synchronize()
    sa, sb = fresh.schedule(0.5, seed=1), toggled.schedule(0.5, seed=1)
    assert sa == sb
    toggled.set_optimizer("momentum", lr=1e-4, momentum=0.9)
    sc = toggled.schedule(0.5, seed=1)
    assert len(sc) == len(sa)
    changed = [(a, c) for a, c in zip(sa, sc) if a != c]
    assert len(changed) == sum(" adam_kernel" in ln for ln in sa) == 2
    for a, c in changed:
        assert c == a.replace(" adam_kernel", " momentum_kernel")
    toggled.set_optimizer("sgd", lr=1e-4)
    sd = toggled.schedule(0.5, seed=1)
    assert [a.replace(" adam_kernel", " sgd_kernel") for a in sa] == sd
    fresh.close()
    toggled.close()


def test_switching_kind_starts_fresh_and_same_kind_keeps_state():
    params = _params("unet")
    x, y = _data()
    s = _session(params=params)
    s.set_optimizer("momentum", lr=1e-3, momentum=0.9)
    s.train_step(x, y, dropout=0.0)
    n = [v for v, _, tr in s.variables() if tr][0]
    a = s.get_slot(n, 0)
    assert np.any(a != 0) and s.optimizer_step() == 1
    s.set_optimizer("momentum", lr=5e-4, momentum=0.5, use_nesterov=True)     # same kind: kept
    assert _bits_equal(s.get_slot(n, 0), a) and s.optimizer_step() == 1
    s.set_optimizer("adam", lr=1e-4)                                         # another kind: fresh
    assert s.optimizer_step() == 0
    assert not np.any(s.get_slot(n, 0)) and not np.any(s.get_slot(n, 1))
    s.close()


# ---- resume --------------------------------------------------------------------------------------------------------------
def _configure(s, kind, decay):
    s.set_adam(1e-3)
    if kind != "adam":
        name, nesterov = KINDS[kind]
        s.set_optimizer(name, lr=1e-3, momentum=0.9, use_nesterov=nesterov)
    if decay:
        s.set_regularization(("weightdecay",))


@pytest.mark.parametrize("kind", ["adam", "momentum"])
@pytest.mark.parametrize("decay", [False, True])
def test_resume_is_bit_identical(kind, decay, tmp_path):
    params = _params("unet")
    x, y = _data()
    a = _session(params=params)
    _configure(a, kind, decay)
    la = [a.train_step(x, y, dropout=0.5, seed=k) for k in range(4)]
    want = {n: a.get_param(n) for n, _, _ in a.variables()}
    a.close()
    b = _session(params=params)
    _configure(b, kind, decay)
    lb = [b.train_step(x, y, dropout=0.5, seed=k) for k in range(2)]
    prefix = b.save_checkpoint(str(tmp_path), 2, optimizer_state=True)
    b.close()
    c = _session(seed=7)
    _configure(c, kind, decay)
    c.restore(str(tmp_path), optimizer_state=True)
    assert c.optimizer_step() == (2 if kind == "adam" else 0)
    if kind == "adam":
        c_state = c.optimizer_state()
        assert c_state["beta2_power"] == np.float32(np.float64(np.float32(B2)) ** 3)
    lb += [c.train_step(x, y, dropout=0.5, seed=k) for k in range(2, 4)]
    assert la == lb
    for n, v in want.items():
        assert _bits_equal(c.get_param(n), v), n
    c.close()
    from sap3d_tensorflow_amd import tf_checkpoint as tfc
    keys = set(k for k, _, _ in tfc.list_variables(prefix))
    suffix = "/Adam" if kind == "adam" else "/Momentum"
    assert any(k.endswith(suffix) for k in keys) and (("beta1_power" in keys) == (kind == "adam"))


def test_tf_style_adam_state_at_step_1000(tmp_path):
    """A bundle as a default TF Saver writes it after 1000 Adam steps (slots and running float32 powers) restores to step 1000,
    and the next step is Adam's step 1001."""
    from sap3d_tensorflow_amd import ops, tf_checkpoint as tfc
    params = _params("unet")
    x, y = _data()
    s = _session(params=params)
    s.set_adam(1e-3)
    rng = np.random.default_rng(4)
    bundle = dict(params)
    slots = {}
    for n, shp, tr in s.variables():
        if tr:
            slots[n] = ((rng.standard_normal(shp) * 1e-3).astype(np.float32), (rng.random(shp) * 1e-6).astype(np.float32))
            bundle[n + "/Adam"], bundle[n + "/Adam_1"] = slots[n]
    b1p, b2p = opt_ref.tf_running_powers(1000, B1, B2)
    bundle["beta1_power"], bundle["beta2_power"] = np.array(b1p), np.array(b2p)
    tfc.write_checkpoint(str(tmp_path / "p3d_1000.ckpt"), bundle)
    s.close()
    s = _session(seed=3)
    s.set_adam(1e-3)
    s.restore(str(tmp_path / "p3d_1000.ckpt"), optimizer_state=True)
    assert s.optimizer_step() == 1000
    for n, (m, v) in slots.items():
        assert _bits_equal(s.get_slot(n, 0), m) and _bits_equal(s.get_slot(n, 1), v), n
    s.backward(x, y, 0.0)
    grads = {n: s.get_grad(n) for n in slots}
    s.train_step(x, y, dropout=0.0)
    z = np.zeros(4, np.float32)
    lr_t = ops.adam(z, z, z, z, 1001, 1e-3, B1, B2, EPS)[3]
    assert lr_t != ops.adam(z, z, z, z, 1, 1e-3, B1, B2, EPS)[3]
    for n, (m, v) in slots.items():
        assert _bits_equal(grads[n], s.get_grad(n)), n
        wp, wm, wv = reg_ref.adam32(params[n], m, v, grads[n], lr_t, B1, B2, EPS, True)
        assert _bits_equal(s.get_param(n), wp) and _bits_equal(s.get_slot(n, 0), wm) and _bits_equal(s.get_slot(n, 1), wv), n
    assert s.optimizer_step() == 1001
    s.close()


def test_restore_without_optimizer_state_ignores_the_slots(tmp_path):
    params = _params("unet")
    x, y = _data()
    a = _session(params=params)
    a.set_optimizer("momentum", lr=1e-3)
    a.train_step(x, y, dropout=0.0)
    a.save_checkpoint(str(tmp_path), 1, optimizer_state=True)
    a.close()
    b = _session(seed=2)
    b.set_optimizer("momentum", lr=1e-3)
    b.restore(str(tmp_path))
    assert b.optimizer_step() == 0
    for n, _, tr in b.variables():
        if tr:
            assert not np.any(b.get_slot(n, 0)), n
    # the bundle without slots: optimizer_state=True refuses it before setting anything
    c = _session(seed=2)
    c.save_checkpoint(str(tmp_path / "plain"), 1)
    c.set_optimizer("momentum", lr=1e-3)
    with pytest.raises(KeyError):
        c.restore(str(tmp_path / "plain"), optimizer_state=True)
    b.close()
    c.close()


# ---- schedule, data parallel and capture ----------------------------------------------------------------------------------
def test_one_rank_communicator_trajectory_and_schedule(monkeypatch):
    from sap3d_tensorflow_amd import P3DSession
    from test_gpu_schedule import happens_before, ordered, parse
    monkeypatch.setenv("P3D_BUCKET_MB", "1")
    cfg, shape = p3d.NetConfig(base=16, blocks=(1, 1, 2)), (2, 16, 32, 32)
    x, y = _data(shape)

    def run(with_comm):
        s = _session("unet", cfg, shape, seed=1)
        if with_comm:
            s.comm_init(P3DSession.comm_unique_id())
        s.set_optimizer("momentum", lr=1e-3, momentum=0.9, use_nesterov=True)
        losses = [s.train_step(x, y, dropout=0.5, seed=k) for k in range(3)]
        ps = {n: s.get_param(n) for n, _, _ in s.variables()}
        sched = s.schedule(0.5, seed=4) if with_comm else None
        s.close()
        return losses, ps, sched

    la, pa, _ = run(False)
    lb, pb, sched = run(True)
    assert la == lb
    for n in pa:
        assert _bits_equal(pa[n], pb[n]), n
    ops = parse(sched)
    streams, clocks = happens_before(ops)
    pos, count = [], {st: 0 for st in streams}
    for _, st, _ in ops:
        count[st] += 1
        pos.append(count[st])
    parts = [i for i, op in enumerate(ops) if op[0] == "L" and op[2].startswith("momentum_kernel")]
    assert len(parts) == 2 and not any(op[0] == "L" and op[2].startswith("adam_kernel") for op in ops)
    reduces = [i for i, op in enumerate(ops) if op[0] == "C" and "allreduce" in op[2]]
    assert reduces
    for d in parts:
        for r in reduces:
            if r < d:
                assert ordered(r, d, ops, clocks, pos), (ops[r], ops[d])
    assert all(ordered(r, parts[-1], ops, clocks, pos) for r in reduces)


_CAPTURE = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, %(root)r)
from oracle import p3d
from sap3d_tensorflow_amd import P3DSession
cfg, shape = p3d.NetConfig(base=16, blocks=(1, 1, 2)), (1, 16, 32, 32)
s = P3DSession("unet", batch=shape[0], frames=shape[1], height=shape[2], width=shape[3], base=cfg.base, blocks=cfg.blocks, seed=1)
s.set_adam(1e-3)
s.upload(p3d.synthetic_clip(0, shape + (3,)), p3d.synthetic_target(3, shape))
out = []
plan = [("adam", 0.9, False), ("adam", 0.9, False), ("momentum", 0.9, False), ("momentum", 0.5, True), ("momentum", 0.5, True),
        ("sgd", 0.9, False), ("sgd", 0.9, False)]
for k, (kind, mom, nest) in enumerate(plan):
    s.set_optimizer(kind, lr=1e-3, momentum=mom, use_nesterov=nest)
    s.train_step_device(0.5, seed=k)
    s.synchronize()
    h = hashlib.sha256()
    for n, _, _ in s.variables():
        h.update(s.get_param(n).tobytes())
    out.append("%%r %%d %%s" %% (s.last_loss(), s.optimizer_step(), h.hexdigest()))
s.close()
print("\n".join(out))
"""


def test_captured_step_follows_the_optimizer_switch():
    res = {}
    for graph in ("0", "1"):
        env = dict(os.environ, P3D_GRAPH=graph)
        r = subprocess.run([sys.executable, "-c", _CAPTURE % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        res[graph] = r.stdout.split("\n")[:7]
    assert res["0"] == res["1"]
    steps = [int(ln.split()[1]) for ln in res["0"]]
    assert steps == [1, 2, 1, 2, 3, 1, 2]
    assert len(set(ln.split()[2] for ln in res["0"])) == 7          # every step moved the parameters


# ---- refusals and driver ---------------------------------------------------------------------------------------------------
def test_refusals():
    from sap3d_tensorflow_amd import P3dError
    from sap3d_tensorflow_amd._lib import fptr, lib
    s = _session()
    h = s._h
    for args in ((3, 1e-3, 0.9, 0), (-1, 1e-3, 0.9, 0), (1, float("nan"), 0.9, 0), (1, float("inf"), 0.9, 0),
                 (1, 1e-3, float("nan"), 0), (1, 1e-3, -0.1, 0)):
        assert lib().p3d_set_optimizer(h, *args) == -1, args
        assert lib().p3d_last_error().decode()
    assert s.optimizer_step() == 0
    tr = [(n, shp) for n, shp, t in s.variables() if t]
    st = [(n, shp) for n, shp, t in s.variables() if not t]
    n, shp = tr[0]
    buf = np.zeros(shp, np.float32)
    assert lib().p3d_get_slot(h, n.encode(), 2, fptr(buf), buf.size) == -1          # Adam has slots 0, 1
    assert lib().p3d_get_slot(h, n.encode(), 0, fptr(buf), buf.size + 1) == -1      # wrong count
    assert lib().p3d_get_slot(h, b"no/such/var", 0, fptr(buf), buf.size) == -1
    if st:
        sn, sshp = st[0]
        sb = np.zeros(sshp, np.float32)
        assert lib().p3d_get_slot(h, sn.encode(), 0, fptr(sb), sb.size) == -1       # not trainable
        assert "not trainable" in lib().p3d_last_error().decode()
    s.set_optimizer("momentum", lr=1e-3)
    assert lib().p3d_set_slot(h, n.encode(), 1, fptr(buf), buf.size) == -1          # Momentum has slot 0 only
    s.set_optimizer("sgd", lr=1e-3)
    assert lib().p3d_get_slot(h, n.encode(), 0, fptr(buf), buf.size) == -1          # SGD has none
    assert lib().p3d_set_optimizer_step(h, -1) == -1
    with pytest.raises(ValueError):
        s.set_optimizer("rmsprop")
    with pytest.raises(P3dError):
        s.set_optimizer("momentum", lr=1e-3, momentum=-1.0)
    z = np.zeros(8, np.float32)
    assert lib().p3d_debug_optimizer(0, 0, fptr(z), fptr(z), fptr(z), 8, 0, 1e-3, 0.9, 0, 0) == -1    # Adam: its own hook
    from sap3d_tensorflow_amd import ops
    with pytest.raises(P3dError):           # the fused launch needs a 16-byte aligned base, as adam_decay's
        ops.optimizer_decay("momentum", z, z, z, [(8, 0.5)], offset=1)
    s.close()


def test_driver_momentum_resume(tmp_path):
    from sap3d_tensorflow_amd import tf_checkpoint as tfc
    drv = os.path.join(ROOT, "drivers", "train.py")
    small = ["--batch", "2", "--imagesize", "32", "32", "--validiter", "100", "--plotiter", "1"]
    opt = ["--optimizer", "momentum", "--nesterov", "--optimizer-state"]
    r = subprocess.run([sys.executable, drv, "--steps", "2", "--saveiter", "2", "--info", "first"] + opt + small,
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    model = tmp_path / "model" / "first"
    prefix = tfc.latest_checkpoint(str(model))
    names = [k for k, _, _ in tfc.list_variables(prefix)]
    mom = [k for k in names if k.endswith("/Momentum")]
    assert mom and not any(k.endswith("/Adam") for k in names)
    assert any(np.any(v != 0) for v in tfc.read_checkpoint(prefix, names=set(mom[:5])).values())
    r = subprocess.run([sys.executable, drv, "--steps", "2", "--saveiter", "100", "--info", "second", "--pretrain", str(model)]
                       + opt + small, cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "Using this model to retrain" in r.stdout
    r = subprocess.run([sys.executable, drv, "--steps", "1", "--nesterov"] + small, cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=900)
    assert r.returncode != 0 and "--nesterov" in (r.stdout + r.stderr)
