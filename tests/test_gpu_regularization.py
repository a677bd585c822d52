"""The regularisation option (P3DSession.set_regularization) on the GPU: the fused decay + Adam launch at op level
(p3d_debug_adam_decay) against a float32 replay bit for bit, the library's tagging against the sets recorded from the oracle's
graph builders (tests/reg_ref.py), whole steps against the plain step, the float64 oracle, the default path, data parallelism
and the captured step.  Scales restated from the reference: weight decay wd = 0.001 (p3d.py:10-16) on the BatchNorm nets and
0.0005 (gn/p3d_gn.py:54-60) on the GroupNorm nets, averaged over the kernels get_conv_weight makes with wd != 0
(train.py:161, gn/train_p3d_gn_dataset.py:188); l2 = 0.0005 * l2_loss averaged over the kernel_regularizer kernels of scope
P3D (gn/p3d_gn.py:11-21,538; gn/train_p3d_gn_dataset.py:189)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from oracle import p3d          # noqa: E402
import reg_ref                  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(HERE)
EPS64 = np.finfo(np.float64).eps
B1, B2, EPS = 0.9, 0.999, 1e-8


# ---- op level ------------------------------------------------------------------------------------------------------------
def _tiles(n, shift):
    """Cut [0, n) into tiles whose offsets fall at `shift` and shift + 1 modulo 4 (mid-4-group for shift != 0), coefficient 0
    next to non-zero ones, and at 8192 for long lengths."""
    k1, k2 = (n // 3) // 4 * 4 + shift, ((2 * n) // 3) // 4 * 4 + shift + 1
    cuts = sorted({0, n} | {k for k in (k1, k2) if 0 < k < n} | set(range(8192 + shift, n, 8192)))
    coefs = [np.float32(0.37), np.float32(0.0), np.float32(1.3e-3), np.float32(0.0), np.float32(2.5e-5)]
    return [(b - a, coefs[i % len(coefs)]) for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]


def _inputs(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 0.1).astype(np.float32)
    m = (rng.standard_normal(n) * 0.01).astype(np.float32)
    v = (rng.random(n) * 1e-3).astype(np.float32)
    return p, g, m, v


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1021, 4096, 3 * 8192 + 517])
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("update,lr_on_device", [(True, False), (True, True), (False, False)])
def test_adam_decay_op(n, shift, update, lr_on_device):
    """Tile offsets at every residue modulo 4; the buffers start 16-byte aligned, as p3d_adam requires."""
    from sap3d_tensorflow_amd import ops
    offset = 0
    p, g, m, v = _inputs(n, n * 7 + shift)
    tiles = _tiles(n, shift)
    t = 3
    a = ops.adam_decay(p, g, m, v, tiles, t, 1e-3, B1, B2, EPS, lr_on_device=lr_on_device, update=update, offset=offset)
    b = ops.adam_decay(p, g, m, v, tiles, t, 1e-3, B1, B2, EPS, lr_on_device=lr_on_device, update=update, offset=offset)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert a[4] == b[4]
    g2, p2, m2, v2, term, lr_t = a
    c = np.concatenate([np.full(k, cf, np.float32) for k, cf in tiles])
    want_g = np.where(c != 0, reg_ref.decayed_grad32(g, c, p), g).astype(np.float32)
    assert np.array_equal(g2.view(np.uint32), want_g.view(np.uint32))
    if update:
        whole = (np.arange(n) & ~3) + 3 < n
        wp, wm, wv = reg_ref.adam32(p, m, v, want_g, lr_t, B1, B2, EPS, whole)
        for got, want in ((p2, wp), (m2, wm), (v2, wv)):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        # coefficient-0 tiles: adam_kernel's bits (p3d_debug_adam over the same range)
        q = ops.adam(p, g, m, v, t, 1e-3, B1, B2, EPS, lr_on_device=lr_on_device, offset=offset)
        z = c == 0
        for got, want in ((p2, q[0]), (m2, q[1]), (v2, q[2])):
            assert np.array_equal(got[z].view(np.uint32), want[z].view(np.uint32))
    else:
        for got, want in ((p2, p), (m2, m), (v2, v)):
            assert np.array_equal(got, want)
    want_term = math.fsum(0.5 * float(cf) * float(x) ** 2 for cf, x in zip(c.astype(np.float64), p.astype(np.float64)))
    assert abs(term - want_term) <= n * EPS64 * max(abs(want_term), 1e-300)


def test_adam_decay_refuses_a_misaligned_base():
    """Like p3d_adam, the launch moves four elements at a time from a 16-byte aligned base: buffers 1-3 elements in are refused."""
    from sap3d_tensorflow_amd import P3dError, ops
    p = np.ones(16, np.float32)
    for off in (1, 2, 3):
        with pytest.raises(P3dError):
            ops.adam_decay(p, p, p, p, [(16, 0.5)], 1, offset=off)
    ops.adam_decay(p, p, p, p, [(16, 0.5)], 1, offset=0)


# ---- sessions --------------------------------------------------------------------------------------------------------------
CFG = p3d.NetConfig(base=16, blocks=(1, 2, 2))
SHAPE = (1, 16, 32, 32)
STRUCTURES = ("unet", "concat", "unet++nonsa", "unet++ds", "gn_p3d", "gn_p3d_concat", "gn_p3d_decoder")


def _session(structure, cfg=CFG, shape=SHAPE, params=None, seed=1):
    from sap3d_tensorflow_amd import P3DSession
    B, T, H, W = shape
    s = P3DSession(structure, batch=B, frames=T, height=H, width=W, base=cfg.base, blocks=cfg.blocks, seed=seed)
    if params is not None:
        s.load(params)
    return s


@pytest.mark.parametrize("structure", STRUCTURES)
def test_tagging_matches_the_recorded_sets(structure, monkeypatch):
    from sap3d_tensorflow_amd import P3dError
    wd_names, l2_names, _ = reg_ref.recorded_sets(structure, CFG, monkeypatch)
    gn = structure.startswith("gn_")
    s = _session(structure)
    names = [n for n, _, tr in s.variables() if tr]
    for n in names:
        assert s.param_regularization(n) == (0.0, 0.0)          # off by default
    if structure == "gn_p3d_decoder":
        terms = ("weightdecay", "l2")
    else:
        terms = ("weightdecay",)
        with pytest.raises(P3dError):
            s.set_regularization(("l2",))
        with pytest.raises(P3dError):
            s.set_regularization(("weightdecay", "l2"))
    s.set_regularization(terms)
    coef_wd = reg_ref.coefficients(wd_names, l2_names, ("weightdecay",), gn=gn)
    coef_l2 = reg_ref.coefficients(wd_names, l2_names, ("l2",), gn=gn) if "l2" in terms else {}
    assert set(coef_wd) <= set(names) and set(coef_l2) <= set(names)
    for n in names:
        cw, cl = s.param_regularization(n)
        assert cw == coef_wd.get(n, np.float32(0)), n
        assert cl == coef_l2.get(n, np.float32(0)), n
    # an explicit scale is taken as the float32 it is
    s.set_regularization(("weightdecay",), wd=0.25)
    n0 = wd_names[0]
    assert s.param_regularization(n0)[0] == np.float32(float(np.float32(0.25)) / len(wd_names))
    s.close()


STEP_CASES = [("unet", ("weightdecay",)), ("concat", ("weightdecay",)), ("unet++ds", ("weightdecay",)),
              ("gn_p3d", ("weightdecay",)), ("gn_p3d_decoder", ("weightdecay", "l2"))]


def _params(structure, cfg=CFG, seed=1):
    if structure.startswith("gn_"):
        from oracle import p3d_gn
        return p3d_gn.init_params(seed, cfg, head=reg_ref.GN_HEADS[structure])
    return p3d.init_params(seed, structure, cfg)


def _ulp32(x):
    x = np.float32(abs(x))
    return float(np.nextafter(x, np.float32(np.inf)) - x)


@pytest.mark.parametrize("structure,terms", STEP_CASES)
def test_whole_step_against_the_plain_step(structure, terms, monkeypatch):
    wd_names, l2_names, _ = reg_ref.recorded_sets(structure, CFG, monkeypatch)
    coef = reg_ref.coefficients(wd_names, l2_names, terms, gn=structure.startswith("gn_"))
    params = {k: np.asarray(v, np.float32) for k, v in _params(structure).items()}
    x = p3d.synthetic_clip(0, SHAPE + (3,))
    y = p3d.synthetic_target(3, SHAPE)
    term = reg_ref.term64(params, coef)
    off, on = _session(structure, params=params), _session(structure, params=params)
    names = [n for n, _, tr in off.variables() if tr]
    on.set_regularization(terms)
    for s in (off, on):
        s.set_adam(1e-3)
    # backward: the gradient-only mode
    l_off, pr_off = off.backward(x, y, 0.0)
    l_on, pr_on = on.backward(x, y, 0.0)
    assert np.array_equal(pr_off, pr_on)
    got_term = on.last_regularization()
    assert abs(got_term - term) <= 1e6 * EPS64 * term                # a sum of ~1e5 squares per variable, in double
    assert abs((l_on - l_off) - term) <= 2 * _ulp32(l_on) + 1e6 * EPS64 * term
    for n in names:
        a, b = off.get_grad(n), on.get_grad(n)
        want = reg_ref.decayed_grad32(a, coef[n], params[n]) if n in coef else a
        assert np.array_equal(b.view(np.uint32), want.view(np.uint32)), n
    # one train step: decay + Adam fused; everything else bit-identical
    l_off = off.train_step(x, y, dropout=0.0)
    l_on = on.train_step(x, y, dropout=0.0)
    assert abs(on.last_regularization() - got_term) == 0.0            # same parameters before the update, same fold
    assert abs((l_on - l_off) - term) <= 2 * _ulp32(l_on) + 1e6 * EPS64 * term
    from sap3d_tensorflow_amd import ops
    lr_t = ops.adam(np.zeros(4, np.float32), np.zeros(4, np.float32), np.zeros(4, np.float32), np.zeros(4, np.float32), 1,
                    1e-3, B1, B2, EPS)[3]
    zero = None
    for n in names:
        ga, gb = off.get_grad(n), on.get_grad(n)
        pa, pb = off.get_param(n), on.get_param(n)
        if n not in coef:
            assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), n
            assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)), n
            continue
        want_g = reg_ref.decayed_grad32(ga, coef[n], params[n])
        assert np.array_equal(gb.view(np.uint32), want_g.view(np.uint32)), n
        zero = np.zeros(want_g.shape, np.float32)
        wp, _, _ = reg_ref.adam32(params[n], zero, zero, want_g, lr_t, B1, B2, EPS, True)
        assert np.array_equal(pb.view(np.uint32), wp.view(np.uint32)), n
    assert zero is not None
    off.close()
    on.close()


# ---- against the float64 oracle --------------------------------------------------------------------------------------------
def test_regularised_backward_against_the_oracle_unet(monkeypatch):
    from gates import grad_gate
    from test_gpu_net import SMALL, grads_vs_oracles, make_session, randomise_norm_params
    cfg, shape = SMALL[0]
    wd_names, l2_names, _ = reg_ref.recorded_sets("unet", cfg, monkeypatch)
    coef = reg_ref.coefficients(wd_names, l2_names, ("weightdecay",))
    p64 = randomise_norm_params(p3d.init_params(1, 'unet', cfg, dtype=np.float64))
    p32 = {k: v.astype(np.float32) for k, v in p64.items()}
    x = p3d.synthetic_clip(0, shape + (3,))
    y = p3d.synthetic_target(3, shape)
    l64, _, g64, _ = p3d.loss_and_grads(p64, x.astype(np.float64), y.astype(np.float64), 0.0, True, 'unet', cfg, np.float64)
    _, _, g32, _ = p3d.loss_and_grads(dict(p32), x, y, 0.0, True, 'unet', cfg, np.float32)
    r64, r32 = reg_ref.grad64(p64, coef), reg_ref.grad64(p32, coef)
    for n in coef:
        g64[n] = g64[n] + r64[n]
        g32[n] = g32[n] + r32[n]
    s = make_session(cfg, shape, p32)
    s.set_regularization(("weightdecay",))
    loss, _ = s.backward(x, y, 0.0)
    want = l64 + reg_ref.term64(p64, coef)
    assert abs(loss - want) < 1e-5 * abs(want)
    grad_gate("backward_small/base%d_%s" % (cfg.base, "x".join(map(str, shape))), *grads_vs_oracles(s, g64, g32))
    s.close()


def test_regularised_backward_against_the_oracle_gn_decoder(monkeypatch):
    from gates import grad_gate
    from oracle import p3d_gn
    from test_gpu_net import GN_DECODER, _gn_params, make_session, rel_l2
    cfg, shape = GN_DECODER[0]
    terms = ("weightdecay", "l2")
    wd_names, l2_names, _ = reg_ref.recorded_sets("gn_p3d_decoder", cfg, monkeypatch)
    coef = reg_ref.coefficients(wd_names, l2_names, terms, gn=True)
    p64 = _gn_params(cfg, np.float64, 'decoder')
    p32 = {k: v.astype(np.float32) for k, v in p64.items()}
    x = p3d.synthetic_clip(0, shape + (3,))
    y = p3d.synthetic_target(3, shape)
    s = make_session(cfg, shape, p32, 'gn_p3d_decoder')
    s.forward(x, 0.0, False)
    base = s.activation('decoder2_conv2')
    s.backward(x, y, dropout=0.5, seed=11)
    dropped = s.activation('decoder2_conv2')
    keep = np.where(base != 0, dropped != 0, True)
    l64, _, g64, _ = p3d_gn.loss_and_grads(p64, x.astype(np.float64), y.astype(np.float64), 0.5, True, cfg, np.float64,
                                           head='decoder', keep_mask=keep.astype(np.float64))
    _, _, g32, _ = p3d_gn.loss_and_grads(dict(p32), x, y, 0.5, True, cfg, np.float32, head='decoder',
                                         keep_mask=keep.astype(np.float32))
    r64, r32 = reg_ref.grad64(p64, coef), reg_ref.grad64(p32, coef)
    for n in coef:
        g64[n] = g64[n] + r64[n]
        g32[n] = g32[n] + r32[n]
    s.set_regularization(terms)
    loss, _ = s.backward(x, y, dropout=0.5, seed=11)
    want = l64 + reg_ref.term64(p64, coef)
    assert abs(loss - want) < 1e-5 * abs(want)
    scale = np.median([np.linalg.norm(v) for v in g64.values()])
    floor = 1e-2 * scale
    grad_gate("gn_decoder/base%d_%s" % (cfg.base, "x".join(map(str, shape))), {n: rel_l2(s.get_grad(n), w, floor) for n, w in g64.items()},
              {n: rel_l2(g32[n], w, floor) for n, w in g64.items()})
    s.close()


# ---- the default path ------------------------------------------------------------------------------------------------------
def test_default_path_untouched():
    params = {k: np.asarray(v, np.float32) for k, v in _params("unet").items()}
    x = p3d.synthetic_clip(0, SHAPE + (3,))
    y = p3d.synthetic_target(3, SHAPE)
    fresh, toggled = _session("unet", params=params), _session("unet", params=params)
    toggled.set_regularization(("weightdecay",))
    toggled.set_regularization(())
    la, pa = fresh.backward(x, y, 0.0)
    lb, pb = toggled.backward(x, y, 0.0)
    assert la == lb and np.array_equal(pa, pb)
    assert toggled.last_regularization() == 0.0
    for n, _, tr in fresh.variables():
        if not tr:
            continue
        assert np.array_equal(fresh.get_grad(n).view(np.uint32), toggled.get_grad(n).view(np.uint32)), n
    for s in (fresh, toggled):
        s.upload(x, y)
        s.train_step_device(0.5, seed=0)
        s.synchronize()
    sa, sb = fresh.schedule(0.5, seed=1), toggled.schedule(0.5, seed=1)
    assert sa == sb
    toggled.set_regularization(("weightdecay",))
    sc = toggled.schedule(0.5, seed=1)
    assert len(sc) == len(sa)
    changed = [(a, c) for a, c in zip(sa, sc) if a != c]
    assert len(changed) == sum(" adam_kernel" in ln for ln in sa) >= 1
    for a, c in changed:
        assert " adam_kernel" in a and c == a.replace(" adam_kernel", " adam_decay_kernel")
    fresh.close()
    toggled.close()


# ---- schedule and data parallelism -----------------------------------------------------------------------------------------
def test_one_rank_communicator_trajectory_and_schedule(monkeypatch):
    from sap3d_tensorflow_amd import P3DSession
    from test_gpu_schedule import happens_before, ordered, parse
    monkeypatch.setenv("P3D_BUCKET_MB", "1")
    cfg, shape = p3d.NetConfig(base=16, blocks=(1, 1, 2)), (2, 16, 32, 32)
    x = p3d.synthetic_clip(0, shape + (3,))
    y = p3d.synthetic_target(3, shape)

    def run(with_comm):
        s = _session("unet", cfg, shape, seed=1)
        if with_comm:
            s.comm_init(P3DSession.comm_unique_id())
        s.set_adam(1e-3)
        s.set_regularization(("weightdecay",))
        losses = [s.train_step(x, y, dropout=0.5, seed=k) for k in range(3)]
        terms = s.last_regularization()
        ps = {n: s.get_param(n) for n, _, _ in s.variables()}
        sched = s.schedule(0.5, seed=4) if with_comm else None
        s.close()
        return losses, terms, ps, sched

    la, ta, pa, _ = run(False)
    lb, tb, pb, sched = run(True)
    assert la == lb and ta == tb
    for n in pa:
        assert np.array_equal(pa[n].view(np.uint32), pb[n].view(np.uint32)), n
    ops = parse(sched)
    streams, clocks = happens_before(ops)
    pos, count = [], {st: 0 for st in streams}
    for _, st, _ in ops:
        count[st] += 1
        pos.append(count[st])
    decay = [i for i, op in enumerate(ops) if op[0] == "L" and op[2].startswith("adam_decay_kernel")]
    assert len(decay) == 2 and not any(op[0] == "L" and op[2].startswith("adam_kernel") for op in ops)
    reduces = [i for i, op in enumerate(ops) if op[0] == "C" and "allreduce" in op[2]]
    assert reduces
    for d in decay:
        # a range is handed to the all-reduce before its optimiser part is enqueued: each part follows every all-reduce
        # issued before it, the last part follows all of them
        for r in reduces:
            if r < d:
                assert ordered(r, d, ops, clocks, pos), (ops[r], ops[d])
    assert all(ordered(r, decay[-1], ops, clocks, pos) for r in reduces)


# ---- captured step ---------------------------------------------------------------------------------------------------------
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
for k, terms in enumerate([(), (), ("weightdecay",), ("weightdecay",), (), ()]):
    s.set_regularization(terms)
    s.train_step_device(0.5, seed=k)
    s.synchronize()
    h = hashlib.sha256()
    for n, _, _ in s.variables():
        h.update(s.get_param(n).tobytes())
    out.append("%%r %%r %%s" %% (s.last_loss(), s.last_regularization(), h.hexdigest()))
s.close()
print("\n".join(out))
"""


def test_captured_step_follows_the_regularization_switch():
    res = {}
    for graph in ("0", "1"):
        env = dict(os.environ, P3D_GRAPH=graph)
        r = subprocess.run([sys.executable, "-c", _CAPTURE % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        res[graph] = r.stdout.split("\n")[:6]
    assert res["0"] == res["1"]
    regs = [float(ln.split()[1]) for ln in res["0"]]
    assert regs[0] == regs[1] == 0.0 and regs[2] > 0 and regs[3] > 0 and regs[4] == regs[5] == 0.0


# ---- driver ----------------------------------------------------------------------------------------------------------------
def test_driver_regularization(tmp_path):
    drv = os.path.join(ROOT, "drivers", "train.py")
    small = ["--batch", "2", "--imagesize", "32", "32", "--validiter", "100", "--saveiter", "100"]
    r = subprocess.run([sys.executable, drv, "--regularization", "both", "--steps", "1"] + small, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode != 0 and "kernel_regularizer" in (r.stderr + r.stdout)
    r = subprocess.run([sys.executable, drv, "--regularization", "weightdecay", "--steps", "2", "--plotiter", "1"] + small,
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
