"""The moving average of the weights (P3DSession.set_ema) on the GPU: ema_kernel at op level against the bit-exact float32 replay
of ema_ref.py, whole steps, the untouched trajectory, the schedule, warm-up, the swap, checkpoints, the captured step, a one-rank
communicator, the refusals and the drivers."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from oracle import p3d          # noqa: E402
import ema_ref                  # noqa: E402
import reg_ref                  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(HERE)
CFG = p3d.NetConfig(base=16, blocks=(1, 2, 2))      # the tiny net of test_gpu_optimizer.py
SHAPE = (1, 16, 32, 32)
f32 = np.float32


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


def _params(structure, cfg=CFG, seed=1):
    if structure.startswith("gn_"):
        from oracle import p3d_gn
        return {k: np.asarray(v, f32) for k, v in p3d_gn.init_params(seed, cfg, head=reg_ref.GN_HEADS[structure]).items()}
    return {k: np.asarray(v, f32) for k, v in p3d.init_params(seed, structure, cfg).items()}


def _session(structure="unet", cfg=CFG, shape=SHAPE, params=None, seed=1):
    from sap3d_tensorflow_amd import P3DSession
    B, T, H, W = shape
    s = P3DSession(structure, batch=B, frames=T, height=H, width=W, base=cfg.base, blocks=cfg.blocks, seed=seed)
    if params is not None:
        s.load(params)
    return s


def _data(shape=SHAPE):
    return p3d.synthetic_clip(0, shape + (3,)), p3d.synthetic_target(3, shape)


def _trainables(s):
    return [n for n, _, tr in s.variables() if tr]


def _shadows(s):
    return {n: s.get_ema(n) for n in _trainables(s)}


def _all_params(s):
    return {n: s.get_param(n) for n, _, _ in s.variables()}


# ---- 1: op level -----------------------------------------------------------------------------------------------------------
def _op_inputs(n, seed):
    """Random shadows and parameters with a few denormals, s == p elements and pairs whose product (s - p) * om underflows."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(n).astype(f32)
    p = (s + rng.standard_normal(n).astype(f32) * f32(0.1)).astype(f32)
    k = np.arange(n)
    s[k % 7 == 1] = f32(3e-41)                       # denormal shadows
    p[k % 11 == 2] = f32(-7e-42)                     # denormal parameters
    p[k % 5 == 3] = s[k % 5 == 3]                    # s == p
    tiny = k % 13 == 4
    s[tiny] = f32(2e-38)                             # s - p = 1e-38 (normal), times om < 1e-1: a denormal or zero product
    p[tiny] = f32(1e-38)
    gone = k % 17 == 5
    s[gone] = f32(3e-45)                             # (s - p) * om rounds to zero
    p[gone] = f32(0.0)
    return s, p


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4097, 2 ** 20 + 3])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("om_on_device", [False, True])
def test_ema_op(n, offset, om_on_device):
    """Offsets 1-3 start the range mid-16-byte line: head elements one by one, float4 groups, the cut last group one by one, all
    with the same arithmetic.  The caller's arrays carry one element more on each side than the launch is given, and the hook
    itself surrounds the device range with guard elements and fails if the launch touched one."""
    from sap3d_tensorflow_amd._lib import check, fptr, lib
    s, p = _op_inputs(n + 2, n * 3 + offset)
    om = ema_ref.om_const(0.999) if n % 2 else ema_ref.om_warmup(0.999, 3)
    got = s.copy()
    inner = got[1:n + 1]                             # a view: the hook writes n elements at got + 1
    assert inner.ctypes.data == got.ctypes.data + 4
    check(lib().p3d_debug_ema(0, fptr(inner), fptr(p[1:n + 1]), n, offset, float(om), 1 if om_on_device else 0))
    want = ema_ref.update32(s[1:n + 1], p[1:n + 1], om)
    assert _bits_equal(got[1:n + 1], want)
    assert _bits_equal(got[[0, n + 1]], s[[0, n + 1]])          # the guards on each side
    same = s[1:n + 1] == p[1:n + 1]
    if same.any():
        assert _bits_equal(got[1:n + 1][same], s[1:n + 1][same])


def test_ema_op_through_ops():
    from sap3d_tensorflow_amd import ops
    s, p = _op_inputs(777, 5)
    assert _bits_equal(ops.ema(s, p, ema_ref.om_const(0.9), offset=2), ema_ref.update32(s, p, ema_ref.om_const(0.9)))


# ---- 2: whole steps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("structure", ["unet", "gn_p3d"])
def test_three_steps_are_the_replay(structure):
    from sap3d_tensorflow_amd._lib import fptr, lib
    params = _params(structure)
    x, y = _data()
    s = _session(structure, params=params)
    s.set_adam(1e-3)
    s.set_ema(0.9)
    om = ema_ref.om_const(0.9)
    prev = _shadows(s)
    for n in prev:
        assert _bits_equal(prev[n], params[n]), n                # seeded from the variables
    for k in range(3):
        s.train_step(x, y, dropout=0.5, seed=k)
        cur = _shadows(s)
        moved = 0
        for n in cur:
            assert _bits_equal(cur[n], ema_ref.update32(prev[n], s.get_param(n), om)), (k, n)
            moved += int(not _bits_equal(cur[n], prev[n]))
        assert moved
        prev = cur
    states = [(n, shp) for n, shp, tr in s.variables() if not tr]
    if structure == "unet":
        assert any(n.endswith("moving_mean") for n, _ in states) and any(n.endswith("moving_variance") for n, _ in states)
    for n, shp in states:
        buf = np.zeros(shp, f32)
        assert lib().p3d_get_ema(s._h, n.encode(), fptr(buf), buf.size) == -1, n
        assert "not trainable" in lib().p3d_last_error().decode()
    s.close()


# ---- 3: the trajectory -----------------------------------------------------------------------------------------------------
def test_trajectory_untouched():
    params = _params("unet")
    x, y = _data()
    runs = []
    for on in (False, True):
        s = _session(params=params)
        s.set_adam(1e-3)
        if on:
            s.set_ema(0.99)
        losses = [s.train_step(x, y, dropout=0.5, seed=k) for k in range(3)]
        runs.append((losses, _all_params(s)))
        s.close()
    assert runs[0][0] == runs[1][0]
    for n in runs[0][1]:
        assert _bits_equal(runs[0][1][n], runs[1][1][n]), n


# ---- 4: the schedule -------------------------------------------------------------------------------------------------------
OPT_KERNELS = ("adam_kernel", "adam_decay_kernel", "adam_scaled_kernel", "adam_decay_scaled_kernel")


def _launches(sched, stream="main"):
    out = []
    for ln in sched:
        f = ln.split()
        if f[0] == "L" and f[1] == stream:
            out.append(f[2])
    return out


@pytest.mark.parametrize("setting", ["plain", "clip", "decay"])
def test_schedule(setting):
    x, y = _data()
    s = _session(params=_params("unet"))
    s.upload(x, y)
    if setting == "clip":
        s.set_grad_clip(float("inf"))
    if setting == "decay":
        s.set_regularization(("weightdecay",))
    off = s.schedule(0.5, seed=1)
    assert not any("ema_kernel" in ln for ln in off)
    s.set_ema(0.9)
    on = s.schedule(0.5, seed=1)
    assert sum(" ema_kernel" in ln for ln in on) == 2
    assert all(ln.split()[1] == "main" for ln in on if " ema_kernel" in ln)
    assert [ln for ln in on if " ema_kernel" not in ln] == off            # nothing else moved
    main = _launches(on)
    opt = [i for i, k in enumerate(main) if k in OPT_KERNELS]
    assert len(opt) == 2
    for i in opt:
        assert main[i + 1] == "ema_kernel", main[i:i + 2]
    # directly: no stream operation of any kind between an optimiser launch and its average
    for i, ln in enumerate(on):
        f = ln.split()
        if f[0] == "L" and f[2] in OPT_KERNELS:
            assert on[i + 1].split()[:3] == ["L", "main", "ema_kernel"], on[i:i + 2]
    s.set_ema(None)
    assert s.schedule(0.5, seed=1) == off
    s.close()


# ---- 5: warm-up ------------------------------------------------------------------------------------------------------------
def test_warmup_follows_the_step_count():
    from sap3d_tensorflow_amd._lib import check, lib
    x, y = _data()
    s = _session(params=_params("unet"))
    s.set_adam(1e-3)
    s.set_ema(0.999, warmup=True)
    prev = _shadows(s)
    for t in (1, 2, 3, 1001):
        if t == 1001:
            check(lib().p3d_set_optimizer_step(s._h, 1000))
        s.train_step(x, y, dropout=0.5, seed=t)
        assert s.optimizer_step() == t
        om = ema_ref.om_warmup(0.999, t)
        cur = _shadows(s)
        for n in cur:
            assert _bits_equal(cur[n], ema_ref.update32(prev[n], s.get_param(n), om)), (t, n)
        prev = cur
    assert len({float(ema_ref.om_warmup(0.999, t)) for t in (1, 2, 3, 1001)}) == 4
    s.close()


# ---- 6: the swap -----------------------------------------------------------------------------------------------------------
def test_swap_scores_the_averages_and_refuses_training():
    from sap3d_tensorflow_amd import P3dError
    params = _params("unet")
    x, y = _data()
    s = _session(params=params)
    s.set_adam(1e-3)
    s.set_ema(0.5)
    for k in range(2):
        s.train_step(x, y, dropout=0.5, seed=k)
    before, shadows = _all_params(s), _shadows(s)
    assert any(not _bits_equal(shadows[n], before[n]) for n in shadows)
    other = _session(params=dict(before, **shadows))              # a second network holding the averages
    want = other.forward(x)
    other.close()
    with s.averaged():
        assert s.ema_swapped()
        got = s.forward(x)
        for n in shadows:
            assert _bits_equal(s.get_param(n), shadows[n]), n     # get_param returns what the buffer holds
        for call in (lambda: s.train_step(x, y), lambda: s.backward(x, y), lambda: s.train_step_device(0.5),
                     lambda: s.set_param(_trainables(s)[0], params[_trainables(s)[0]]), lambda: s.set_ema(0.9),
                     lambda: s.set_ema(None), lambda: s.init_params(3)):
            with pytest.raises(P3dError, match="exchanged"):
                call()
    assert _bits_equal(got, want)
    assert not _bits_equal(got, s.forward(x))
    assert not s.ema_swapped()
    after = _all_params(s)
    for n in before:
        assert _bits_equal(after[n], before[n]), n                 # two swaps restore every bit
    for n in shadows:
        assert _bits_equal(s.get_ema(n), shadows[n]), n
    with pytest.raises(ZeroDivisionError):                         # the weights come back through an exception
        with s.averaged():
            1 / 0
    assert not s.ema_swapped()
    s.train_step(x, y, dropout=0.5, seed=2)                        # the handle still works
    assert s.optimizer_step() == 3
    s.close()


# ---- 7: checkpoints --------------------------------------------------------------------------------------------------------
def test_checkpoints_carry_the_shadows(tmp_path):
    from sap3d_tensorflow_amd import tf_checkpoint as tfc
    params = _params("unet")
    x, y = _data()

    def fresh(p=None, seed=1):
        s = _session(params=p, seed=seed)
        s.set_adam(1e-3)
        return s

    a = fresh(params)
    a.set_ema(0.9)
    for k in range(4):
        a.train_step(x, y, dropout=0.5, seed=k)
    want_p, want_s = _all_params(a), _shadows(a)
    a.close()
    b = fresh(params)
    b.set_ema(0.9)
    for k in range(2):
        b.train_step(x, y, dropout=0.5, seed=k)
    mid = _shadows(b)
    prefix = b.save_checkpoint(str(tmp_path), 2, optimizer_state=True, ema=True)
    b.set_ema(None)
    plain = b.save_checkpoint(str(tmp_path / "plain"), 2, optimizer_state=True)
    b.close()
    keys = set(k for k, _, _ in tfc.list_variables(prefix))
    assert set(ema_ref.shadow_name(n) for n in mid) <= keys
    assert not any(k.endswith(ema_ref.SUFFIX) for k, _, _ in tfc.list_variables(plain))
    c = fresh(seed=7)
    c.set_ema(0.9)
    c.restore(prefix, optimizer_state=True, ema=True)
    for n in mid:
        assert _bits_equal(c.get_ema(n), mid[n]), n
    for k in range(2, 4):
        c.train_step(x, y, dropout=0.5, seed=k)
    got_p, got_s = _all_params(c), _shadows(c)
    for n in want_p:
        assert _bits_equal(got_p[n], want_p[n]), n
    for n in want_s:
        assert _bits_equal(got_s[n], want_s[n]), n
    with pytest.raises(KeyError, match="moving averages"):
        c.restore(plain, ema=True)
    for n in want_p:
        assert _bits_equal(c.get_param(n), want_p[n]), n           # the refusal set nothing
    c.close()
    d = fresh(seed=9)                                               # the option off: the averages as the weights
    d.restore(prefix, ema_as_weights=True)
    saved = tfc.read_checkpoint(prefix)
    for n, _, tr in d.variables():
        assert _bits_equal(d.get_param(n), mid[n] if tr else saved[n]), n
    with pytest.raises(KeyError, match="moving averages"):
        d.restore(plain, ema_as_weights=True)
    d.close()


# ---- 8: the captured step --------------------------------------------------------------------------------------------------
_CAPTURE = r"""
import hashlib, sys
sys.path.insert(0, %(root)r)
from oracle import p3d
from sap3d_tensorflow_amd import P3DSession
cfg, shape = p3d.NetConfig(base=16, blocks=(1, 1, 2)), (1, 16, 32, 32)
s = P3DSession("unet", batch=shape[0], frames=shape[1], height=shape[2], width=shape[3], base=cfg.base, blocks=cfg.blocks, seed=1)
s.set_adam(1e-3)
s.upload(p3d.synthetic_clip(0, shape + (3,)), p3d.synthetic_target(3, shape))
plan = [(0.999, True), (0.999, True), (0.999, True), (0.9, False), (0.9, False), (0.5, False), (0.5, True)]
for k, (decay, warm) in enumerate(plan):
    if k == 0 or plan[k - 1] != plan[k]:      # (set_ema drops a captured step: the warm-up steps replay one graph)
        s.set_ema(decay, warmup=warm)
    s.train_step_device(0.5, seed=k)
    s.synchronize()
    h, hp = hashlib.sha256(), hashlib.sha256()
    for n, _, tr in s.variables():
        hp.update(s.get_param(n).tobytes())
        if tr:
            h.update(s.get_ema(n).tobytes())
    print("%%r %%d %%s %%s" %% (s.last_loss(), s.optimizer_step(), hp.hexdigest(), h.hexdigest()))
s.close()
"""


def test_captured_step_carries_the_average():
    res = {}
    for graph in ("0", "1"):
        env = dict(os.environ, P3D_GRAPH=graph)
        r = subprocess.run([sys.executable, "-c", _CAPTURE % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "capture failed" not in r.stderr, r.stderr[-3000:]
        res[graph] = r.stdout.split("\n")[:7]
    assert res["0"] == res["1"]
    assert [int(ln.split()[1]) for ln in res["0"]] == [1, 2, 3, 4, 5, 6, 7]
    assert len(set(ln.split()[3] for ln in res["0"])) == 7          # every step moved the shadows


# ---- 9: a one-rank communicator --------------------------------------------------------------------------------------------
def test_one_rank_communicator_same_shadows(monkeypatch):
    from sap3d_tensorflow_amd import P3DSession
    monkeypatch.setenv("P3D_BUCKET_MB", "1")
    cfg, shape = p3d.NetConfig(base=16, blocks=(1, 1, 2)), (2, 16, 32, 32)
    x, y = _data(shape)

    def run(with_comm):
        s = _session("unet", cfg, shape, seed=1)
        if with_comm:
            s.comm_init(P3DSession.comm_unique_id())
        s.set_adam(1e-3)
        s.set_ema(0.9)
        losses = [s.train_step(x, y, dropout=0.5, seed=k) for k in range(3)]
        sh = _shadows(s)
        sched = s.schedule(0.5, seed=4) if with_comm else None
        s.close()
        return losses, sh, sched

    la, sa, _ = run(False)
    lb, sb, sched = run(True)
    assert la == lb
    for n in sa:
        assert _bits_equal(sa[n], sb[n]), n
    assert any(ln.startswith("C ") and "allreduce" in ln for ln in sched)
    main = _launches(sched)
    assert sum(k == "ema_kernel" for k in main) == 2
    for i, k in enumerate(main):
        if k == "adam_kernel":
            assert main[i + 1] == "ema_kernel"
    assert not any(" ema_kernel" in ln and ln.split()[1] != "main" for ln in sched)


# ---- 10: refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    from sap3d_tensorflow_amd._lib import fptr, lib
    s = _session()
    h = s._h
    n, shp = [(n, shp) for n, shp, tr in s.variables() if tr][0]
    buf = np.zeros(shp, f32)
    assert lib().p3d_get_ema(h, n.encode(), fptr(buf), buf.size) == -1             # the option is off
    assert "off" in lib().p3d_last_error().decode()
    assert lib().p3d_set_ema_var(h, n.encode(), fptr(buf), buf.size) == -1
    assert lib().p3d_ema_swap(h) == -1 and lib().p3d_ema_swapped(h) == 0
    sched = s.schedule(0.5, seed=0)
    for decay in (1.0, 1.5, float("nan"), float("inf")):
        assert lib().p3d_set_ema(h, decay, 0) == -1, decay
        assert lib().p3d_last_error().decode()
        assert lib().p3d_get_ema(h, n.encode(), fptr(buf), buf.size) == -1         # nothing changed: still off
    assert s.schedule(0.5, seed=0) == sched
    s.set_ema(0.0)                                                                 # 0 is valid: the shadow is the variable
    for decay in (1.0, float("nan")):
        assert lib().p3d_set_ema(h, decay, 1) == -1, decay
    assert lib().p3d_get_ema(h, n.encode(), fptr(buf), buf.size) == 0              # ... and a refusal leaves it on
    assert lib().p3d_get_ema(h, n.encode(), fptr(buf), buf.size + 1) == -1         # wrong count
    assert lib().p3d_set_ema_var(h, n.encode(), fptr(buf), buf.size - 1) == -1
    assert lib().p3d_get_ema(h, b"no/such/var", fptr(buf), buf.size) == -1
    z = np.zeros(8, f32)
    assert lib().p3d_debug_ema(0, fptr(z), fptr(z), 8, 4, 0.1, 0) == -1
    assert lib().p3d_debug_ema(0, fptr(z), fptr(z), 0, 0, 0.1, 0) == -1
    # p3d_set_param leaves the shadows alone; p3d_init_params seeds them again; another optimiser kind leaves them alone
    s.set_ema_var(n, np.full(shp, 2.0, f32))
    s.set_param(n, np.full(shp, 3.0, f32))
    assert np.all(s.get_ema(n) == 2.0)
    s.set_optimizer("sgd", lr=1e-3)
    assert np.all(s.get_ema(n) == 2.0)
    s.init_params(5)
    assert _bits_equal(s.get_ema(n), s.get_param(n))
    s.close()


# ---- 11: the drivers -------------------------------------------------------------------------------------------------------
def test_drivers(tmp_path):
    from sap3d_tensorflow_amd import tf_checkpoint as tfc
    drv = os.path.join(ROOT, "drivers")
    small = ["--batch", "2", "--imagesize", "32", "32", "--validiter", "3", "--validclips", "1", "--plotiter", "1"]
    r = subprocess.run([sys.executable, os.path.join(drv, "train.py"), "--ema-decay", "0.9", "--steps", "3", "--saveiter", "3",
                        "--optimizer-state", "--info", "ema"] + small, cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "Metrics:" in r.stdout
    model = tmp_path / "model" / "ema"
    prefix = tfc.latest_checkpoint(str(model))
    names = [k for k, _, _ in tfc.list_variables(prefix)]
    shadows = [k for k in names if k.endswith("/" + ema_ref.SUFFIX)]
    assert shadows and all(k[:-len(ema_ref.SUFFIX) - 1] in names for k in shadows)
    assert not any("moving_mean/" in k for k in shadows)
    some = tfc.read_checkpoint(prefix, names=set(shadows[:5]) | set(k[:-len(ema_ref.SUFFIX) - 1] for k in shadows[:5]))
    assert any(not _bits_equal(some[k], some[k[:-len(ema_ref.SUFFIX) - 1]]) for k in shadows[:5])
    r = subprocess.run([sys.executable, os.path.join(drv, "test.py"), "--ema", "--model", str(model), "--structure", "unet",
                        "--clips", "2"], cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "Testing Finished!" in r.stdout
    videos = tmp_path / "videos"
    videos.mkdir()
    np.save(videos / "synth.npy", np.random.default_rng(0).integers(0, 256, (17, 120, 160, 3)).astype(np.uint8))
    r = subprocess.run([sys.executable, os.path.join(drv, "gen_pred.py"), "--ema", "--model", str(model), "--structure", "unet",
                        "--videos", str(videos), "--out", str(tmp_path / "pred"), "--batch", "2"], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert np.load(tmp_path / "pred" / "synth.npy").shape == (17, 112, 112)
