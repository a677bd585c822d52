"""Gradient accumulation over micro-batches (P3DSession.set_grad_accum) on the GPU: grad_accum_kernel at op level against the
bit-exact replay of accum_ref.py, whole cycles against a twin session's backward passes and the numpy optimiser replays, the
moving statistics, the option off, the schedule without and with a one-rank communicator, clipping and the moving average on
together, resets and refusals, P3D_GRAPH=1, and the training driver.

Every comparison of gradients, weights and losses is bitwise: a cycle's applied gradient is ((g0 + g1) + g2) in float32, and the
micro-batch gradients are those of p3d_backward on the same weights (the backward's bits are the train step's,
test_gpu_determinism.py).  The reported norm is held to the bounds tests/test_gpu_grad_clip.py derives: n 2^-52 relative for the
double sum of exact squares, 2 double ulps for the norm, 1 float32 ulp for the scale."""
import hashlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from oracle import p3d          # noqa: E402
import accum_ref                # noqa: E402
import clip_ref                 # noqa: E402
import ema_ref                  # noqa: E402
import opt_ref                  # noqa: E402
import reg_ref                  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(HERE)
CFG = p3d.NetConfig(base=16, blocks=(1, 2, 2))      # the tiny net of test_gpu_ema.py
SHAPE = (1, 16, 32, 32)
B1, B2, EPS = 0.9, 0.999, 1e-8
f32 = np.float32
OPT_WORDS = ("adam", "momentum", "sgd")


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


_BATCHES = {}


def _micro(j, shape=SHAPE):
    """Micro-batch j: its own clip, target and dropout seed (computed once and shared)."""
    if (j, shape) not in _BATCHES:
        _BATCHES[(j, shape)] = (p3d.synthetic_clip(j, shape + (3,)), p3d.synthetic_target(3 + j, shape), 10 + j)
    return _BATCHES[(j, shape)]


def _trainables(s):
    return [n for n, _, tr in s.variables() if tr]


def _all_params(s):
    return {n: s.get_param(n) for n, _, _ in s.variables()}


def _grads(s):
    return {n: s.get_grad(n) for n in _trainables(s)}


def _step(s, j, shape=SHAPE):
    x, y, seed = _micro(j, shape)
    return s.train_step(x, y, dropout=0.5, seed=seed)


def _back(s, j, shape=SHAPE):
    x, y, seed = _micro(j, shape)
    return s.backward(x, y, dropout=0.5, seed=seed)[0]


# ---- 1: op level -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4097, 2 ** 20 + 3])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("mode", ["store", "add", "finish"])
def test_grad_accum_op(n, offset, mode):
    """Offsets 1-3 start the range mid-16-byte line: head elements one by one, float4 groups, the cut last group one by one.  The
    caller's arrays carry one element more on each side than the launch is given; the hook itself surrounds the device range
    with guard elements and fails if the launch touched one or changed the operand its mode only reads.  The inputs hold -0,
    denormals, g = -acc, +-inf, overflow and addends that are rounded away, and no NaN (test_accum_cpu.py)."""
    from sap3d_tensorflow_amd._lib import check, fptr, lib
    acc, g = accum_ref.special_inputs(n + 2, n * 3 + offset)
    a_io, g_io = acc.copy(), g.copy()
    a_in, g_in = a_io[1:n + 1], g_io[1:n + 1]            # views: the hook reads and writes n elements one past the start
    assert a_in.ctypes.data == a_io.ctypes.data + 4
    check(lib().p3d_debug_grad_accum(0, accum_ref.MODES[mode], fptr(a_in), fptr(g_in), n, offset))
    want = accum_ref.launch(mode, acc[1:n + 1], g[1:n + 1])
    written, kept, kept_ref = (g_io, a_io, acc) if mode == "finish" else (a_io, g_io, g)
    assert _bits_equal(written[1:n + 1], want)
    assert _bits_equal(written[[0, n + 1]], (g if mode == "finish" else acc)[[0, n + 1]])      # one element on each side
    assert _bits_equal(kept, kept_ref)                                                        # the operand the mode reads


def test_signed_zero_through_the_kernel():
    from sap3d_tensorflow_amd import ops
    nz, pz = np.full(9, -0.0, f32), np.zeros(9, f32)
    for offset in (0, 3):
        assert np.all(ops.grad_accum(pz, nz, "store", offset=offset).view(np.uint32) == 0x80000000)      # STORE keeps -0
        assert np.all(ops.grad_accum(pz, nz, "add", offset=offset).view(np.uint32) == 0)                 # +0 + -0 = +0
        assert np.all(ops.grad_accum(pz, nz, "finish", offset=offset).view(np.uint32) == 0)
        assert np.all(ops.grad_accum(nz, nz, "add", offset=offset).view(np.uint32) == 0x80000000)


def test_grad_accum_op_through_ops():
    from sap3d_tensorflow_amd import ops
    acc, g = accum_ref.special_inputs(777, 5)
    keep_a, keep_g = acc.copy(), g.copy()
    for mode in ("store", "add", "finish"):
        assert _bits_equal(ops.grad_accum(acc, g, mode, offset=2), accum_ref.launch(mode, acc, g)), mode
    assert _bits_equal(acc, keep_a) and _bits_equal(g, keep_g)


# ---- 2: a cycle is the replay ----------------------------------------------------------------------------------------------
def _lr_t(t, lr):
    from sap3d_tensorflow_amd import ops
    z = np.zeros(4, f32)
    return ops.adam(z, z, z, z, t, lr, B1, B2, EPS)[3]


@pytest.mark.parametrize("structure", ["unet", "gn_p3d"])
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("opt", ["adam", "sgd", "adam+weightdecay"])
def test_a_cycle_is_the_replay(structure, K, opt):
    """A accumulates; its twin B (same weights, no regularisation term, never stepping) gives every micro-batch's gradient and
    data loss through backward.  The weights do not move during a cycle, so these are the gradients A must have seen."""
    params = _params(structure)
    A, Bt = _session(structure, params=params), _session(structure, params=params)
    names = _trainables(A)
    lr = 1e-3 if opt != "sgd" else 1e-6
    if opt == "sgd":
        A.set_optimizer("sgd", lr=lr)
    else:
        A.set_adam(lr)
    coef = {}
    if opt.endswith("weightdecay"):
        A.set_regularization(("weightdecay",))
        coef = {n: f32(A.param_regularization(n)[0]) for n in names}
        coef = {n: c for n, c in coef.items() if c != 0}
        assert coef
    assert A.grad_accum == (1, 0)
    A.set_grad_accum(K)
    assert A.grad_accum == (K, 0)
    for cycle in range(2):                                 # the second cycle starts from a store: nothing of the first leaks
        p0 = _all_params(A)
        if cycle:
            Bt.load(p0)
        t0 = A.optimizer_step()
        assert t0 == cycle
        g, losses = [], []
        for j in range(K):
            losses.append(_back(Bt, cycle * K + j))
            g.append(_grads(Bt))
        assert any(not _bits_equal(g[0][n], g[1][n]) for n in names)
        for j in range(K - 1):
            loss = _step(A, cycle * K + j)
            assert f32(loss).tobytes() == f32(losses[j]).tobytes(), (cycle, j)      # the data loss alone
            assert A.last_regularization() == 0.0
            assert A.optimizer_step() == t0 and A.grad_accum == (K, j + 1)
            for n, _, _ in A.variables():
                if n in g[j]:
                    assert _bits_equal(A.get_param(n), p0[n]), (cycle, j, n)
                    assert _bits_equal(A.get_grad(n), g[j][n]), (cycle, j, n)
        loss = _step(A, cycle * K + K - 1)
        assert A.optimizer_step() == t0 + 1 and A.grad_accum == (K, 0)
        if coef:
            term = reg_ref.term64(p0, coef)
            assert A.last_regularization() > 0
            assert abs(A.last_regularization() - term) <= 1e6 * 2.0 ** -52 * term
            ulp = float(np.spacing(f32(abs(loss))))
            assert abs((loss - losses[K - 1]) - term) <= 2 * ulp + 1e6 * 2.0 ** -52 * term
        else:
            assert f32(loss).tobytes() == f32(losses[K - 1]).tobytes()
        moved = 0
        for n in names:
            total = accum_ref.cycle([gj[n] for gj in g])
            if cycle == 0 and K == 3:                      # the order is the library's, not another
                assert _bits_equal(total, ((g[0][n] + g[1][n]).astype(f32) + g[2][n]).astype(f32))
            applied = reg_ref.decayed_grad32(total, coef[n], p0[n]) if n in coef else total
            assert _bits_equal(A.get_grad(n), applied), (cycle, n)
            if opt == "sgd":
                want = opt_ref.sgd32(p0[n], applied, lr)
            elif cycle == 0:
                zero = np.zeros_like(applied)
                want = reg_ref.adam32(p0[n], zero, zero, applied, _lr_t(1, lr), B1, B2, EPS, True)[0]
            else:
                want = None                                # (Adam's second update needs its slots: the gradient above is the check)
            got = A.get_param(n)
            if want is not None:
                assert _bits_equal(got, want), (cycle, n)
            moved += int(not _bits_equal(got, p0[n]))
        assert moved
    A.close()
    Bt.close()


# ---- 3: moving statistics follow every micro-step --------------------------------------------------------------------------
def test_moving_statistics_follow_every_micro_step():
    params = _params("unet")
    K = 3
    A, T = _session(params=params), _session(params=params)
    A.set_adam(1e-3)
    A.set_grad_accum(K)
    T.set_optimizer("sgd", lr=0.0)                         # K plain train steps whose weights stay put
    for j in range(K):
        _step(A, j)
        _step(T, j)
    states = [n for n, _, tr in A.variables() if not tr]
    assert any(n.endswith("moving_mean") for n in states) and any(n.endswith("moving_variance") for n in states)
    moved = 0
    for n in states:
        assert _bits_equal(A.get_param(n), T.get_param(n)), n
        moved += int(not _bits_equal(A.get_param(n), params[n]))
    assert moved
    for n in _trainables(T):
        assert _bits_equal(T.get_param(n), params[n]), n   # (the twin's weights did stay put)
    A.close()
    T.close()


# ---- 4: off is off ---------------------------------------------------------------------------------------------------------
def test_off_is_off():
    params = _params("unet")
    runs = []
    for call in (False, True):
        s = _session(params=params)
        s.set_adam(1e-3)
        if call:
            s.set_grad_accum(1)
        losses = [_step(s, j) for j in range(3)]
        assert s.optimizer_step() == 3 and s.grad_accum == (1, 0)
        runs.append((losses, _all_params(s), s.schedule(0.5, seed=1)))
        s.close()
    assert runs[0][0] == runs[1][0]
    for n in runs[0][1]:
        assert _bits_equal(runs[0][1][n], runs[1][1][n]), n
    assert runs[0][2] == runs[1][2]
    assert not any("grad_accum" in ln or ln.startswith("G ") for ln in runs[0][2])


# ---- 5: the schedule -------------------------------------------------------------------------------------------------------
def _launches(sched, stream="main"):
    return [ln.split()[2] for ln in sched if ln.split()[0] == "L" and ln.split()[1] == stream]


def _is_opt(kernel):
    return any(kernel.startswith(w) for w in OPT_WORDS)


def _accum_lines(sched):
    """[(index, stream, mode, lo, hi)] of the accumulation launches; each is announced by a G line right ahead of its L line."""
    out = []
    for i, ln in enumerate(sched):
        f = ln.split()
        if f[0] == "G":
            nxt = sched[i + 1].split()
            assert nxt[:3] == ["L", f[1], "grad_accum_kernel<%d>" % accum_ref.MODES[f[2]]], sched[i:i + 2]
            out.append((i, f[1], f[2], int(f[3]), int(f[4])))
    assert len(out) == sum("grad_accum_kernel" in ln for ln in sched)
    return out


@pytest.mark.parametrize("setting", ["plain", "clip+ema"])
def test_schedule(setting):
    x, y, _ = _micro(0)
    s = _session(params=_params("unet"))
    s.upload(x, y)
    n_train = s.bucket_audit(1 << 20)[1]
    if setting == "clip+ema":
        s.set_grad_clip(float("inf"))
        s.set_ema(0.9)
    off = s.schedule(0.5, seed=1)
    s.set_grad_accum(3)
    traces = [s.schedule(0.5, seed=1) for _ in range(3)]
    assert s.grad_accum == (3, 0) and s.optimizer_step() == 2
    for j, tr in enumerate(traces[:2]):
        for ln in tr:
            f = ln.split()
            assert "allreduce" not in ln
            if f[0] == "L":
                assert not _is_opt(f[2]) and "sumsq" not in f[2] and "ema" not in f[2], ln
        acc = _accum_lines(tr)
        assert [(a[1], a[2], a[3], a[4]) for a in acc] == [("main", "store" if j == 0 else "add", 0, n_train)]
        waits = [i for i, ln in enumerate(tr) if ln.split()[0] == "W" and ln.split()[1] == "main"]
        assert waits and acc[0][0] > waits[-1]             # after the main stream has joined the side stream
        assert all(ln.split()[0] != "L" for ln in tr[acc[0][0] + 2:])      # and it is the micro-step's last launch
    ap = traces[2]
    fin = _accum_lines(ap)
    assert all(a[1] == "main" and a[2] == "finish" for a in fin)
    assert [(a[3], a[4]) for a in fin] == [(fin[0][3], n_train), (0, fin[0][3])] and 0 < fin[0][3] < n_train
    kinds = []
    for k in _launches(ap):
        kinds.append("finish" if k == "grad_accum_kernel<2>" else "sumsq" if "sumsq" in k else "opt" if _is_opt(k) else None)
    kinds = [k for k in kinds if k]
    # every range is finished ahead of its first reader, in the optimiser's two ranges: [split, n) in the early slot, [0, split)
    # at the tail; under clipping the readers are the norm's two ranges, and both optimiser parts follow
    assert kinds == (["finish", "opt", "finish", "opt"] if setting == "plain" else ["finish", "sumsq", "finish", "sumsq", "opt", "opt"])
    # and nothing else moved: without its two finishing launches the applying micro-step is the plain step
    drop = set(i for a in fin for i in (a[0], a[0] + 1))
    assert [ln for i, ln in enumerate(ap) if i not in drop] == off
    s.set_grad_accum(1)
    assert s.schedule(0.5, seed=1) == off
    s.close()


# ---- 6: a one-rank communicator --------------------------------------------------------------------------------------------
def test_one_rank_communicator(monkeypatch):
    from sap3d_tensorflow_amd import P3DSession
    monkeypatch.setenv("P3D_BUCKET_MB", "1")
    cfg, shape = p3d.NetConfig(base=16, blocks=(1, 1, 2)), (2, 16, 32, 32)

    def run(with_comm):
        s = _session("unet", cfg, shape, seed=1)
        if with_comm:
            s.comm_init(P3DSession.comm_unique_id())
        s.set_adam(1e-3)
        s.set_grad_accum(2)
        losses = [_step(s, j, shape) for j in range(4)]
        assert s.optimizer_step() == 2
        out = _all_params(s)
        n_train = s.bucket_audit(1 << 20)[1]               # (the audit hook is no micro-step and leaves the cycle alone)
        traces = [s.schedule(0.5, seed=4) for _ in range(2)] if with_comm else None
        s.close()
        return losses, out, traces, n_train

    la, pa, _, _ = run(False)
    lb, pb, traces, n_train = run(True)
    assert la == lb
    for n in pa:
        assert _bits_equal(pa[n], pb[n]), n
    assert not any("allreduce" in ln for ln in traces[0])
    assert [(a[1], a[2], a[3], a[4]) for a in _accum_lines(traces[0])] == [("main", "store", 0, n_train)]
    ap = traces[1]
    red = [(i, int(ln.split()[3]), int(ln.split()[4])) for i, ln in enumerate(ap) if ln.startswith("C ") and "allreduce" in ln]
    assert len(red) > 1                                    # more than one bucket
    spans = sorted((lo, hi) for _, lo, hi in red)
    assert spans[0][0] == 0 and spans[-1][1] == n_train
    assert all(spans[k][1] == spans[k + 1][0] for k in range(len(spans) - 1))      # [0, n_train) exactly once
    fin = _accum_lines(ap)
    assert all(a[1] == "comm" and a[2] == "finish" for a in fin)
    # each bucket is finished on the comm stream right ahead of its collective, after the bucket's two event waits
    assert [(a[0] + 2, a[3], a[4]) for a in fin] == red
    for a in fin:
        assert ap[a[0] - 1].split()[:2] == ["W", "comm"], ap[a[0] - 2:a[0] + 1]


# ---- 7: clipping and the moving average on together ------------------------------------------------------------------------
def test_with_clipping_and_the_moving_average():
    from sap3d_tensorflow_amd import P3dError
    params = _params("unet")
    K, lr = 2, 1e-6
    A, Bt = _session(params=params), _session(params=params)
    names = _trainables(A)
    g = []
    for j in range(K):
        _back(Bt, j)
        g.append(_grads(Bt))
    total = {n: accum_ref.cycle([gj[n] for gj in g]) for n in names}
    ref = clip_ref.sumsq64(np.concatenate([v.ravel() for v in total.values()]))
    count = sum(v.size for v in total.values())
    clip = float(f32(math.sqrt(ref) / 4))
    A.set_optimizer("sgd", lr=lr)
    A.set_grad_clip(clip)
    A.set_ema(0.9)
    A.set_grad_accum(K)
    om = ema_ref.om_const(0.9)
    _step(A, 0)
    with pytest.raises(P3dError, match="no train step"):   # an accumulating micro-step reports no norm
        A.last_grad_norm()
    for n in names:
        assert _bits_equal(A.get_ema(n), params[n]) and _bits_equal(A.get_param(n), params[n]), n
    _step(A, 1)
    nm, sc, ss = A.last_grad_norm(with_sumsq=True)
    print("sumsq", repr(ss), "ref", repr(ref), "norm ulps", clip_ref.ulps64(nm, math.sqrt(ref)), "scale", sc)
    assert abs(ss - ref) <= count * 2.0 ** -52 * ref
    assert clip_ref.ulps64(nm, math.sqrt(ref)) <= 2
    assert clip_ref.ulps32(sc, clip_ref.scale32(math.sqrt(ref), clip)) <= 1 and sc < 1
    p1, sh1 = {}, {}
    for n in names:
        p1[n], sh1[n] = A.get_param(n), A.get_ema(n)
        assert _bits_equal(A.get_grad(n), total[n]), n     # clipping does not rewrite the gradient buffer
        assert _bits_equal(p1[n], opt_ref.sgd32(params[n], clip_ref.scaled32(total[n], f32(sc)), lr)), n
        assert _bits_equal(sh1[n], ema_ref.update32(params[n], p1[n], om)), n      # one move per cycle
    assert any(not _bits_equal(sh1[n], params[n]) for n in names)
    _step(A, 2)                                            # the next cycle's accumulating micro-step touches neither
    assert A.last_grad_norm(with_sumsq=True) == (nm, sc, ss)
    for n in names:
        assert _bits_equal(A.get_ema(n), sh1[n]) and _bits_equal(A.get_param(n), p1[n]), n
    A.close()
    Bt.close()


# ---- 8: resets and refusals ------------------------------------------------------------------------------------------------
def test_resets_and_refusals():
    from sap3d_tensorflow_amd import P3dError
    from sap3d_tensorflow_amd._lib import fptr, lib
    params = _params("unet")

    def fresh(init_seed=None):
        s = _session(params=None if init_seed is not None else params)
        if init_seed is not None:
            s.init_params(init_seed)
        s.set_adam(1e-3)
        return s

    def cycle(s):                                          # micro-batches 1 and 2
        losses = [_step(s, 1), _step(s, 2)]
        assert s.grad_accum == (2, 0)
        return losses, {n: s.get_param(n) for n in _trainables(s)}

    def same(a, b):
        assert a[0] == b[0]
        for n in a[1]:
            assert _bits_equal(a[1][n], b[1][n]), n

    s = fresh()
    for k in (0, -3):
        assert lib().p3d_set_grad_accum(s._h, k) == -1 and lib().p3d_last_error().decode()
        assert s.grad_accum == (1, 0)
    s.set_grad_accum(2)
    want = cycle(s)
    s.close()

    s = fresh()                                            # a call mid-cycle, with the same k, discards the partial sum
    s.set_grad_accum(2)
    _step(s, 0)
    assert s.grad_accum == (2, 1)
    assert lib().p3d_set_grad_accum(s._h, 0) == -1 and s.grad_accum == (2, 1)      # a refusal changes nothing
    s.set_grad_accum(2)
    assert s.grad_accum == (2, 0)
    same(cycle(s), want)
    s.close()

    s = fresh()                                            # backward mid-cycle, and the calls that leave a cycle alone
    s.set_grad_accum(2)
    _step(s, 1)
    _back(s, 0)
    first = _trainables(s)[0]
    s.set_param(first, params[first])
    s.set_optimizer("adam", lr=1e-3)
    s.set_ema(0.9)
    s.ema_swap()
    assert s.grad_accum == (2, 1)
    x, y, _ = _micro(2)
    for call in (lambda: s.train_step(x, y), lambda: s.train_step_device(0.5), lambda: s.profile_step(0.5)):
        with pytest.raises(P3dError, match="exchanged"):   # training calls are still refused while exchanged
            call()
    assert s.grad_accum == (2, 1)
    s.ema_swap()
    s.set_ema(None)
    losses = [None, _step(s, 2)]
    assert s.grad_accum == (2, 0) and losses[1] == want[0][1]
    for n in want[1]:
        assert _bits_equal(s.get_param(n), want[1][n]), n
    s.close()

    a = fresh(init_seed=5)                                 # init_params discards a partial sum too
    a.set_grad_accum(2)
    ref = cycle(a)
    a.close()
    s = fresh()
    s.set_grad_accum(2)
    _step(s, 0)
    s.init_params(5)
    assert s.grad_accum == (2, 0) and s.optimizer_step() == 0
    same(cycle(s), ref)
    s.close()

    z, z2 = np.zeros(8, f32), np.zeros(8, f32)
    assert lib().p3d_debug_grad_accum(0, 1, fptr(z), fptr(z2), 8, 4) == -1
    assert lib().p3d_debug_grad_accum(0, 1, fptr(z), fptr(z2), 0, 0) == -1
    assert lib().p3d_debug_grad_accum(0, 3, fptr(z), fptr(z2), 8, 0) == -1


def test_profile_step_is_a_micro_step():
    x, y, _ = _micro(0)
    s = _session(params=_params("unet"))
    s.set_adam(1e-3)
    s.upload(x, y)
    s.set_grad_accum(2)
    first = [r["kernel"] for r in s.profile_step(0.5, seed=1)]
    assert s.grad_accum == (2, 1) and s.optimizer_step() == 0
    assert first[-1] == "grad_accum_kernel<0>" and not any(_is_opt(k) for k in first)
    second = [r["kernel"] for r in s.profile_step(0.5, seed=2)]
    assert s.grad_accum == (2, 0) and s.optimizer_step() == 1
    assert second.count("grad_accum_kernel<2>") == 1 and second.index("grad_accum_kernel<2>") < min(
        i for i, k in enumerate(second) if _is_opt(k))
    s.close()


# ---- 9: P3D_GRAPH=1 --------------------------------------------------------------------------------------------------------
_CAPTURE = r"""
import hashlib, sys
sys.path.insert(0, %(root)r)
from oracle import p3d
from sap3d_tensorflow_amd import P3DSession
cfg, shape = p3d.NetConfig(base=16, blocks=(1, 1, 2)), (1, 16, 32, 32)
s = P3DSession("unet", batch=shape[0], frames=shape[1], height=shape[2], width=shape[3], base=cfg.base, blocks=cfg.blocks, seed=1)
s.set_adam(1e-3)
for k in range(6):      # a plain step (captured under P3D_GRAPH=1), two cycles of two, a plain step again
    if k == 1:
        s.set_grad_accum(2)
    if k == 5:
        s.set_grad_accum(1)
    s.upload(p3d.synthetic_clip(k, shape + (3,)), p3d.synthetic_target(3 + k, shape))
    s.train_step_device(0.5, seed=k)
    s.synchronize()
    h = hashlib.sha256()
    for n, _, tr in s.variables():
        h.update(s.get_param(n).tobytes())
    print("%%r %%d %%d %%s" %% (s.last_loss(), s.optimizer_step(), s.grad_accum[1], h.hexdigest()))
s.close()
"""


def test_captured_step_is_set_aside_during_a_cycle():
    res = {}
    for graph in ("0", "1"):
        env = dict(os.environ, P3D_GRAPH=graph)
        r = subprocess.run([sys.executable, "-c", _CAPTURE % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "capture failed" not in r.stderr, r.stderr[-3000:]
        res[graph] = r.stdout.split("\n")[:6]
    assert res["0"] == res["1"]
    assert [(int(ln.split()[1]), int(ln.split()[2])) for ln in res["0"]] == [(1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (4, 0)]


# ---- 10: the driver --------------------------------------------------------------------------------------------------------
def test_driver(tmp_path):
    from sap3d_tensorflow_amd import P3DSession, synthetic as law, tf_checkpoint as tfc
    r = subprocess.run([sys.executable, os.path.join(ROOT, "drivers", "train.py"), "--accum-steps", "2", "--steps", "4", "--saveiter", "2",
                        "--plotiter", "1", "--validiter", "1000", "--batch", "2", "--imagesize", "32", "32", "--info", "acc"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "Optimiser updates: 2 from 4 batches" in r.stdout
    steps = [int(ln.split("Training step:")[1].split()[0]) for ln in r.stdout.split("\n") if "Training step:" in ln]
    assert steps == [1, 2]
    model = tmp_path / "model" / "acc"
    prefix = tfc.latest_checkpoint(str(model))
    assert os.path.basename(prefix) == "p3d_2.ckpt"
    saved = tfc.read_checkpoint(prefix)
    shape = (2, 16, 32, 32)
    s = P3DSession("unet", batch=2, frames=16, height=32, width=32, seed=0)
    s.set_adam(1e-4)
    s.set_grad_accum(2)
    losses = []
    for m in range(4):
        losses.append(s.train_step(law.synthetic_clip(m, shape + (3,)), law.synthetic_target(10_000 + m, shape), dropout=0.5, seed=m + 1))
    assert s.optimizer_step() == 2
    for n, _, _ in s.variables():
        assert _bits_equal(saved[n], s.get_param(n)), n
    printed = [float(ln.split("Training Loss")[1].split()[0]) for ln in r.stdout.split("\n") if "Training Loss" in ln]
    assert printed == [losses[0] + losses[1], losses[2] + losses[3]]      # the sum of the cycle's losses
    s.close()
