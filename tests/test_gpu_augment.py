"""Clip augmentation on the device (P3DSession.set_augment) on the GPU: augment.hip's launches at op level against the bit-exact
replay of augment_ref.py, the library's draws against the pinned fixture, and at net level an augmented train step against a
plain train step of a twin session that is fed the replay's augmented clip -- with the fixation loss and under accumulation,
too --, the entry points that never augment, the option off, refusals, the device-resident form, and the training driver.

Every comparison is bitwise (uint32 views): replay and kernels perform the same float32 operations in the same order, and a
train step's bits are a function of its inputs and weights (test_gpu_determinism.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from oracle import p3d          # noqa: E402
import augment_ref as ar        # noqa: E402
from test_augment_cpu import CFG_KEYS, _decision_ints, load_fixture      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(HERE)
CFG = p3d.NetConfig(base=16, blocks=(1, 1, 1))
SHAPE = (2, 16, 32, 32)
AUG = dict(flip=0.5, reverse=0.5, min_scale=0.6, contrast=0.2, brightness=0.1)
f32 = np.float32


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def _row(shape, flip=False, reverse=False, y0=0, x0=0, ch=None, cw=None, a=1.0, b=0.0):
    return (flip, reverse, y0, x0, shape[2] if ch is None else ch, shape[3] if cw is None else cw, f32(a), f32(b))


def _check(shape, rows, offset=0, with_fix=True, specials=False, seed=0):
    from sap3d_tensorflow_amd import ops
    x, y, fix = ar.random_clip(seed + 17 * offset, shape, specials=specials)
    keep = (x.copy(), y.copy(), fix.copy())
    xo, yo, fo = ops.augment(x, y, fix if with_fix else None, rows, offset=offset)
    wx, wy, wf = ar.batch(x, y, fix if with_fix else None, rows)
    assert _same(xo, wx), (shape, rows, offset)
    assert _same(yo, wy), (shape, rows, offset)
    if with_fix:
        assert np.array_equal(fo, wf), (shape, rows, offset)
    else:
        assert fo is None
    assert _same(x, keep[0]) and _same(y, keep[1]) and np.array_equal(fix, keep[2])
    return xo, yo, fo


# ---- 1: op level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("with_fix", [True, False])
def test_neutral_flip_only_and_everything_on(offset, with_fix):
    shape = (3, 3, 5, 7)
    rows = [_row(shape), _row(shape, flip=True), _row(shape, flip=True, reverse=True, y0=1, x0=2, ch=3, cw=4, a=1.3, b=-0.2)]
    _check(shape, rows, offset, with_fix)


@pytest.mark.parametrize("shape", [(2, 2, 1, 6), (2, 2, 6, 1), (1, 1, 1, 1), (2, 3, 1, 1)])
def test_one_row_and_one_column(shape):
    B, T, H, W = shape
    rows = [_row(shape, flip=True, reverse=True, x0=W // 3, cw=max(1, W // 2), y0=H // 3, ch=max(1, H // 2), a=0.7, b=0.1)
            for _ in range(B)]
    rows[-1] = _row(shape, flip=True)
    for offset in (0, 3):
        _check(shape, rows, offset)


@pytest.mark.parametrize("W", [7, 8])
def test_middle_column_under_flip(W):
    shape = (2, 2, 4, W)
    xo, yo, fo = _check(shape, [_row(shape, flip=True), _row(shape, flip=True, x0=1, cw=W - 2, y0=1, ch=2)])
    x, y, fix = ar.random_clip(0, shape)
    assert _same(yo[0], y[0][:, :, ::-1]) and np.array_equal(fo[0], fix[0][:, :, ::-1])
    if W % 2:
        assert _same(yo[0][:, :, W // 2], y[0][:, :, W // 2])      # the middle column stays where it is


def test_one_frame_under_reverse():
    shape = (2, 1, 5, 7)
    xo, yo, _ = _check(shape, [_row(shape, reverse=True), _row(shape, reverse=True, flip=True, a=0.9)])
    assert _same(yo[0], ar.random_clip(0, shape)[1][0])


@pytest.mark.parametrize("offset", [0, 2])
def test_windows(offset):
    shape = (4, 2, 5, 7)
    rows = [_row(shape, y0=2, x0=3, ch=1, cw=1),                   # 1 x 1: every pixel is that sample
            _row(shape, y0=4, x0=0, ch=1, cw=7),                   # 1 x W: the last row, columns kept
            _row(shape, a=1.25, b=0.5),                            # full, photometric alone
            _row(shape, y0=2, x0=3, ch=3, cw=4, reverse=True)]     # touching the bottom-right corner
    xo, yo, fo = _check(shape, rows, offset)
    x, y, fix = ar.random_clip(17 * offset, shape)
    assert _same(yo[0], np.broadcast_to(y[0][:, 2:3, 3:4], yo[0].shape))
    assert _same(yo[1], np.broadcast_to(y[1][:, 4:5, :], yo[1].shape))
    assert _same(yo[2], y[2]) and np.array_equal(fo[2], fix[2]) and not _same(xo[2], x[2])


@pytest.mark.parametrize("offset", [0, 1])
def test_special_values_pass_through_the_copies(offset):
    """Neutral, flip only, reverse only: no arithmetic touches x, y or the bytes, so NaN payloads, infinities, -0 and denormals
    keep their bits, and bytes other than 0 / 255 stay as they are."""
    shape = (3, 3, 5, 7)
    rows = [_row(shape), _row(shape, flip=True), _row(shape, reverse=True)]
    xo, yo, fo = _check(shape, rows, offset, specials=True)
    bits = xo.view(np.uint32)
    assert (bits == 0xffc12345).any() and (bits == 0x80000000).any() and (bits == 0x00000123).any() and np.isinf(xo).any()
    assert (fo == 200).any() and (fo == 1).any()


def test_more_than_one_block_per_clip():
    shape = (2, 16, 32, 48)
    _check(shape, [_row(shape, flip=True, reverse=True, y0=5, x0=9, ch=20, cw=31, a=1.1, b=-0.05), _row(shape)])


def test_refusals_of_the_hook():
    from sap3d_tensorflow_amd import ops, P3dError
    shape = (1, 2, 5, 7)
    x, y, fix = ar.random_clip(0, shape)
    for bad in (_row(shape, y0=3, ch=3), _row(shape, x0=4, cw=4), _row(shape, ch=0), _row(shape, cw=8), _row(shape, y0=-1, ch=2)):
        with pytest.raises(P3dError):                              # a window that leaves the frame is refused before any launch
            ops.augment(x, y, fix, [bad])
    with pytest.raises(P3dError):
        ops.augment(x, y, fix, [_row(shape)], offset=4)


# ---- 2: the draws --------------------------------------------------------------------------------------------------------------
def test_draws_are_the_replay():
    from sap3d_tensorflow_amd import ops
    rows = load_fixture()
    assert len(rows) >= 100
    for row in rows:
        cfg = dict(zip(CFG_KEYS, row["cfg"]))
        got = ops.augment_draw(row["seed"], row["g"], row["H"], row["W"], **cfg)
        assert _decision_ints(got) == row["decision"] == _decision_ints(ar.draw(row["seed"], row["g"], row["H"], row["W"], **cfg)), row


# ---- 3: net level --------------------------------------------------------------------------------------------------------------
_PARAMS = {}


def _params():
    if not _PARAMS:
        _PARAMS.update({k: np.asarray(v, f32) for k, v in p3d.init_params(1, "unet", CFG).items()})
    return _PARAMS


def _session(loss=None):
    from sap3d_tensorflow_amd import P3DSession
    B, T, H, W = SHAPE
    s = P3DSession("unet", batch=B, frames=T, height=H, width=W, base=CFG.base, blocks=CFG.blocks, seed=1)
    s.load(_params())
    s.set_adam(1e-3)
    if loss:
        s.set_loss(loss)
    return s


_BATCHES = {}


def _batch(j):
    """Batch j: clip, target, fixation maps and a seed whose decisions use every branch (computed once and shared)."""
    from sap3d_tensorflow_amd import synthetic as law
    if j not in _BATCHES:
        y = p3d.synthetic_target(3 + j, SHAPE)
        for seed in range(100 * j + 1, 100 * j + 100):
            d = ar.draws(seed, SHAPE[0], SHAPE[2], SHAPE[3], **AUG)
            if any(r[0] for r in d) and any(r[1] for r in d) and not all(r[0] for r in d) and all((r[4], r[5]) != SHAPE[2:] for r in d):
                break
        _BATCHES[j] = (p3d.synthetic_clip(j, SHAPE + (3,)), y, law.synthetic_fixations(20 + j, y), seed)
    return _BATCHES[j]


def _state(s):
    return {n: s.get_param(n) for n, _, _ in s.variables()}, {n: s.get_grad(n) for n, _, tr in s.variables() if tr}


def _assert_same_state(a, b):
    for part_a, part_b in zip(_state(a), _state(b)):
        for n in part_a:
            assert _same(part_a[n], part_b[n]), n


def _decisions(s):
    return [(d["flip"], d["reverse"], d["y0"], d["x0"], d["ch"], d["cw"], d["a"], d["b"]) for d in s.last_augment()]


@pytest.mark.parametrize("setting", ["smooth_l1", "kld_cc_nss", "accum2"])
def test_augmented_step_is_the_plain_step_on_the_replay(setting):
    loss = "kld_cc_nss" if setting == "kld_cc_nss" else None
    A, Bt = _session(loss), _session(loss)
    A.set_augment(**AUG)
    assert A.augment == {k: float(f32(v)) for k, v in AUG.items()} and Bt.augment is None
    steps = 2 if setting == "accum2" else 1
    if steps == 2:
        A.set_grad_accum(2)
        Bt.set_grad_accum(2)
    for j in range(steps):
        x, y, fix, seed = _batch(j)
        want = ar.draws(seed, SHAPE[0], SHAPE[2], SHAPE[3], **AUG)
        xa, ya, fa = ar.batch(x, y, fix if loss else None, want)
        assert not _same(xa, x) and not _same(ya, y)
        la = A.train_step(x, y, dropout=0.5, seed=seed, fixations=fix if loss else None)
        lb = Bt.train_step(xa, ya, dropout=0.5, seed=seed, fixations=fa)
        assert _decision_ints_all(_decisions(A)) == _decision_ints_all(want)
        assert f32(la).tobytes() == f32(lb).tobytes(), (setting, j, la, lb)
        assert A.last_augment_ms() > 0.0
        _assert_same_state(A, Bt)
        if loss:
            assert repr(A.last_loss_terms()) == repr(Bt.last_loss_terms()) and A.last_loss_terms()["counts"]["nss"] > 0
    assert A.optimizer_step() == Bt.optimizer_step() == 1
    A.close()
    Bt.close()


def _decision_ints_all(rows):
    return [_decision_ints(r) for r in rows]


def test_entry_points_that_never_augment_and_the_option_off():
    from sap3d_tensorflow_amd import P3dError
    from sap3d_tensorflow_amd._lib import lib
    x, y, _, seed = _batch(0)
    A, N = _session(), _session()                                  # N: never on
    for call in (lambda: A.augment_inputs(seed), A.last_augment, A.last_augment_ms):      # off: refused
        with pytest.raises(P3dError):
            call()
    A.set_augment(**AUG)
    with pytest.raises(P3dError):                                  # on, and nothing augmented yet
        A.last_augment()
    for s in (A, N):
        s.upload(x, y)
    sched = N.schedule(0.5, seed=1)
    assert A.schedule(0.5, seed=1) == sched                        # no launch enters the step's list
    assert not any("augment" in ln for ln in sched)
    _assert_same_state(A, N)
    # backward, forward, train_step_device and the schedule hook see the staged inputs as given
    la, pa = A.backward(x, y, dropout=0.5, seed=seed)
    ln, pn = N.backward(x, y, dropout=0.5, seed=seed)
    assert f32(la).tobytes() == f32(ln).tobytes() and _same(pa, pn)
    _assert_same_state(A, N)
    assert _same(A.forward(x), N.forward(x))
    for s in (A, N):
        s.upload(x, y)
        s.train_step_device(0.5, seed=seed)
    assert f32(A.last_loss()).tobytes() == f32(N.last_loss()).tobytes()
    _assert_same_state(A, N)
    with pytest.raises(P3dError):                                  # still nothing augmented
        A.last_augment()
    # an augmented step differs ...
    A.train_step(x, y, dropout=0.5, seed=seed)
    N.train_step(x, y, dropout=0.5, seed=seed)
    assert any(not _same(A.get_param(n), N.get_param(n)) for n, _, tr in A.variables() if tr)
    # ... and off after on is never on
    before = A.augment
    for bad in (dict(flip=1.5), dict(flip=-0.1), dict(reverse=2.0), dict(min_scale=0.0), dict(min_scale=1.5), dict(contrast=1.0),
                dict(contrast=-0.1), dict(brightness=-0.5), dict(brightness=float("inf")), dict(flip=float("nan"))):
        with pytest.raises(P3dError):
            A.set_augment(**dict(AUG, **bad))
        assert A.augment == before                                 # a refusal changes nothing
    rows = _decisions(A)
    assert A.augment is not None and lib().p3d_last_augment(A._h, None, None) == 0
    A.set_augment(None)
    assert A.augment is None and lib().p3d_augment_inputs(A._h, 1) == -1 and lib().p3d_last_augment(A._h, None, None) == -1
    A.set_augment()                                                # the neutral values are off as well
    assert A.augment is None
    for s in (A, N):
        s.load(_params())
        s.set_optimizer("sgd", lr=1e-4)                            # (a fresh optimiser on both: no slots left from above)
    x1, y1, _, seed1 = _batch(1)
    assert f32(A.train_step(x1, y1, dropout=0.5, seed=seed1)).tobytes() == f32(N.train_step(x1, y1, dropout=0.5, seed=seed1)).tobytes()
    _assert_same_state(A, N)
    assert A.schedule(0.5, seed=1) == N.schedule(0.5, seed=1)
    assert len(rows) == SHAPE[0]
    A.close()
    N.close()


def test_augment_inputs_then_the_device_step_is_the_train_step():
    x, y, fix, seed = _batch(1)
    A, D = _session("kld_cc_nss"), _session("kld_cc_nss")
    for s in (A, D):
        s.set_augment(**AUG)
    la = A.train_step(x, y, dropout=0.5, seed=seed, fixations=fix)
    D.upload(x, y, fixations=fix)
    D.augment_inputs(seed)
    D.train_step_device(0.5, seed=seed)
    assert f32(la).tobytes() == f32(D.last_loss()).tobytes()
    assert _decision_ints_all(_decisions(A)) == _decision_ints_all(_decisions(D))
    _assert_same_state(A, D)
    A.close()
    D.close()


# ---- 4: the driver -------------------------------------------------------------------------------------------------------------
def test_driver(tmp_path):
    from sap3d_tensorflow_amd import P3DSession, synthetic as law
    r = subprocess.run([sys.executable, os.path.join(ROOT, "drivers", "train.py"), "--aug-flip", "0.5", "--aug-min-scale", "0.8", "--steps", "2",
                        "--batch", "2", "--imagesize", "32", "32", "--plotiter", "1", "--validiter", "1000", "--saveiter", "1000",
                        "--info", "aug"], cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "Training Finished!" in r.stdout
    printed = [float(v) for v in re.findall(r"Training Loss (\S+)", r.stdout)]
    shape = (2, 16, 32, 32)
    s = P3DSession("unet", batch=2, frames=16, height=32, width=32, seed=0)
    s.set_adam(1e-4)
    s.set_augment(flip=0.5, min_scale=0.8)
    losses = [s.train_step(law.synthetic_clip(m, shape + (3,)), law.synthetic_target(10_000 + m, shape), dropout=0.5, seed=m + 1)
              for m in range(2)]
    s.close()
    assert printed == losses
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "drivers", "train.py"), "--aug-min-scale", "0", "--steps", "1", "--batch", "2",
                          "--imagesize", "32", "32"], cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert bad.returncode != 0 and "--aug-" in bad.stderr
