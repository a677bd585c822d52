"""Gradient clipping by the global norm (P3DSession.set_grad_clip) on the GPU: grad_sumsq_kernel and the scaled optimiser
launches at op level against tests/clip_ref.py, then the whole net.

Bounds.  Every term g^2 is an exact non-negative double and each of at most n additions rounds once, so
|sumsq - ref| <= n 2^-52 ref whatever the order; sqrt is correctly rounded on both sides and ref moves sumsq by far less than
an ulp at these n, so norm is held to 2 double ulps of sqrt(ref) and the float32 scale to 1 ulp of the reference's."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref                      # noqa: E402
import opt_ref                       # noqa: E402
import reg_ref                       # noqa: E402
from oracle import p3d               # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CH = 8192
SIZES = [1, 3, 4, 5, CH - 1, CH, CH + 1, 3 * CH + 7, 70 * CH]


def draws(n, seed):
    """normal draws times 1e4, one element in every thousand at 1e-3: a float32 accumulator loses the small ones and more"""
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(n) * 1e4).astype(f32)
    g[::1000] = f32(1e-3)
    return g


def check_sum(ss, nm, ref, n):
    print("n", n, "sumsq", repr(ss), "ref", repr(ref), "rel", abs(ss - ref) / ref, "norm ulps", clip_ref.ulps64(nm, math.sqrt(ref)))
    assert abs(ss - ref) <= n * 2.0 ** -52 * ref
    assert clip_ref.ulps64(nm, math.sqrt(ref)) <= 2


@pytest.mark.parametrize("n", SIZES)
def test_sum_norm_and_scale_at_every_size_and_offset(n):
    from sap3d_tensorflow_amd import ops
    g = draws(n, n)
    ref = clip_ref.sumsq64(g)
    rnorm = math.sqrt(ref)
    for offset in (0, 1, 3):
        ss, nm, sc = ops.grad_norm(g, rnorm / 4, offset=offset)
        check_sum(ss, nm, ref, n)
        want = clip_ref.scale32(rnorm, rnorm / 4)
        print("scale", sc, "ref", want)
        assert clip_ref.ulps32(sc, want) <= 1
        for clip in (2 * rnorm, np.inf):
            ss2, nm2, sc2 = ops.grad_norm(g, clip, offset=offset)
            assert (ss2, nm2) == (ss, nm)
            assert f32(sc2).tobytes() == f32(1.0).tobytes()


def test_results_do_not_depend_on_the_cut_the_order_the_grid_or_the_run():
    from sap3d_tensorflow_amd import ops
    n = 4 * CH + 77                      # 5 chunks
    g = draws(n, 7)
    clip = math.sqrt(clip_ref.sumsq64(g)) / 4

    def bits(r):
        return (np.float64(r[0]).tobytes(), np.float64(r[1]).tobytes(), f32(r[2]).tobytes())
    for offset in (0, 3):
        whole = bits(ops.grad_norm(g, clip, offset=offset))
        assert bits(ops.grad_norm(g, clip, offset=offset)) == whole                      # run to run
        for k in range(1, 5):
            cut = k * CH
            assert bits(ops.grad_norm(g, clip, ranges=[(cut, n), (0, cut)], offset=offset)) == whole, k
            assert bits(ops.grad_norm(g, clip, ranges=[(0, cut), (cut, n)], offset=offset)) == whole, k
        for blocks in (1, 2, 3):
            assert bits(ops.grad_norm(g, clip, blocks=blocks, offset=offset)) == whole, blocks
    big = draws(70 * CH, 70)             # more partials than a wave is wide, on one block and on many
    assert bits(ops.grad_norm(big, 1.0, blocks=1)) == bits(ops.grad_norm(big, 1.0)) == bits(ops.grad_norm(big, 1.0, blocks=7))


def test_tile_table_with_coefficients_and_padding():
    """g' = f32(g + f32(c w)) on the tiles with a coefficient; the padding tile belongs to no chunk: it holds NaN here, so a
    kernel that read it could not meet the bound."""
    from sap3d_tensorflow_amd import ops
    tiles = [(CH, 0.0), (CH, 1e-3), (100, None), (CH, 0.0), (CH - 3, 1e-3), (7, 0.0), (5, 1e-3)]
    n = sum(t[0] for t in tiles)
    rng = np.random.default_rng(3)
    g = draws(n, 5)
    w = (rng.standard_normal(n) * 1e6).astype(f32)
    parts, at = [], 0
    for length, c in tiles:
        if c is None:
            g[at:at + length] = np.nan
            w[at:at + length] = np.nan
        else:
            parts.append(reg_ref.decayed_grad32(g[at:at + length], c, w[at:at + length]) if c else g[at:at + length])
        at += length
    ref = clip_ref.sumsq64(np.concatenate(parts))
    for offset in (0, 1, 3):
        ss, nm, sc = ops.grad_norm(g, math.sqrt(ref) / 4, p=w, tiles=tiles, offset=offset)
        check_sum(ss, nm, ref, n)
        assert clip_ref.ulps32(sc, clip_ref.scale32(math.sqrt(ref), math.sqrt(ref) / 4)) <= 1
    cut = 2 * CH + 100                   # between the padding and the next variable
    a = ops.grad_norm(g, 1.0, p=w, tiles=tiles)
    assert ops.grad_norm(g, 1.0, p=w, tiles=tiles, ranges=[(cut, n), (0, cut)]) == a
    assert ops.grad_norm(g, 1.0, p=w, tiles=tiles, ranges=[(2 * CH, n), (0, 2 * CH)]) == a


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_nan_or_an_inf_gradient_gives_a_nan_scale(bad):
    from sap3d_tensorflow_amd import ops
    g = draws(CH + 5, 1)
    g[CH + 1] = bad
    for clip in (1.0, np.inf):
        ss, nm, sc = ops.grad_norm(g, clip)
        assert not math.isfinite(nm) and np.isnan(sc)


def test_bad_arguments_are_refused():
    from sap3d_tensorflow_amd import ops, P3dError
    g = draws(2 * CH, 2)
    for clip in (0.0, -1.0, np.nan):
        with pytest.raises(P3dError):
            ops.grad_norm(g, clip)
    with pytest.raises(P3dError):
        ops.grad_norm(g, 1.0, ranges=[(0, CH)])                       # a chunk nobody takes
    with pytest.raises(P3dError):
        ops.grad_norm(g, 1.0, ranges=[(0, CH + 1), (CH + 1, 2 * CH)])  # a range that cuts a chunk
    with pytest.raises(P3dError):
        ops.grad_norm(g, 1.0, tiles=[(CH, 1e-3), (CH, 0.0)])          # a coefficient without parameters


KINDS = ["adam", "momentum", "nesterov", "sgd"]


@pytest.mark.parametrize("n", [5, CH + 1])
@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_scaled_optimiser_launch_equals_the_unscaled_one_on_the_scaled_gradient(kind, tiled, n):
    """The yardstick is the parent's kernels (test_gpu_optimizer.py, test_gpu_regularization.py pin them): the scaled launch
    on g equals the unscaled launch fed f32(g' s), bit for bit, in p, m and v."""
    from sap3d_tensorflow_amd import ops
    rng = np.random.default_rng(n + len(kind))
    p, g, m = ((rng.standard_normal(n) * sc).astype(f32) for sc in (1.0, 10.0, 1.0))
    v = (rng.random(n) * 50).astype(f32)
    s = f32(0.37)
    tiles = [(n // 2 + 1, 1e-3), (n - n // 2 - 1, 0.0)] if tiled else None
    gp = g
    if tiled:
        k = tiles[0][0]
        gp = np.concatenate([reg_ref.decayed_grad32(g[:k], 1e-3, p[:k]), g[k:]])
    g2 = clip_ref.scaled32(gp, s)
    assert not np.array_equal(g2, gp)
    if kind == "adam":
        want = ops.adam(p, g2, m, v, t=3, lr=1e-2)[:3]
        if tiled:
            r = ops.adam_decay(p, g, m, v, tiles, t=3, lr=1e-2, gscale=s)
            got, gback = r[1:4], r[0]
        else:
            got, gback = ops.adam(p, g, m, v, t=3, lr=1e-2, gscale=s)[:3], None
    else:
        name, nest = ("sgd", False) if kind == "sgd" else ("momentum", kind == "nesterov")
        want = ops.optimizer(name, p, g2, m, lr=1e-2, use_nesterov=nest)
        if tiled:
            r = ops.optimizer_decay(name, p, g, m, tiles, lr=1e-2, use_nesterov=nest, gscale=s)
            got, gback = r[1:3], r[0]
        else:
            got, gback = ops.optimizer(name, p, g, m, lr=1e-2, use_nesterov=nest, gscale=s), None
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert not np.array_equal(got[0], p)
    if gback is not None:
        assert np.array_equal(gback, gp)          # the gradient comes back with the decay's part and without the scale


# ---- whole net ---------------------------------------------------------------------------------------------------------
CFG, SHAPE = p3d.NetConfig(base=8, blocks=(3, 3, 3)), (2, 16, 32, 32)      # test_gpu_net.SMALL[0]


def session(seed=1):
    from sap3d_tensorflow_amd import P3DSession
    return P3DSession("unet", batch=SHAPE[0], frames=SHAPE[1], height=SHAPE[2], width=SHAPE[3], base=CFG.base, blocks=CFG.blocks,
                      seed=seed)


@pytest.fixture(scope="module")
def data():
    x, y = p3d.synthetic_clip(0, SHAPE + (3,)), p3d.synthetic_target(3, SHAPE)
    x.setflags(write=False); y.setflags(write=False)
    return x, y


def trainables(s):
    return [n for n, _, tr in s.variables() if tr]


def grads(s):
    return {n: s.get_grad(n) for n in trainables(s)}


def params(s):
    return {n: s.get_param(n) for n in trainables(s)}


def all_params(s):
    return {n: s.get_param(n) for n, _, _ in s.variables()}


def norm_ref(g):
    return clip_ref.sumsq64(np.concatenate([v.ravel() for v in g.values()])), sum(v.size for v in g.values())


def check_reported(s, ref, n, clip):
    nm, sc, ss = s.last_grad_norm(with_sumsq=True)
    check_sum(ss, nm, ref, n)
    want = clip_ref.scale32(math.sqrt(ref), clip)
    print("scale", sc, "ref", want)
    assert clip_ref.ulps32(sc, want) <= 1
    return f32(sc)


@pytest.mark.parametrize("kind", ["sgd", "momentum", "nesterov"])
def test_clipped_step_is_the_replay_of_the_optimiser_on_the_scaled_gradient(kind, data):
    x, y = data
    s = session()
    lr, steps = 1e-4, (1 if kind == "sgd" else 2)
    s.set_optimizer("sgd" if kind == "sgd" else "momentum", lr=lr, momentum=0.9, use_nesterov=kind == "nesterov")
    acc = {n: np.zeros_like(v) for n, v in params(s).items()}
    clip = None
    for t in range(steps):
        s.backward(x, y, dropout=0.5, seed=11 + t)          # the backward's bits are the train step's (test_gpu_determinism.py)
        g, p0 = grads(s), params(s)
        ref, n = norm_ref(g)
        if clip is None:
            clip = float(f32(math.sqrt(ref) / 4))
            s.set_grad_clip(clip)
        s.train_step(x, y, dropout=0.5, seed=11 + t)
        sc = check_reported(s, ref, n, clip)
        assert sc < 1
        p1 = params(s)
        for name in g:
            assert np.array_equal(s.get_grad(name), g[name]), name          # the gradient buffer is not rewritten
            wp, acc[name] = opt_ref.update32(kind, p0[name], acc[name], clip_ref.scaled32(g[name], sc), lr, 0.9)
            assert np.array_equal(p1[name], wp), (t, name)
    s.close()


@pytest.mark.parametrize("setup", ["adam", "momentum", "adam+weightdecay"])
def test_a_threshold_never_reached_gives_the_unclipped_bits(setup, data):
    x, y = data
    runs = []
    for clip in (None, 1e30):
        s = session(seed=5)
        if setup == "momentum":
            s.set_optimizer("momentum", lr=1e-7)
        if setup.endswith("weightdecay"):
            s.set_regularization(("weightdecay",))
        if clip:
            s.set_grad_clip(clip)
        losses = []
        for i in range(3):
            losses.append(f32(s.train_step(x, y, dropout=0.5, seed=100 + i)).tobytes())
            if clip:
                assert f32(s.last_grad_norm()[1]).tobytes() == f32(1.0).tobytes()
        runs.append((losses, all_params(s)))
        s.close()
    assert runs[0][0] == runs[1][0]
    for n, v in runs[0][1].items():
        assert np.array_equal(v, runs[1][1][n]), n


def test_norm_with_regularisation_is_that_of_g_plus_c_w(data):
    x, y = data
    s = session()
    s.backward(x, y, dropout=0.5, seed=11)
    g, w = grads(s), params(s)
    s.set_regularization(("weightdecay",))
    s.set_grad_clip(float("inf"))
    s.backward(x, y, dropout=0.5, seed=11)
    gp = {}
    for n in g:
        c = f32(sum(s.param_regularization(n)))
        gp[n] = reg_ref.decayed_grad32(g[n], c, w[n]) if c else g[n]
    assert any(not np.array_equal(gp[n], g[n]) for n in g)
    ref, n = norm_ref(gp)
    assert check_reported(s, ref, n, np.inf).tobytes() == f32(1.0).tobytes()
    for name in g:
        assert np.array_equal(s.get_grad(name), gp[name]), name          # what backward returns with the term on, unscaled
    s.close()


def test_off_is_off_and_the_schedule_shows_the_sums_before_the_optimiser(data):
    from sap3d_tensorflow_amd import P3dError
    x, y = data
    s = session()
    s.upload(x, y)
    fresh = s.schedule(0.5, 3)
    with pytest.raises(P3dError):
        s.last_grad_norm()
    s.set_grad_clip(1.0)
    with pytest.raises(P3dError):
        s.last_grad_norm()                       # on, but no step yet
    on = s.schedule(0.5, 3)
    launches = [l.split()[2] for l in on if l.startswith("L ")]
    sums = [i for i, k in enumerate(launches) if k == "grad_sumsq_kernel"]
    opts = [i for i, k in enumerate(launches) if re.fullmatch(r"(adam|momentum|sgd)(_decay)?(_scaled)?_kernel", k)]
    assert sums and opts and max(sums) < min(opts)
    assert all(launches[i] == "adam_scaled_kernel" for i in opts)
    assert not any("grad_sumsq_kernel" in l for l in fresh)
    assert math.isfinite(s.last_grad_norm()[0])
    s.set_grad_clip(0)
    with pytest.raises(P3dError):
        s.last_grad_norm()
    assert s.schedule(0.5, 3) == fresh
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            s.set_grad_clip(bad)
    s.close()


def test_captured_step_with_clipping_replays_the_eager_bits():
    """As test_gpu_determinism.py switches the capture path on: P3D_GRAPH is read once per process, so both runs are children."""
    script = (
        "import sys, hashlib, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "from oracle import p3d\n"
        "from sap3d_tensorflow_amd import P3DSession\n"
        "shape = (2, 16, 32, 32)\n"
        "s = P3DSession('unet', batch=2, frames=16, height=32, width=32, base=8, blocks=(3, 3, 3), seed=3)\n"
        "s.set_optimizer('momentum', lr=1e-4)\n"
        "s.set_grad_clip(1.0)\n"
        "s.upload(p3d.synthetic_clip(0, shape + (3,)), p3d.synthetic_target(3, shape))\n"
        "out = []\n"
        "for i in range(3):\n"
        "    s.train_step_device(0.5, seed=50 + i)\n"
        "    nm, sc = s.last_grad_norm()\n"
        "    assert 0 < sc < 1, sc\n"
        "    out += [np.float32(s.last_loss()).tobytes().hex(), np.float64(nm).tobytes().hex(), np.float32(sc).tobytes().hex()]\n"
        "h = hashlib.sha256()\n"
        "for n, _, _ in s.variables():\n"
        "    h.update(s.get_param(n).tobytes())\n"
        "print('RESULT', ' '.join(out), h.hexdigest())\n"
        "s.close()\n" % ROOT)
    outs = []
    for graph in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, P3D_GRAPH=graph), capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT")]
        assert line, r.stdout[-2000:]
        outs.append(line[0])
        if graph == "1":
            assert "capture failed" not in r.stderr, r.stderr[-2000:]
    assert outs[0] == outs[1]


def test_train_driver_prints_the_norm_and_the_scale(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "drivers", "train.py"), "--batch", "2", "--imagesize", "32", "32",
                        "--steps", "2", "--plotiter", "1", "--validiter", "100", "--saveiter", "100", "--info", "c",
                        "--optimizer", "sgd", "--clip-norm", "1.0"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    m = re.findall(r"Training Loss (\S+) gnorm (\S+) scale (\S+)", r.stdout)
    assert len(m) == 2, r.stdout[-2000:]
    for loss, gn, sc in m:
        assert math.isfinite(float(loss)) and math.isfinite(float(gn)) and 0.0 < float(sc) <= 1.0
