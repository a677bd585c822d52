"""A read-out facility's test hook runs the stage its op entry point runs: the same carve, upload, launches and copies back, the
hook's inside a block of its own with every buffer between guards, the op's on the stream's scratch.  At offset 0 both see the same
alignment modulo 16, so what they return is equal bit for bit, floats included -- once per option that changes the stage's list of
buffers.  (The other offsets, and the values themselves, are the business of each facility's own tests.)  3 maps of 7 x 19 bytes;
distortion takes 12 x 19, the smallest of this width with more than one row of SSIM windows."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distortion_ref       # noqa: E402

N, H, W = 3, 7, 19
SHOTS = [0, 2]


@functools.lru_cache(maxsize=None)
def inputs(H=H):
    rng = np.random.RandomState(11)
    yy, xx = np.mgrid[0:H, 0:W]
    sal = np.stack([255.0 * np.exp(-((yy - 2 - k) ** 2 / 6.0 + (xx - 5 - 4 * k) ** 2 / 14.0)) for k in range(N)])
    sal = np.clip(sal + rng.randint(0, 40, sal.shape), 0, 255).astype(np.uint8)
    density = rng.randint(0, 256, (N, H, W)).astype(np.uint8)
    fixation = np.where(rng.rand(N, H, W) < 0.1, 255, 0).astype(np.uint8)
    frames = rng.randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    assert (fixation.reshape(N, -1) >= 128).sum(axis=1).min() >= 2
    for a in (sal, density, fixation, frames):
        a.setflags(write=False)
    return sal, density, fixation, frames


def same(hook, op, tag):
    """Every array the two calls return holds the same bits (a None on one side is a None on the other)."""
    hook = hook if isinstance(hook, tuple) else (hook,)
    op = op if isinstance(op, tuple) else (op,)
    assert len(hook) == len(op), tag
    for i, (a, b) in enumerate(zip(hook, op)):
        if a is None or b is None:
            assert a is None and b is None, tag + (i,)
            continue
        assert a.dtype == b.dtype and a.shape == b.shape, tag + (i, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), tag + (i, np.argwhere(a != b)[:4].tolist())


@pytest.mark.parametrize("with_frames", [True, False])
@pytest.mark.parametrize("contour", [None, 128])
def test_render(with_frames, contour):
    from sap3d_tensorflow_amd import dataflow
    sal, _, _, frames = inputs()
    kw = dict(contour=contour, thickness=2)
    args = (sal, frames if with_frames else None, dataflow.render_table())
    same(dataflow.render_overlay(*args, offset=0, **kw), dataflow.render_overlay(*args, **kw), ("render", with_frames, contour))


@pytest.mark.parametrize("with_frames", [True, False])
@pytest.mark.parametrize("shots", [None, SHOTS])
def test_reframe(with_frames, shots):
    from sap3d_tensorflow_amd import dataflow
    sal, _, _, frames = inputs()
    kw = dict(gate=20, smooth=1, shots=shots)
    args = (sal, frames if with_frames else None, (3, 5))
    same(dataflow.reframe(*args, offset=0, **kw), dataflow.reframe(*args, **kw), ("reframe", with_frames, shots))


@pytest.mark.parametrize("kw", [dict(labels=True), dict(labels=False), dict(labels=True, link=True, shots=SHOTS)],
                         ids=["labels", "records", "link-shots"])
def test_regions(kw):
    from sap3d_tensorflow_amd import dataflow
    sal = inputs()[0]
    same(dataflow.regions(sal, 100, offset=0, **kw), dataflow.regions(sal, 100, **kw), ("regions", sorted(kw.items())))


@pytest.mark.parametrize("kw", [dict(levels=True, stats=True), dict(levels=False, stats=False), dict(levels=True, stats=True, shots=SHOTS)],
                         ids=["full", "offsets", "shots"])
def test_qpmap(kw):
    from sap3d_tensorflow_amd import dataflow
    sal = inputs()[0]
    law = dataflow.qp_law(-20, 6)
    kw = dict(kw, block=8, dilate=1, fall=1, rise=3)
    same(dataflow.qpmap(sal, law, offset=0, **kw), dataflow.qpmap(sal, law, **kw), ("qpmap", sorted(kw.items())))


@pytest.mark.parametrize("shots", [None, SHOTS])
@pytest.mark.parametrize("grid", [True, False])
@pytest.mark.parametrize("passes", [1, 2])      # 1: no temporary; 2: one
def test_prefilter(passes, grid, shots):
    from sap3d_tensorflow_amd import dataflow
    sal, _, _, frames = inputs()
    law = dataflow.prefilter_law(gate=200, full=20)
    kw = dict(block=8, dilate=1, fall=2, rise=4, radius=2, passes=passes, grid=grid, shots=shots)
    same(dataflow.prefilter(sal, frames, law, offset=0, **kw), dataflow.prefilter(sal, frames, law, **kw), ("prefilter", passes, grid, shots))


@pytest.mark.parametrize("block", [0, 8])       # 0: no block map; 8: one
def test_distortion(block):
    from sap3d_tensorflow_amd import dataflow
    rows, cols = distortion_ref.windows(12, W)
    assert rows and cols                         # SSIM has windows
    sal, _, _, ref = inputs(12)
    test = distortion_ref.near(ref, 3)
    args = (sal, ref, test, (block, 100), dataflow.distortion_law(gate=100, floor=1))
    hook, op = dataflow.distortion(*args, offset=0), dataflow.distortion(*args)
    assert (op[1] is None) == (block == 0)
    same(hook, op, ("distortion", block))


@pytest.mark.parametrize("with_fixation", [True, False])
def test_score(with_fixation):
    from sap3d_tensorflow_amd import metrics
    sal, density, fixation, _ = inputs()
    flags = ("cc", "sim", "judd", "kl", "nss") if with_fixation else ("cc", "sim", "kl")
    args = (sal, density, fixation if with_fixation else None)
    hook, tables = metrics.score_bytes(*args, flags=flags, with_tables=True, offset=0)
    same(hook, metrics.score_bytes(*args, flags=flags), ("score", with_fixation))
    assert tables["hs"].shape == (N, 256)


def test_sweep():
    from sap3d_tensorflow_amd import metrics
    sal, _, fixation, _ = inputs()
    idx, nf = metrics.borji_draws_u8(fixation, 3, np.random.RandomState(5))
    hook, tables = metrics.score_sweep(sal, fixation, idx, nf, with_tables=True, offset=0, n_rep=3)
    assert hook.shape == (N, 3) and tables["top"].shape == (N, 3)
    same(hook, metrics.score_sweep(sal, fixation, idx, nf, n_rep=3), ("sweep",))
