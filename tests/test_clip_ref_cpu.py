"""No-GPU checks of gradient clipping: the reference of tests/clip_ref.py against torch.nn.utils.clip_grad_norm_, its exact 1
below the threshold, and the boundary (ABI symbols, ctypes signatures, Python entry points, the driver's flag)."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import clip_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_scale_agrees_with_torch_clip_grad_norm(seed):
    """torch scales by clip / (norm + 1e-6), clamped to 1: the 1e-6 is the whole difference (2e-6 relative at norms >= 1)."""
    import torch
    rng = np.random.default_rng(seed)
    gs = [rng.standard_normal(s) * 10.0 ** rng.integers(-1, 3) for s in ((7, 5), (33,), (4, 3, 2))]
    gs = [g.astype(np.float32) for g in gs]      # the reference takes float32 gradients: torch gets the same values, in float64
    ps = [torch.nn.Parameter(torch.zeros(g.shape, dtype=torch.float64)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = torch.tensor(g.astype(np.float64))
    norm = math.sqrt(clip_ref.sumsq64(np.concatenate([g.ravel() for g in gs])))
    clip = float(np.float32(norm / 3.0))
    total = torch.nn.utils.clip_grad_norm_(ps, clip)
    assert abs(float(total) - norm) <= 1e-12 * norm
    s = float(clip_ref.scale32(norm, clip))
    for p, g in zip(ps, gs):
        ratio = p.grad.numpy() / g.astype(np.float64)
        assert np.all(np.abs(ratio / s - 1.0) <= 2e-6)


def test_reference_scale_is_exactly_one_at_and_below_the_threshold():
    for norm in (0.0, 1e-30, 0.5, 1.0, 123.456, 3.0e7):
        for clip in (norm, norm * (1 + 1e-7) + 1e-38, norm * 2 + 1.0, np.inf):
            c = float(np.float32(clip))
            if c >= norm and c > 0:
                assert clip_ref.scale32(norm, c).tobytes() == np.float32(1.0).tobytes(), (norm, clip)
    assert clip_ref.scale32(4.0, 1.0) == np.float32(0.25)
    assert np.isnan(clip_ref.scale32(np.inf, 1.0)) and np.isnan(clip_ref.scale32(np.nan, np.inf))
    g = np.array([3.0, -4.0], np.float32)
    assert clip_ref.sumsq64(g) == 25.0
    assert np.array_equal(clip_ref.scaled32(g, 1.0), g)


def test_abi_symbols_and_python_entry_points_exist():
    from sap3d_tensorflow_amd import _lib, ops, P3DSession
    hdr = open(os.path.join(ROOT, "include", "p3d_hip.h")).read()
    for decl in (r"int p3d_set_grad_clip\(p3d_handle\* h, float clip_norm\);",
                 r"int p3d_get_grad_norm\(p3d_handle\* h, double\* sumsq, double\* norm, float\* scale\);",
                 r"int p3d_debug_grad_norm\(int device,", r"int p3d_debug_opt_scaled\(int device, int kind,"):
        assert re.search(decl, hdr), decl
    lib = _lib.lib()
    for sym in ("p3d_set_grad_clip", "p3d_get_grad_norm", "p3d_debug_grad_norm", "p3d_debug_opt_scaled"):
        assert hasattr(lib, sym), sym
        assert sym in _lib.SIGNATURES, sym
    assert callable(P3DSession.set_grad_clip) and callable(P3DSession.last_grad_norm)
    assert list(inspect.signature(ops.grad_norm).parameters)[:6] == ["g", "clip_norm", "p", "tiles", "ranges", "offset"]
    for fn in (ops.adam, ops.adam_decay, ops.optimizer, ops.optimizer_decay):
        assert inspect.signature(fn).parameters["gscale"].default is None, fn.__name__
    assert lib.p3d_set_grad_clip(None, 1.0) == -1          # null handle: an error, not a crash
    src = open(os.path.join(ROOT, "drivers", "train.py")).read()
    assert '"--clip-norm"' in src and "[addition] clip the gradients" in src
