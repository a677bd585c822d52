"""No-GPU checks of the moving average of the weights: the replay of tests/ema_ref.py against its closed forms and the float64
recurrence, why the ABI takes the decay as a double, the shadows' names through a TF bundle, and the boundary (header symbols,
ctypes signatures, Python entry points, the drivers' flags)."""
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import ema_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.mark.parametrize("decay", [0.999, 0.9, 0.5])
def test_warmup_decay_follows_its_closed_form_and_reaches_the_decay(decay):
    """d_t = min(decay, (1 + t) / (10 + t)).  1 + t and 10 + t are exact in float32 at these t, so the quotient is the exact
    ratio rounded once: float32(Fraction)."""
    for t in (1, 2, 3, 100):
        q = f32(float(Fraction(1 + t, 10 + t)))       # Fraction -> double -> float32: double rounding cannot bite at 8-bit integers
        assert f32(1 + t) / f32(10 + t) == q
        assert ema_ref.decay_warmup(decay, t) == min(f32(decay), q), t
        assert ema_ref.om_warmup(decay, t) == f32(1.0) - min(f32(decay), q), t
    assert ema_ref.decay_warmup(0.999, 1) == f32(2.0) / f32(11.0)
    # from the first t with (1 + t) / (10 + t) >= decay on, d_t is float32(decay): t >= (10 decay - 1) / (1 - decay)
    first = next(t for t in range(1, 20000) if f32(1 + t) / f32(10 + t) >= f32(decay))
    exact = (10 * Fraction(decay) - 1) / (1 - Fraction(decay))
    assert abs(first - exact) <= 1 + 2.0 ** -22 * float(exact) * 10      # float32's rounding of the ratio moves the crossing by a step at most
    for t in (first, first + 1, 2 * first, 10 ** 6):
        assert ema_ref.decay_warmup(decay, t) == f32(decay), t
    if first > 1:
        assert ema_ref.decay_warmup(decay, first - 1) < f32(decay)


def test_constant_om_is_the_double_subtraction_rounded_once():
    """The reason p3d_set_ema takes a double: float32(1.0 - 0.999) is not 1.f - 0.999f."""
    via_double = ema_ref.om_const(0.999)
    via_float = f32(1.0) - f32(0.999)
    assert via_double == f32(1.0 - 0.999)
    assert via_double != via_float
    assert ema_ref.om(0.999) == via_double and ema_ref.om(0.999, True, 10 ** 6) == via_float      # warm-up is float32 throughout


def test_replay_rounds_every_operation():
    s, p, om = f32(1.0), f32(1.0 - 2.0 ** -24), f32(0.1)
    assert ema_ref.update32([s], [p], om)[0] == f32(s - f32(f32(s - p) * om))
    x = np.array([0.0, 1.5, -2.25, 1e-40], f32)
    assert np.array_equal(ema_ref.update32(x, x, 0.25).view(np.uint32), x.view(np.uint32))      # s == p: unchanged, denormals too


def test_200_steps_against_the_float64_recurrence():
    """s_k in float32 against float64 on a fixed target.  One step is s' = fl(s - fl(fl(s - p) om)): three roundings, each at
    most u = 2^-24 relative to a value bounded by max|s| + max|p| <= 2 M, M = max(|s_0|, |p|) (s stays between s_0 and p); the
    product's factor om < 1 only shrinks the first two.  The recurrence contracts errors by decay < 1, so they add at most
    linearly: |s32 - s64| <= 200 * 3 * 2 M u, plus om's own rounding, 200 * u * 2 M.  Bound: 200 * 2^-24 * 8 M."""
    rng = np.random.default_rng(0)
    decay = 0.99
    s0 = rng.standard_normal(4096).astype(f32)
    p = rng.standard_normal(4096).astype(f32)
    s32, s64 = s0.copy(), s0.astype(np.float64)
    om = ema_ref.om_const(decay)
    for _ in range(200):
        s32 = ema_ref.update32(s32, p, om)
        s64 = ema_ref.update64(s64, p, decay)
    M = max(float(np.abs(s0).max()), float(np.abs(p).max()))
    tol = 200 * 2.0 ** -24 * 8 * M
    err = float(np.abs(s32.astype(np.float64) - s64).max())
    print("200 steps: error %.3g, tolerance %.3g" % (err, tol))
    assert err <= tol
    assert float(np.abs(s64 - p).max()) < float(np.abs(s0.astype(np.float64) - p).max()) * decay ** 200 * (1 + 1e-9)


def test_shadow_names_round_trip_through_a_bundle(tmp_path):
    from sap3d_tensorflow_amd import tf_checkpoint as tfc
    from sap3d_tensorflow_amd.session import EMA_SUFFIX, ema_names
    assert EMA_SUFFIX == ema_ref.SUFFIX
    variables = [("conv1/kernel", (1, 3, 3, 3, 4), True), ("conv1/bn/gamma", (4,), True), ("conv1/bn/moving_mean", (4,), False)]
    names = ema_names(variables)
    assert names == {"conv1/kernel/ExponentialMovingAverage": "conv1/kernel", "conv1/bn/gamma/ExponentialMovingAverage": "conv1/bn/gamma"}
    rng = np.random.default_rng(1)
    bundle = {n: rng.standard_normal(shp).astype(f32) for n, shp, _ in variables}
    bundle.update({k: rng.standard_normal(bundle[n].shape).astype(f32) for k, n in names.items()})
    prefix = str(tmp_path / "p3d_1.ckpt")
    tfc.write_checkpoint(prefix, bundle)
    listed = set(k for k, _, _ in tfc.list_variables(prefix))
    assert listed == set(bundle)
    assert set(k for k in listed if k.endswith("/" + ema_ref.SUFFIX)) == set(ema_ref.shadow_name(n) for n, _, tr in variables if tr)
    back = tfc.read_checkpoint(prefix, names=set(names))
    assert set(back) == set(names)
    for k in names:
        assert np.array_equal(back[k].view(np.uint32), bundle[k].view(np.uint32))


ABI = ("p3d_set_ema", "p3d_get_ema", "p3d_set_ema_var", "p3d_ema_swap", "p3d_ema_swapped", "p3d_debug_ema")


def test_boundary():
    import ctypes as C
    from sap3d_tensorflow_amd import _lib, ops
    from sap3d_tensorflow_amd.session import P3DSession
    header = open(os.path.join(ROOT, "include", "p3d_hip.h")).read()
    for name in ABI:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["p3d_set_ema"][1][1] is C.c_double          # the decay crosses the ABI as a double
    for m in ("set_ema", "get_ema", "set_ema_var", "ema_swap", "averaged", "ema_state"):
        assert callable(getattr(P3DSession, m)), m
    assert "ema" in inspect.signature(P3DSession.save_checkpoint).parameters
    assert {"ema", "ema_as_weights"} <= set(inspect.signature(P3DSession.restore).parameters)
    assert callable(ops.ema)
    for drv, flags in (("train.py", ("--ema-decay", "--ema-warmup")), ("test.py", ("--ema",)), ("gen_pred.py", ("--ema",))):
        text = open(os.path.join(ROOT, "drivers", drv)).read()
        for f in flags:
            assert '"%s"' % f in text, (drv, f)
