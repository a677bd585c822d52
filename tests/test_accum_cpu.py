"""No-GPU checks of gradient accumulation over micro-batches: the replay of tests/accum_ref.py (its fixed order, signed zeros,
denormals, and that the inputs the GPU tests feed it hold no NaN), and the boundary (header symbols, ctypes signatures, Python
entry points, the driver's flag)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import accum_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _bits(a):
    return np.asarray(a, f32).view(np.uint32)


def test_the_order_is_left_to_right():
    """((g0 + g1) + g2) is what the library applies; float32 addition is not associative, so another order gives other bits on
    some elements of a seeded case -- and on a hand-made one: (1 + 2^-24) + 2^-24 = 1 (two ties to even), 1 + (2^-24 + 2^-24)
    = 1 + 2^-23."""
    rng = np.random.default_rng(0)
    g = [(rng.standard_normal(4096) * 10.0 ** rng.integers(-2, 3, 4096)).astype(f32) for _ in range(3)]
    want = (f32(1) * g[0] + g[1]).astype(f32)
    want = (want + g[2]).astype(f32)
    got = accum_ref.cycle(g)
    assert np.array_equal(_bits(got), _bits(want))
    other = (g[0] + (g[1] + g[2]).astype(f32)).astype(f32)
    swapped = ((g[0] + g[2]).astype(f32) + g[1]).astype(f32)
    n_other, n_swapped = int((_bits(got) != _bits(other)).sum()), int((_bits(got) != _bits(swapped)).sum())
    print("elements that differ from g0 + (g1 + g2): %d, from (g0 + g2) + g1: %d of 4096" % (n_other, n_swapped))
    assert n_other > 0 and n_swapped > 0
    exact = (g[0].astype(np.float64) + g[1].astype(np.float64)) + g[2].astype(np.float64)
    # two roundings, each at most half an ulp of a partial sum bounded by sum |g_j|
    assert np.all(np.abs(got.astype(np.float64) - exact) <= 2 * 2.0 ** -24 * sum(np.abs(t).astype(np.float64) for t in g))
    u = f32(2.0 ** -24)
    assert accum_ref.cycle([np.array([1.0], f32), np.array([u], f32), np.array([u], f32)])[0] == f32(1.0)
    assert accum_ref.cycle([np.array([u], f32), np.array([u], f32), np.array([1.0], f32)])[0] == f32(1.0) + f32(2.0 ** -23)


def test_one_micro_batch_is_a_copy_and_the_sum_is_not_a_mean():
    g = np.array([1.5, -0.0, 3e-41, -np.inf], f32)
    assert np.array_equal(_bits(accum_ref.cycle([g])), _bits(g))
    assert np.array_equal(accum_ref.cycle([g[:1]] * 4), np.array([6.0], f32))


def test_signed_zeros_and_denormals():
    nz, pz = f32(-0.0), f32(0.0)
    assert _bits(accum_ref.store([nz]))[0] == 0x80000000                    # a store keeps -0
    assert _bits(accum_ref.add32([pz], [nz]))[0] == 0                       # +0 + -0 = +0
    assert _bits(accum_ref.add32([nz], [nz]))[0] == 0x80000000              # -0 + -0 = -0
    assert _bits(accum_ref.add32([f32(1.25)], [f32(-1.25)]))[0] == 0        # exact cancellation gives +0
    a, b = f32(3e-41), f32(5e-42)
    s = accum_ref.add32([a], [b])[0]
    assert s != 0 and s < np.finfo(f32).tiny                                # denormals are not flushed,
    assert float(s) == float(a) + float(b)                                  # and their sum is exact
    assert np.array_equal(_bits(accum_ref.finish([a], [b])), _bits(accum_ref.add32([a], [b])))
    assert accum_ref.add32([f32(3e38)], [f32(3e38)])[0] == np.inf


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4097, 2 ** 20 + 3])
def test_op_inputs_hold_every_special_case_and_no_nan(n):
    """What test_gpu_grad_accum.py feeds the kernel: no NaN goes in and none comes out of any mode, so bit comparisons are
    comparisons of values; from 1023 elements on every special case is present."""
    for offset in range(4):
        acc, g = accum_ref.special_inputs(n + 2, n * 3 + offset)
        assert not np.isnan(acc).any() and not np.isnan(g).any()
        for mode in accum_ref.MODES:
            assert not np.isnan(accum_ref.launch(mode, acc, g)).any(), mode
        if n >= 1023:
            tiny = np.finfo(f32).tiny
            s = accum_ref.add32(acc, g)
            assert ((acc != 0) & (np.abs(acc) < tiny)).any() and ((g != 0) & (np.abs(g) < tiny)).any()
            assert ((s != 0) & (np.abs(s) < tiny)).any()
            assert (np.signbit(g) & (g == 0)).any() and (np.signbit(acc) & (acc == 0)).any()
            assert ((g == -acc) & (acc != 0)).any()
            assert np.isposinf(s).any() and np.isneginf(s).any()
            assert (np.isposinf(s) & np.isfinite(acc) & np.isfinite(g)).any()              # overflow
            assert ((s == acc) & (g != 0) & np.isfinite(acc)).any()                        # an addend rounded away
            assert (np.signbit(accum_ref.store(g)) & ~np.signbit(s) & (s == 0)).any()      # store keeps -0, add gives +0


ABI = ("p3d_set_grad_accum", "p3d_get_grad_accum", "p3d_debug_grad_accum")


def test_boundary():
    from sap3d_tensorflow_amd import _lib, ops
    from sap3d_tensorflow_amd.session import P3DSession
    header = open(os.path.join(ROOT, "include", "p3d_hip.h")).read()
    for name in ABI:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert "SUMMED, not averaged" in header
    assert callable(P3DSession.set_grad_accum) and isinstance(P3DSession.grad_accum, property)
    assert callable(ops.grad_accum) and ops.GRAD_ACCUM_MODES == accum_ref.MODES


def test_train_help_lists_the_flag():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "drivers", "train.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--accum-steps" in r.stdout
