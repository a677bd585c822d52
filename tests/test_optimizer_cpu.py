"""No-GPU checks of the Momentum / SGD optimiser option and of the optimiser state in checkpoints: the float32 replays in
opt_ref.py against TF's formulas in float64, the beta-power <-> step round trip, the header and the slot names."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import opt_ref              # noqa: E402

ROOT = os.path.dirname(HERE)
U32 = np.finfo(np.float32).eps / 2          # unit roundoff of float32


@pytest.mark.parametrize("kind", ["momentum", "nesterov", "sgd"])
@pytest.mark.parametrize("lr,momentum", [(1e-4, 0.9), (3e-2, 0.99), (1.0, 0.0)])
def test_replays_match_float64_to_float32_rounding(kind, lr, momentum):
    rng = np.random.default_rng(7)
    n = 100_000
    p = rng.standard_normal(n).astype(np.float32)
    a = (rng.standard_normal(n) * 0.1).astype(np.float32)
    g = (rng.standard_normal(n) * 0.1).astype(np.float32)
    p32, a32 = opt_ref.update32(kind, p, a, g, lr, momentum)
    p64, a64 = opt_ref.update64(kind, p, a, g, lr, momentum)
    lr64, m64 = float(np.float32(lr)), float(np.float32(momentum))
    a_abs, g_abs = np.abs(a.astype(np.float64)), np.abs(g.astype(np.float64))
    if kind != "sgd":
        # accum = fl(fl(a m) + g): two roundings, each at most u of its result
        bound_a = U32 * (2 * a_abs * m64 + g_abs) * (1 + U32)
        assert np.all(np.abs(a32 - a64) <= bound_a)
        step_abs = np.abs(a64) * lr64 if kind == "momentum" else (g_abs + np.abs(a64) * m64) * lr64
        step_err = lr64 * bound_a * (m64 if kind == "nesterov" else 1.0)
        bound_p = U32 * np.abs(p64) + 4 * U32 * step_abs + step_err + U32 * (np.abs(p) + step_abs)
    else:
        assert np.array_equal(a32, a)
        bound_p = U32 * np.abs(p64) + 2 * U32 * lr64 * g_abs + U32 * np.abs(p)
    assert p32.dtype == np.float32 and np.all(np.abs(p32 - p64) <= bound_p * (1 + 8 * U32))


def test_sgd_and_momentum_zero_agree():
    """Momentum 0 and no history is plain gradient descent with one extra rounding-free add (0 * a + g == g)."""
    rng = np.random.default_rng(3)
    p, g = rng.standard_normal(1000).astype(np.float32), rng.standard_normal(1000).astype(np.float32)
    pm, am = opt_ref.momentum32(p, np.zeros_like(p), g, 1e-2, 0.0)
    assert np.array_equal(pm, opt_ref.sgd32(p, g, 1e-2)) and np.array_equal(am, g)


def test_beta_powers_round_trip_to_5000():
    from sap3d_tensorflow_amd.session import adam_step_from_powers
    b1, b2 = np.float32(0.9), np.float32(0.999)
    p1, p2 = b1, b2                                   # TF's running float32 product
    for t in range(5001):
        assert adam_step_from_powers(p1, p2) == t
        exact = [np.float32(np.float64(b) ** (t + 1)) for b in (b1, b2)]      # what optimizer_state() writes
        assert adam_step_from_powers(*exact) == t
        p1, p2 = np.float32(p1 * b1), np.float32(p2 * b2)
    assert opt_ref.tf_running_powers(5001) == (p1, p2)       # the helper makes the same product
    # other betas: the step comes from beta2_power, beta1_power must fit it
    for t in (0, 1, 17, 999, 2500):
        q1, q2 = opt_ref.tf_running_powers(t, 0.5, 0.99)
        assert adam_step_from_powers(q1, q2, 0.5, 0.99) == t


def test_beta_powers_that_fit_no_step_are_refused():
    from sap3d_tensorflow_amd.session import adam_step_from_powers
    p1, p2 = opt_ref.tf_running_powers(100)
    with pytest.raises(ValueError):
        adam_step_from_powers(np.float32(p1 * 1.01), p2)              # beta1_power of another step
    with pytest.raises(ValueError):
        adam_step_from_powers(p1, np.float32(1.5))                    # above 1
    with pytest.raises(ValueError):
        adam_step_from_powers(p1, np.float32(0.0))
    with pytest.raises(ValueError):
        adam_step_from_powers(np.float32(0.95), np.float32(0.9995))     # beta2_power above beta2: no step
    # a beta1_power drifted by a running product stays accepted (relative 1e-3)
    assert adam_step_from_powers(np.float32(p1 * (1 + 5e-4)), p2) == 100


def test_header_declares_the_optimizer_interface():
    src = open(os.path.join(ROOT, "include", "p3d_hip.h")).read()
    assert re.search(r"enum\s*\{\s*P3D_OPT_ADAM\s*=\s*0\s*,\s*P3D_OPT_MOMENTUM\s*=\s*1\s*,\s*P3D_OPT_SGD\s*=\s*2\s*\}", src)
    for decl in (r"int p3d_set_optimizer\(p3d_handle\* h, int kind, float lr, float momentum, int use_nesterov\);",
                 r"int p3d_get_slot\(p3d_handle\* h, const char\* var, int slot, float\* host, int64_t count\);",
                 r"int p3d_set_slot\(p3d_handle\* h, const char\* var, int slot, const float\* host, int64_t count\);",
                 r"int p3d_get_optimizer_step\(p3d_handle\* h, int64_t\* t\);",
                 r"int p3d_set_optimizer_step\(p3d_handle\* h, int64_t t\);",
                 r"int p3d_debug_optimizer\(int device, int kind,",
                 r"int p3d_debug_optimizer_decay\(int device, int kind,"):
        assert re.search(decl, src), decl
    from sap3d_tensorflow_amd import _lib
    assert _lib.OPTIMIZERS == {"adam": 0, "momentum": 1, "sgd": 2}
    for n in ("p3d_set_optimizer", "p3d_get_slot", "p3d_set_slot", "p3d_get_optimizer_step", "p3d_set_optimizer_step",
              "p3d_debug_optimizer", "p3d_debug_optimizer_decay"):
        assert n in _lib.SIGNATURES, n


STRUCTURES = ("unet", "concat", "unet++nonsa", "unet++ds", "gn_p3d", "gn_p3d_concat", "gn_p3d_decoder")


@pytest.mark.parametrize("structure", STRUCTURES)
def test_slot_names_map_onto_the_variable_list(structure):
    from oracle import p3d, p3d_gn
    from sap3d_tensorflow_amd.session import slot_names
    cfg = p3d.NetConfig(base=16, blocks=(1, 2, 2))
    heads = {"gn_p3d": "p3d", "gn_p3d_concat": "concat", "gn_p3d_decoder": "decoder"}
    if structure in heads:
        params = p3d_gn.init_params(1, cfg, head=heads[structure])
    else:
        params = p3d.init_params(1, structure, cfg)
    variables = [(n, v.shape, not n.endswith(("/moving_mean", "/moving_variance"))) for n, v in params.items()]
    trainables = [n for n, _, tr in variables if tr]
    assert trainables
    adam, mom, sgd = (slot_names(variables, k) for k in ("adam", "momentum", "sgd"))
    assert sgd == {}
    assert sorted(adam) == sorted([n + "/Adam" for n in trainables] + [n + "/Adam_1" for n in trainables])
    assert sorted(mom) == sorted(n + "/Momentum" for n in trainables)
    assert all(adam[n + "/Adam"] == (n, 0) and adam[n + "/Adam_1"] == (n, 1) and mom[n + "/Momentum"] == (n, 0)
               for n in trainables)
    # no slot name collides with a variable, or with the Adam powers a default Saver writes beside them
    names = set(params) | {"beta1_power", "beta2_power"}
    assert not (set(adam) | set(mom)) & names
