"""numpy replay of gradient accumulation over micro-batches (P3DSession.set_grad_accum), bit for bit what grad_accum_kernel
computes in float32.  No TensorFlow is involved: include/p3d_hip.h is the contract, and this file replays it.

    micro-step 0            acc = g0                      a copy of the bits: -0 stays -0
    micro-steps 1 .. K-2    acc = fadd(acc, g_j)          rounded once to float32
    micro-step  K-1         g   = fadd(acc, g_{K-1})      the same add, written to the gradient buffer

so the applied gradient is ((g0 + g1) + g2) + ... per element, in that order, a SUM and not a mean.  float32 adds keep
denormals (nothing is flushed), x + (-x) = +0, and -0 + +0 = +0 under round-to-nearest."""
import numpy as np

f32 = np.float32
MODES = {"store": 0, "add": 1, "finish": 2}


def store(g):
    """acc = g: the bits of g."""
    return np.array(g, f32, copy=True)


def add32(acc, g):
    """fadd(acc, g) per element, rounded once."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(acc, f32) + np.asarray(g, f32)).astype(f32)


def finish(acc, g):
    """The applying micro-step's gradient: the same add as add32."""
    return add32(acc, g)


def launch(mode, acc, g):
    """What one launch leaves in the operand it writes (acc under store / add, g under finish)."""
    return store(g) if mode in ("store", 0) else add32(acc, g)


def cycle(grads):
    """The gradient applied after the micro-batch gradients `grads` (a list, K >= 1), in the library's order."""
    acc = store(grads[0])
    for g in grads[1:]:
        acc = add32(acc, g)
    return acc


def special_inputs(n, seed):
    """(acc, g) of n elements for the op-level test: random normals with -0.0, denormals, exact cancellation (g = -acc), +-inf
    (never inf + -inf: no NaN is produced or compared) and large / small pairs whose sum rounds the small one away."""
    rng = np.random.default_rng(seed)
    acc = rng.standard_normal(n).astype(f32)
    g = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(f32)
    k = np.arange(n)
    acc[k % 7 == 1] = f32(3e-41)                         # denormal accumulator, normal gradient
    g[k % 11 == 2] = f32(-7e-42)                         # denormal gradient
    both = k % 13 == 3
    acc[both] = f32(3e-41); g[both] = f32(5e-42)         # denormal + denormal = denormal, exactly
    cancel = k % 5 == 4
    g[cancel] = -acc[cancel]                             # x + (-x) = +0
    acc[k % 17 == 5] = f32(-0.0)
    g[k % 19 == 6] = f32(-0.0)
    nz = k % 23 == 7
    acc[nz] = f32(0.0); g[nz] = f32(-0.0)                # +0 + -0 = +0, while a store of -0 keeps -0
    nn = k % 29 == 8
    acc[nn] = f32(-0.0); g[nn] = f32(-0.0)               # -0 + -0 = -0
    pinf = k % 31 == 9
    acc[pinf] = f32(np.inf); g[pinf] = f32(1.0)
    ninf = k % 37 == 10
    acc[ninf] = f32(-2.5); g[ninf] = f32(-np.inf)
    big = k % 41 == 11
    acc[big] = f32(3e38); g[big] = f32(3e38)             # overflow to +inf
    lost = k % 43 == 12
    acc[lost] = f32(1e8); g[lost] = f32(1.0)             # the small addend is rounded away
    half = k % 47 == 13
    acc[half] = f32(1.0); g[half] = f32(2.0 ** -24)      # a tie: rounds to even, stays 1.0
    return acc, g
