"""Float64 statement and float32 replay of the Momentum and SGD optimisers (P3DSession.set_optimizer), and TF's beta powers.

TensorFlow's kernels (training_ops.cc ApplyMomentum, ApplyGradientDescent):
  * Momentum:  accum = accum * momentum + grad;  var -= accum * lr
  * Nesterov:  accum = accum * momentum + grad;  var -= grad * lr + accum * momentum * lr   (the updated accum)
  * SGD:       var -= lr * grad
The library's kernels (elementwise.hip opt_elem) round every product and sum on its own, with no fused multiply-add; the
replays below make the same roundings in numpy float32, so the kernels must match them bit for bit.

tf.train.AdamOptimizer keeps beta1_power and beta2_power as float32 variables that start at beta and are multiplied by beta
after every step: after t completed steps they hold beta^(t+1), with the drift of a running float32 product."""
import numpy as np

f32 = np.float32


def momentum32(p, a, g, lr, momentum, nesterov=False):
    """-> (p, accum) after one step, every operation rounded to float32."""
    p, a, g = (np.asarray(t, f32).copy() for t in (p, a, g))
    lr, mom = f32(lr), f32(momentum)
    a = (a * mom + g).astype(f32)
    if nesterov:
        p = (p - (g * lr + (a * mom) * lr)).astype(f32)
    else:
        p = (p - lr * a).astype(f32)
    return p, a


def sgd32(p, g, lr):
    p, g = np.asarray(p, f32), np.asarray(g, f32)
    return (p - f32(lr) * g).astype(f32)


def momentum64(p, a, g, lr, momentum, nesterov=False):
    """TF's formulas in float64 (lr and momentum as the float32 values the kernels take)."""
    p, a, g = (np.asarray(t, np.float64) for t in (p, a, g))
    lr, mom = float(f32(lr)), float(f32(momentum))
    a = a * mom + g
    p = p - (g * lr + a * mom * lr) if nesterov else p - lr * a
    return p, a


def sgd64(p, g, lr):
    return np.asarray(p, np.float64) - float(f32(lr)) * np.asarray(g, np.float64)


def update32(kind, p, a, g, lr, momentum=0.9, nesterov=False):
    """(p, accum) after one step of kind "momentum" | "nesterov" | "sgd" (accum unchanged by SGD)."""
    if kind == "sgd":
        return sgd32(p, g, lr), np.asarray(a, f32)
    return momentum32(p, a, g, lr, momentum, kind == "nesterov")


def update64(kind, p, a, g, lr, momentum=0.9, nesterov=False):
    if kind == "sgd":
        return sgd64(p, g, lr), np.asarray(a, np.float64)
    return momentum64(p, a, g, lr, momentum, kind == "nesterov")


def tf_running_powers(t, beta1=0.9, beta2=0.999):
    """beta1_power, beta2_power as TF holds them after t completed steps: float32 beta, times float32 beta t times."""
    b1, b2 = f32(beta1), f32(beta2)
    p1, p2 = b1, b2
    for _ in range(t):
        p1, p2 = f32(p1 * b1), f32(p2 * b2)
    return p1, p2
