"""Float32 replay and float64 statement of the moving average of the weights (P3DSession.set_ema), the contract of
include/p3d_hip.h:

  s = s - (s - p) * om          float32, every operation rounded on its own (TF's assign_moving_average)
  constant decay   om = float32(1.0 - decay), the subtraction in double
  warm-up          t = float32(steps); q = (1 + t) / (10 + t); d = min(float32(decay), q); om = 1 - d, all in float32
steps counts the completed optimiser steps including the current one.  No TensorFlow pins this: the text is the contract."""
import numpy as np

f32 = np.float32
SUFFIX = "ExponentialMovingAverage"


def om_const(decay):
    return f32(1.0 - float(decay))


def decay_warmup(decay, steps):
    """d_t of step `steps` (1-based) in float32."""
    t = f32(steps)
    q = f32(f32(f32(1.0) + t) / f32(f32(10.0) + t))
    return min(f32(decay), q)


def om_warmup(decay, steps):
    return f32(f32(1.0) - decay_warmup(decay, steps))


def om(decay, warmup=False, steps=None):
    return om_warmup(decay, steps) if warmup else om_const(decay)


def update32(s, p, om_):
    """The kernel's arithmetic: numpy float32 arrays round every operation once and fuse nothing."""
    s, p = np.asarray(s, f32), np.asarray(p, f32)
    d = (s - p).astype(f32)
    e = (d * f32(om_)).astype(f32)
    return (s - e).astype(f32)


def update64(s, p, decay):
    s, p = np.asarray(s, np.float64), np.asarray(p, np.float64)
    return s - (s - p) * (1.0 - float(decay))


def shadow_name(var):
    return "%s/%s" % (var, SUFFIX)
