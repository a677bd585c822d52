"""Float64 statement and float32 replay of gradient clipping by the global norm (P3DSession.set_grad_clip).

  sumsq = sum g^2      every square of a float32 value is exact in float64 (48 bits); math.fsum adds them without error
  norm  = sqrt(sumsq)
  scale = float32(clip / max(norm, clip))     exactly 1 while norm <= clip; 1 under clip = inf; NaN for a norm that is not finite
  g''   = float32(g * scale)                  one rounding, and the optimiser's own arithmetic after it
clip is the float32 value the library takes."""
import math

import numpy as np

f32 = np.float32


def sumsq64(g):
    g = np.asarray(g, np.float32).ravel().astype(np.float64)
    return math.fsum((g * g).tolist())


def scale32(norm, clip):
    clip = float(f32(clip))
    if not math.isfinite(norm):
        return f32(np.nan)
    if math.isinf(clip):
        return f32(1.0)
    return f32(clip / max(float(norm), clip))


def scaled32(g, scale):
    return (np.asarray(g, f32) * f32(scale)).astype(f32)


def ulps64(a, b):
    return abs(float(a) - float(b)) / np.spacing(abs(float(b)))


def ulps32(a, b):
    return abs(float(f32(a)) - float(f32(b))) / float(np.spacing(abs(f32(b))))
