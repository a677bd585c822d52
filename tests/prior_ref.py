"""numpy replay of the fixation priors of include/p3d_hip.h (p3d_prior_*, p3d_set_prior_stage; csrc/prior.hip), bit for bit: the
counts in plain integer arithmetic, the finish through tests/postprocess_ref.py (float32 counts, BLUR, NORM max), the two apply
laws in float32 with every product and sum a numpy operation of its own, hence rounded once."""
import numpy as np

import postprocess_ref as pref

KINDS = ("fixations", "bytes")
MODES = ("mul", "mix")
MAX_MAPS = 16000000
EDGE_BYTES = np.array([0, 1, 127, 128, 255], np.uint8)      # either side of the "fixated" rule, and the extremes


def edge_maps(rng, n, H, W):
    """uint8 [n, H, W] drawn from EDGE_BYTES."""
    return EDGE_BYTES[rng.integers(0, len(EDGE_BYTES), size=(n, H, W))]


def tally(maps, kind):
    """What every map adds per pixel, int64 [n, H, W]: 1 where the byte is >= 128, or the byte."""
    m = np.asarray(maps)
    assert m.dtype == np.uint8 and m.ndim == 3
    if kind == "fixations":
        return (m >= 128).astype(np.int64)
    if kind == "bytes":
        return m.astype(np.int64)
    raise ValueError(kind)


def count(maps, kind="fixations", sign=1, counts=None):
    """COUNT -> (uint32 [H, W], underflow flag).  The words wrap modulo 2^32 as the device's do; the flag says that the true
    result went below zero somewhere."""
    assert sign in (1, -1)
    add = tally(maps, kind).sum(axis=0)
    have = np.zeros(add.shape, np.int64) if counts is None else np.asarray(counts, np.uint32).astype(np.int64)
    true = have + sign * add
    return (true % (1 << 32)).astype(np.uint32), bool((true < 0).any())


def finish(counts, taps):
    """FINISH: float32(count) (round to nearest even), BLUR with `taps` (empty: none), NORM max -> float32 [H, W]."""
    c = np.asarray(counts, np.uint32).astype(np.float32)
    return pref.normalise(pref.blur(c, taps)[None], "max")[0]


def apply(maps, prior, mode, a):
    """APPLY on float32 maps [..., H, W] with b = float32(1.0 - float64(float32(a)))."""
    v = np.asarray(maps, np.float32)
    g = np.asarray(prior, np.float32)
    a = np.float32(a)
    b = np.float32(1.0 - float(a))
    if mode == "mul":
        t = b * g
        t = t + a
        out = v * t
    elif mode == "mix":
        p, q = b * v, a * g
        out = p + q
    else:
        raise ValueError(mode)
    assert out.dtype == np.float32
    return out
