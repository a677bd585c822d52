"""The yardstick of the decision-pinned gradient tests (tests/test_gpu_pinned.py), on the CPU alone.

A pinned comparison differentiates the float64 oracle on the ReLU masks and max-pool choices of ANOTHER evaluation of the same
graph (oracle/nn.py Tape.pins), so that what is left between the two is summation order and rounding.  How large that may be is
not a constant: it is what a float32 evaluation of the same oracle, on the same pins, leaves against float64 -- tensor by
tensor.  This file holds the three pieces of that:

 * recording(): takes the decisions of one oracle evaluation in the form P3DSession.decisions() returns them, so that the rule
   can be tried on the reference alone (tests/test_pinned_yardstick_cpu.py);
 * errors(): the per-tensor rel-L2 of the pinned tests;
 * the rule: with e32[n] the float32 oracle's error on the same pins and m the median of e32,
       bound[n] = min(FACTOR * max(e32[n], m), flat).
   FACTOR = 5 is the factor of every noise bound of this suite (gates.noise_excess, attention_ref.rule, test_gpu_full.py); the
   floor m keeps a tensor that numpy happens to get almost exactly (e32 of a few 1e-7) from asking the same of another order of
   summation; it is computed from the reference when the test runs.  `flat` is the bound the pinned tests had before the rule
   (PLAIN): the rule can only ask more than that, never less.
"""
import contextlib

import numpy as np

from oracle import nn

PLAIN = 2e-3          # the flat bound of the pinned tests (the absolute part of the fp32-noise bound of the gradient tests)
FACTOR = 5.0


# ---- decisions of an oracle evaluation ----------------------------------------------------------------------------------------
@contextlib.contextmanager
def recording(pool_tol=1e-3):
    """While active, every oracle.nn.relu on a tagged value (the output of a normalisation layer, or a sum gated under its name)
    and every oracle.nn.max_pool3d leaves its decision in the dict this yields: {'relu': {tag: bool array}, 'pool': [the pools'
    inputs], 'relu_sites': count, 'pool_tol': pool_tol} -- what P3DSession.decisions() gives for a HIP pass.  A pinned relu
    records the mask it was given."""
    pins = {"relu": {}, "pool": [], "relu_sites": 0, "pool_tol": pool_tol}
    relu0, pool0 = nn.relu, nn.max_pool3d

    def relu(tape, x):
        if x.tag is not None:
            assert x.tag not in pins["relu"], "two ReLUs under the tag %r" % x.tag
            pin = None if tape.pins is None else tape.pins.get("relu", {}).get(x.tag)
            pins["relu"][x.tag] = x.data > 0 if pin is None else np.asarray(pin).reshape(x.data.shape).astype(bool)
            pins["relu_sites"] += 1
        return relu0(tape, x)

    def max_pool3d(tape, x, ksize, strides):
        pins["pool"].append(x.data.astype(np.float32))
        return pool0(tape, x, ksize, strides)

    nn.relu, nn.max_pool3d = relu, max_pool3d
    try:
        yield pins
    finally:
        nn.relu, nn.max_pool3d = relu0, pool0


def flipped(pins):
    """The same decisions for the batch in reverse order."""
    out = dict(pins)
    out["relu"] = {k: v[::-1] for k, v in pins["relu"].items()}
    out["pool"] = [p[::-1] for p in pins["pool"]]
    return out


@contextlib.contextmanager
def reversed_k():
    """A second float32 order of the oracle: every conv sums its input channels (forward, filter gradient: its rows of one tap
    keep their order) and its output channels (input gradient) from the last to the first.  Same function, other rounding."""
    fwd0, bwi0 = nn.conv3d_forward, nn.conv3d_backward_input

    def conv3d_forward(x, w, strides):
        return fwd0(x[..., ::-1], w[:, :, :, ::-1, :], strides)

    def conv3d_backward_input(dy, w, strides, xshape):
        return bwi0(dy[..., ::-1], w[..., ::-1], strides, xshape)

    nn.conv3d_forward, nn.conv3d_backward_input = conv3d_forward, conv3d_backward_input
    try:
        yield
    finally:
        nn.conv3d_forward, nn.conv3d_backward_input = fwd0, bwi0


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def errors(g, g64):
    """Per-tensor rel-L2 of the gradients `g` (a mapping, or a function of the name: P3DSession.get_grad) against the float64
    ones, relative to the larger of the tensor's norm and 1e-2 of the median norm.  Returns (errors, names of the tensors under
    that floor): e.g. conv biases in front of a batch-statistics BatchNorm have a gradient of exactly zero."""
    get = g if callable(g) else g.__getitem__
    floor = 1e-2 * np.median([np.linalg.norm(v) for v in g64.values()])
    errs = {n: float(np.linalg.norm(np.asarray(get(n)).astype(np.float64) - w) / max(np.linalg.norm(w), floor)) for n, w in g64.items()}
    return errs, sorted(n for n, w in g64.items() if np.linalg.norm(w) < floor)


# ---- the rule -------------------------------------------------------------------------------------------------------------------
def yardstick(e32):
    """max(e32[n], median e32) per tensor: what FACTOR multiplies."""
    m = float(np.median(list(e32.values())))
    return {n: max(float(e), m) for n, e in e32.items()}


def bounds(e32, flat=PLAIN):
    return {n: min(FACTOR * y, flat) for n, y in yardstick(e32).items()}


def ratios(e, e32):
    """e[n] / max(e32[n], median e32): the rule asks <= FACTOR."""
    y = yardstick(e32)
    return {n: e[n] / y[n] for n in e32}


def failures(e, e32, flat=PLAIN):
    """[(error, bound, name)] of the tensors above their bound, worst ratio first."""
    b = bounds(e32, flat)
    return sorted(((e[n], b[n], n) for n in e32 if not e[n] <= b[n]), key=lambda t: -t[0] / t[1])


def table(e, e32, top=5):
    """The `top` largest ratios with their tensors, for the printed lines."""
    y = yardstick(e32)
    worst = sorted(((e[n] / y[n], n) for n in e32), reverse=True)[:top]
    return ", ".join("%.2f %s (%.1e / %.1e)" % (r, n, e[n], e32[n]) for r, n in worst)
