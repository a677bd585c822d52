"""Float64 expected results for the conv launches in the forms the train step uses (tests/test_gpu_conv_launch.py): operands
that are channel slices of wider rows, results added to what the output holds, the residue classes of a strided conv's input
gradient that no filter tap reaches, and the fp16 option of the 1x1x1 convs.

Everything is built from oracle.nn in float64.  The fp16 reference rounds both operands with astype(np.float16) -- round to
nearest even, what the kernel's (_Float16)v does -- and then runs the float64 conv: the product of two fp16 values is exact in
float32 (11 x 11 significant bits), so against THIS reference the fp16 mode carries only its float32 accumulation error."""
import numpy as np

from oracle import nn

f64 = np.float64


def embed(a, ld, offset, fill):
    """[..., C] -> [rows, ld] float32 with `a` in columns offset .. offset + C and `fill` everywhere else."""
    a = np.asarray(a, np.float32)
    a = a.reshape(-1, a.shape[-1])
    out = np.full((a.shape[0], ld), fill, np.float32)
    out[:, offset:offset + a.shape[1]] = a
    return out


def outside(buf, C, offset):
    """The columns of [rows, ld] `buf` outside the slice offset .. offset + C: left of it, then right of it."""
    return np.concatenate([buf[:, :offset], buf[:, offset + C:]], axis=1)


def nan_fill(payload=0x5A5A5):
    """A quiet float32 NaN with a recognisable payload: a kernel that writes 'a NaN' of its own does not reproduce its bits."""
    return np.array([0x7FC00000 | (payload & 0x3FFFFF)], np.uint32).view(np.float32)[0]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def round16(a):
    """What the fp16 option does to an operand: round to nearest even to fp16 (values are exact in float64 after)."""
    return np.asarray(a, np.float32).astype(np.float16).astype(f64)


def draw16(rng, shape, scale=1.0):
    """Operands for the fp16 cases: magnitudes in [2^-6, 4] * scale with random signs, so that no operand is an fp16 subnormal
    (with scale >= 2^-8: the smallest normal fp16 is 2^-14) and every one carries a rounding error of up to 2^-11 relative."""
    mag = np.exp2(rng.uniform(-6.0, 2.0, shape))
    return (mag * rng.choice([-1.0, 1.0], shape) * scale).astype(np.float32)


# ---- the three conv kinds in float64 --------------------------------------------------------------------------------------------
def forward(x, w, s, bias=None, f16=False):
    x, w = (round16(x), round16(w)) if f16 else (np.asarray(x, f64), np.asarray(w, f64))
    y = nn.conv3d_forward(x, w, s)
    return y + np.asarray(bias, f64) if bias is not None else y


def input_grad(dy, w, s, xshape, f16=False):
    dy, w = (round16(dy), round16(w)) if f16 else (np.asarray(dy, f64), np.asarray(w, f64))
    return nn.conv3d_backward_input(dy, w, s, tuple(xshape))


def filter_grad(x, dy, wshape, s):
    return nn.conv3d_backward_filter(np.asarray(x, f64), np.asarray(dy, f64), tuple(wshape), s)


def transpose(x, kernel, s, bias=None):
    """tf.layers.conv3d_transpose 'same', kernel [kd,kh,kw,Cout,Cin]."""
    t = nn.Tape()
    b = nn.Var(np.asarray(bias, f64)) if bias is not None else None
    return nn.conv3d_transpose(t, nn.Var(np.asarray(x, f64)), nn.Var(np.asarray(kernel, f64)), s, b).data


def transpose_filter_grad(x, dy, kshape, s):
    """Gradient of transpose() with respect to its kernel: the filter gradient of the conv whose input is the output."""
    return nn.conv3d_backward_filter(np.asarray(dy, f64), np.asarray(x, f64), tuple(kshape), s)


def transpose_input_grad(dy, kernel, s):
    return nn.conv3d_forward(np.asarray(dy, f64), np.asarray(kernel, f64), s)


# ---- residue classes without a tap ----------------------------------------------------------------------------------------------
def empty_mask(xshape, k, s):
    """[D, H, W] bool: the positions of a SAME conv's input that no (tap, output position) pair reads -- where the input gradient
    is zero whatever dy is, and where a transposed conv's output is exactly its bias.  Along each axis position i is read iff some
    tap a in [0, k) has (i + pad - a) % s == 0 with the output index (i + pad - a) / s in [0, O)."""
    axes = []
    for ax in range(3):
        I = int(xshape[1 + ax])
        O, pb, _ = nn.same_pads(I, k[ax], s[ax])
        hit = np.zeros(I, bool)
        for i in range(I):
            for a in range(k[ax]):
                q = i + pb - a
                if q % s[ax] == 0 and 0 <= q // s[ax] < O:
                    hit[i] = True
        axes.append(hit)
    reached = axes[0][:, None, None] & axes[1][None, :, None] & axes[2][None, None, :]
    return ~reached


def accumulated(prior, result):
    """What an accumulating launch must leave: prior + result in float64."""
    return np.asarray(prior, f64) + np.asarray(result, f64)


def f32_distance(fn32, want):
    """Relative distance (of max |want|) of a float32 evaluation of the same case from the float64 one: the yardstick for a case
    that cannot keep the default tolerance (the bound is then 4 x this, written in the case's comment)."""
    return np.abs(np.asarray(fn32, f64) - want).max() / max(np.abs(want).max(), 1e-30)
