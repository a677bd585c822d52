"""The dropout mask, replayed on the CPU (include/p3d_hip.h at p3d_forward states it; three kernels files carry a copy each:
csrc/elementwise.hip, gn.hip, attention.hip).

    z = seed + 0x9E3779B97F4A7C15 * (e + 1)                       uint64, wrapping
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
    z = (z ^ (z >> 27)) * 0x94D049BB133111EB
    z = z ^ (z >> 31)                                             (the SplitMix64 finaliser)
    u01(seed, e) = float32(z >> 40) * 2^-24
    keep(e) = u01(seed, e) >= float32(rate)

e = row * C + c is the DENSE index of an element of a [rows, C] activation, whatever row stride its buffer has.  Independent
of oracle/ and of the library: numpy uint64 arithmetic only."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
MUL1 = np.uint64(0xBF58476D1CE4E5B9)
MUL2 = np.uint64(0x94D049BB133111EB)


def u01(seed, idx):
    """float32 uniform in [0, 1) of (seed, element index); idx a non-negative integer or an array of them."""
    with np.errstate(over="ignore"):
        e = np.asarray(idx, dtype=np.uint64)
        z = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) + GOLDEN * (e + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * MUL1
        z = (z ^ (z >> np.uint64(27))) * MUL2
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)      # (24 bits: exact in float32)


def keep(seed, rate, rows, C):
    """bool [rows, C]: True where the element of dense index row * C + c is kept."""
    e = np.arange(int(rows) * int(C), dtype=np.uint64)
    return (u01(seed, e) >= np.float32(rate)).reshape(int(rows), int(C))


def scale(rate):
    """What a kept element is multiplied by: 1 / (1 - rate), formed in float32 (set_dropout, net.hip)."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(rate))
