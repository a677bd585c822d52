"""Numpy replay of the fixation pool and shuffled AUC's sampling (include/p3d_hip.h, "Shuffled AUC in the evaluation pass"): STORE,
UNION and SELECT as the header states them.  tests/test_sauc_device_cpu.py holds the replay to oracle.evaluation.AUC_shuffled;
tests/test_gpu_sauc_device.py holds the kernels to the replay with tolerance 0."""
import numpy as np

SCAN_BLOCK = 256          # P3D_FIX_SCAN_BLOCK: words per block of the union's scan


def n_words(n_pix):
    return (int(n_pix) + 63) // 64


def pack(maps):
    """STORE: uint8 [n, H, W] -> uint64 [n, ceil(H W / 64)]; bit j of word k <=> byte 64 k + j >= 128; the high bits of the last
    word are 0."""
    m = np.asarray(maps)
    m = m[None] if m.ndim == 2 else m
    n = m.shape[0]
    flat = m.reshape(n, -1) >= 128
    nw = n_words(flat.shape[1])
    out = np.zeros((n, nw * 8), np.uint8)
    for i in range(n):
        b = np.packbits(flat[i], bitorder="little")
        out[i, :len(b)] = b
    return out.view("<u8").astype(np.uint64).reshape(n, nw)


def unpack(words, n_pix):
    """The boolean pixels [n, n_pix] of packed words [n, nw]."""
    w = np.ascontiguousarray(np.asarray(words, np.uint64).astype("<u8"))
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :n_pix].astype(bool)


def other_maps(pool, others):
    """UNION as np.any: pool uint8 [capacity, H, W], others int [B, M] -> bool [B, H, W]."""
    pool = np.asarray(pool)
    return np.stack([np.any(pool[np.asarray(row)] >= 128, axis=0) for row in np.asarray(others)])


def union(pool, others):
    """-> (uni uint64 [B, nw], the exclusive prefix of the words' bit counts uint32 [B, nw], n_other uint32 [B])."""
    other = other_maps(pool, others)
    B = other.shape[0]
    uni = pack(other.astype(np.uint8) * 255)
    counts = unpack(uni, uni.shape[1] * 64).reshape(B, -1, 64).sum(axis=2).astype(np.uint32)
    prefix = (np.cumsum(counts, axis=1, dtype=np.uint32) - counts).astype(np.uint32)
    return uni, prefix, counts.sum(axis=1).astype(np.uint32)


def select(other, ranks):
    """SELECT: np.nonzero(other.ravel())[0][ranks]."""
    return np.nonzero(np.asarray(other).ravel())[0][np.asarray(ranks, dtype=np.int64)]


def replay_idx(pool, others, ranks, n_rows, n_rep):
    """The pixel indices of every clip's ranks (metrics.shuffled_draws' layout) -> a list of int arrays [n_rows[b], n_rep]."""
    other = other_maps(pool, others)
    out, at = [], 0
    for b in range(other.shape[0]):
        n = int(n_rows[b]) * n_rep
        out.append(select(other[b], ranks[at:at + n]).reshape(int(n_rows[b]), n_rep))
        at += n
    return out
