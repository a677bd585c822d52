"""Synthetic clips with the value law of the reference's loader (dataflow.py:204-208, gen_pred.py:117-121):
RGB uint8 minus the channel means [90,102,98], divided by 255; targets uniform in [0,1).
Seeded with numpy's PCG64 so every box draws identical inputs."""
import numpy as np

MEAN_RGB = np.array([90, 102, 98], np.float32)


def synthetic_clip(seed, shape):
    """shape [B,T,H,W,3] float32 in about [-0.40, 0.65]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    u8 = rng.integers(0, 256, size=shape).astype(np.float32)
    return ((u8 - MEAN_RGB) / 255.0).astype(np.float32)


def synthetic_target(seed, shape):
    """shape [B,T,H,W] float32 saliency targets in [0,1)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.random(size=shape, dtype=np.float32)


def synthetic_fixations(seed, target, share=0.02):
    """Fixation maps drawn from a target [B,T,H,W]: uint8 of the same shape, 255 where a uniform draw falls under
    share * y / mean(y of the map) -- about `share` of every map, denser where the target is higher -- and at the map's
    maximum, so that no map is empty."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y = np.asarray(target, np.float32)
    flat = y.reshape(y.shape[0], y.shape[1], -1)
    mean = np.maximum(flat.mean(axis=2, keepdims=True), np.float32(1e-12))
    f = rng.random(size=flat.shape, dtype=np.float32) < np.float32(share) * flat / mean
    np.put_along_axis(f, flat.argmax(axis=2)[..., None], True, axis=2)
    return (f.reshape(y.shape) * np.uint8(255)).astype(np.uint8)


def synthetic_test_set(seed, n, size=(1080, 960), density_size=(270, 480), frames=16, crop=112):
    """An evaluation set for drivers/test.py: x [n,frames,crop,crop,3] float32 by the synthetic_clip law; density uint8
    [n, Hd, Wd] uniform bytes; fixation uint8 [n, H, W]: clip i gets 255 at k ~ U{50..999} uniform pixel draws (with
    replacement), except every third clip (i % 3 == 2), which stays empty (the reference's metrics give NaN there)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = synthetic_clip(seed, (n, frames, crop, crop, 3))
    density = rng.integers(0, 256, size=(n,) + tuple(density_size), dtype=np.uint8)
    fixation = np.zeros((n,) + tuple(size), np.uint8)
    for i in range(n):
        k = int(rng.integers(50, 1000))
        pix = rng.integers(0, size[0] * size[1], size=k)
        if i % 3 != 2:
            fixation[i].reshape(-1)[pix] = 255
    return x, density, fixation
