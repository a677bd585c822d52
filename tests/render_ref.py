"""numpy replay of include/p3d_hip.h's "Rendering 8-bit maps" (p3d_render_u8, p3d_video_render; csrc/render.hip), written with
shifted arrays: the blend through a table of colour and opacity, the plain heat map, and the contour of a level set.  Everything is
integer arithmetic; every comparison against it is exact."""
import numpy as np


def unpack(table):
    """uint32 [256] -> (colour int64 [256, 3] in B, G, R order, opacity int64 [256])."""
    t = np.asarray(table, dtype=np.uint32).astype(np.int64)
    return np.stack([t & 255, (t >> 8) & 255, (t >> 16) & 255], axis=-1), (t >> 24) & 255


def pack(b, g, r, o):
    return (np.asarray(b, np.uint32) | (np.asarray(g, np.uint32) << 8) | (np.asarray(r, np.uint32) << 16) | (np.asarray(o, np.uint32) << 24)).astype(np.uint32)


def blend(frame, colour, o):
    """BLEND on int64 arrays that broadcast: (frame (255 - o) + colour o + 127) // 255."""
    return (frame * (255 - o) + colour * o + 127) // 255


def contour_mask(s, L, t):
    """bool [.., H, W]: a = (s >= L) holds and some pixel inside the map within t in both directions has a false.  The pixels
    outside the map are padded as true, so they never count."""
    a = np.asarray(s) >= L
    H, W = a.shape[-2:]
    pad = [(0, 0)] * (a.ndim - 2) + [(t, t), (t, t)]
    p = np.pad(a, pad, constant_values=True)
    every = np.ones_like(a)
    for dy in range(2 * t + 1):
        for dx in range(2 * t + 1):
            every &= p[..., dy:dy + H, dx:dx + W]
    return a & ~every


def render(sal, frames, table, contour=0, thickness=1, contour_bgr=(255, 255, 255)):
    """sal uint8 [n, H, W] (or [H, W]), frames uint8 [.., H, W, 3] in B, G, R order or None -> uint8 [.., H, W, 3]."""
    s = np.asarray(sal)
    colour, o = unpack(table)
    c = colour[s]                                          # [.., H, W, 3]
    if frames is None:
        out = c
    else:
        out = blend(np.asarray(frames).astype(np.int64), c, o[s][..., None])
    out = out.astype(np.uint8)
    if contour:
        out[contour_mask(s, contour, thickness)] = np.asarray(contour_bgr, np.uint8)
    return out


# ---- the inputs of the GPU tests: a Gaussian blob plus noise (ragged level sets), random frames, three tables ----
def blob(n, H, W, seed=0):
    rng = np.random.default_rng([seed, n, H, W])
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n, H, W), np.uint8)
    for i in range(n):
        cy, cx = rng.uniform(0.3, 0.7) * (H - 1), rng.uniform(0.3, 0.7) * (W - 1)
        sy, sx = max(H * rng.uniform(0.2, 0.35), 0.8), max(W * rng.uniform(0.2, 0.35), 0.8)
        g = 235. * np.exp(-0.5 * (((yy - cy) / sy) ** 2 + ((xx - cx) / sx) ** 2)) + rng.normal(0., 14., (H, W))
        out[i] = np.clip(np.rint(g), 0, 255).astype(np.uint8)
    return out


def frames_for(sal, seed=1):
    return np.random.default_rng([seed] + list(sal.shape)).integers(0, 256, sal.shape + (3,), dtype=np.uint8)


def tables(seed=2):
    """dict: a random table, an opaque one (o = 255) and a transparent one (o = 0), random colours each."""
    rng = np.random.default_rng(seed)
    rnd = rng.integers(0, 2 ** 32, 256, dtype=np.uint64).astype(np.uint32)
    return dict(random=rnd, opaque=rnd | np.uint32(0xff000000), transparent=rnd & np.uint32(0x00ffffff))
