"""Numpy replay of the resident training set's contract (include/p3d_hip.h, "Resident training set"; csrc/trainset.hip): what the
stores keep and what a stage leaves in the staged buffers, bit for bit.  Test infrastructure only.

The stores of V concatenated videos (video v's frames at base[v] = F_0 + .. + F_{v-1}):
  frames     "u8": the decoded BGR bytes [sum F, H, W, 3] as put; "f32": the floats of mapf_frames
  density    the byte v of the 8-bit resize to the grid (oracle.dataflow.resize_linear_u8), y = v / 255.
  fixations  the bytes on the grid
A stage cuts clip k = frames start[k] .. start[k] + T - 1 of video[k] out of every store."""
import numpy as np


def bases(frames_per_video):
    return np.concatenate([[0], np.cumsum(np.asarray(frames_per_video, np.int64))])


def normalise_u8(bgr, mean_rgb):
    """The "u8" gather's closed form: per RGB channel c, fdiv(fsub(float32(bgr[2 - c]), mean[c]), 255), each rounded once to float32
    -- mapf's arithmetic at equal sizes, where both resize weights are 0 and adding their +-0 products changes no bit."""
    rgb = np.asarray(bgr)[..., ::-1].astype(np.float32)
    mean = np.asarray(mean_rgb, np.float32)
    return ((rgb - mean).astype(np.float32) / np.float32(255.0)).astype(np.float32)


def density_f32(byte):
    """(float)((double)v / 255.0): numpy's uint8 / 255. is float64, fed as float32 (dataflow.py:210-214)."""
    return (np.asarray(byte, np.uint8) / 255.0).astype(np.float32)


def clip_first_frames(frames_per_video, clips, T):
    """The first frame of every clip in the concatenation; a clip outside its video is a ValueError, as the stage refuses it."""
    base = bases(frames_per_video)
    out = []
    for k, (v, s) in enumerate(clips):
        if not 0 <= v < len(frames_per_video):
            raise ValueError("clip %d names video %d" % (k, v))
        if not 0 <= s <= frames_per_video[v] - T:
            raise ValueError("clip %d starts at %d, outside [0, %d]" % (k, s, frames_per_video[v] - T))
        out.append(int(base[v]) + s)
    return out


def cut(store, frames_per_video, clips, T):
    """[B, T, ...] of a store [sum F, ...]: a copy of the elements."""
    return np.stack([store[f:f + T] for f in clip_first_frames(frames_per_video, clips, T)])


def stage(frame_format, frames_store, density_store, fix_store, frames_per_video, clips, T, mean_rgb):
    """(x, y, fix) after a stage; y / fix None where their store is None.  frames_store: bytes [sum F, H, W, 3] BGR for "u8" (or the
    flat [sum F, hw, 3]), the normalised floats for "f32"."""
    fr = cut(frames_store, frames_per_video, clips, T)
    x = normalise_u8(fr, mean_rgb) if frame_format == "u8" else fr
    y = density_f32(cut(density_store, frames_per_video, clips, T)) if density_store is not None else None
    fix = cut(fix_store, frames_per_video, clips, T) if fix_store is not None else None
    return x, y, fix
