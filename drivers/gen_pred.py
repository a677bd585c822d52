#!/usr/bin/env python3
"""Python-3 counterpart of the reference's sliding-window inference (gen_pred.py) on libp3dhip.

For every video: a 16-frame queue slides by ONE frame (gen_pred.py:100-134); the first window emits all 16 maps,
every later window only its last map (gen_pred.py:154-168); frames are normalised like gen_pred.py:117-121
((RGB - [90,102,98]) / 255 after resizing to 112x112) by the fused GPU pass of sap3d_tensorflow_amd.dataflow.  cv2 is outside
this path, so a video here is a .npy array [F,H,W,3] uint8 RGB (decoding the reference's JPEG folders is out of scope).
Stride-1 windows are batched (`--batch`) instead of run one by one: `p3d_predict_windows` gives every window the result of
its own batch-of-1 run (the backbone BatchNorm uses batch statistics even at inference, p3d.py:140, so a plain batched
forward would couple the windows).

Output (`--write`):
  npy       one float32 array [F,112,112] per video, <out>/<video>.npy (the default);
  png, jpg  the reference's write-out (gen_pred.py:154-168): <out>/<video>/frame_<k>.<ext>, k = 1..F, one 8-bit image per
            frame at `--size` (1080x960), the bytes cv2.imwrite(cv2.resize(float64(map * 255.), (960, 1080))) encodes,
            resized and quantised on the GPU (P3DSession.pred_maps_u8).  A video whose directory exists is skipped
            (gen_pred.py:83-86).  PNG is lossless: its pixels are exactly those bytes.  JPEG is written by PIL at
            quality 95 (cv2's default); the files are not byte-identical to cv2's encoder.  Files are encoded on `--writers`
            threads while the GPU runs the next batch.  --blur-sigma / --blur-radius / --normalize (an addition) smooth and
            normalise every map at `--size` on the GPU before it is quantised (P3DSession.set_postprocess).

`--resident` (an addition) keeps a video on the device instead: the uint8 frames are normalised straight into a frame store
(P3DSession.video_put_u8), windows are cut there (video_predict) and the maps are read once per video.  `--stride N` places a
window every N frames, and a last one at F - 16 so that every frame is covered; `--overlap newest` gives a frame the map of the
first window that holds it (at stride 1 the reference's rule: the npy files hold the default path's bytes), `--overlap mean` the
mean of every window that predicted it.  A stride other than 1 and `--overlap mean` imply `--resident`.  `--temporal gauss|ema`
(an addition, implies `--resident`) smooths the maps along the frame axis on the device as they are read
(P3DSession.set_video_temporal): a Gaussian of `--temporal-sigma` frames (radius `--temporal-radius`, at most 24; 0: cv2's rule)
with reflected ends, or the causal moving average m_f = A m_{f-1} + (1 - A) v_f of `--temporal-alpha`; npy files then hold the
filtered maps, png / jpg the images of the filtered maps.  `--render DIR` (an addition, needs `--resident`) also keeps the
decoded frames on the device and writes DIR/<video>/frame_<k>.png: every frame at its own size with its 8-bit map laid over it
on the device (P3DSession.video_render), whatever `--write` and `--truth` do beside it.  `--shots detect|FILE.npy` (an addition, needs `--resident`) installs a
shot table on every video before its maps are read -- the hard cuts found on the device in the decoded frames
(P3DSession.video_detect_shots, shaped by `--shots-grid`, `-threshold`, `-window`, `-ratio`, `-min-length`), or the starts in FILE.npy
-- so that `--temporal` filters inside the shots and `--reframe` smooths its track inside them; it writes `<out>/<video>_shots.npy`
and, under detect, `<out>/<video>_cutsignal.npy`.  `--shots-gradual` (an addition, with `--shots detect`) finds dissolves and fades as
well (P3DSession.video_detect_transitions, shaped by `--shots-lag`, `-high`, `-dip`, `-mono`, `-mono-min`) and also writes
`<out>/<video>_shotkinds.npy`, `_lagsignal.npy` and `_spread.npy`.  `--shot-windows` (an addition, needs `--shots`) installs the table before the
windows are cut and keeps every window inside its shot (P3DSession.video_predict_shots, dataflow.shot_window_starts): per shot a
window every `--stride` frames and a last one at the shot's end; a shot shorter than 16 frames takes one window, filled by reflecting
inside the shot, and no map is predicted from frames of another shot.  `--reframe DIR` (an addition, needs
`--resident`, may stand beside `--render`) writes DIR/<video>/frame_<k>.png, every frame cut -- not resized -- to the window of
`--reframe-size HC WC` or `--reframe-aspect A:B` (width : height; default 9:16) that holds the most saliency at or above
`--reframe-gate`, on a track averaged over `--reframe-smooth` frames to either side (P3DSession.video_reframe, one call per
video so that the filter sees all of it), and DIR/<video>/track.npy, int64 [F, 7]: the smoothed (y, x), the raw (y, x), and the
masses of the best window, of the window taken and of the whole map.  `--regions DIR` (an addition, needs `--resident`) writes
DIR/<video>/regions.npy, int32 [F, K, 15], and counts.npy, int32 [F, 3]: the connected regions of every map's pixels at or above
`--regions-gate` (`--regions-connectivity` 4 or 8), the `--regions-max` heaviest of at least `--regions-min-area` pixels a frame,
each with its box, area, mass, peak and centre (P3DSession.video_regions at `--size`, one call per video; the fields are
include/p3d_hip.h's P3D_REGION_*); `--regions-link` carries an ID from frame to frame by overlap, inside the shots of `--shots`;
`--regions-labels` also writes labels.npy, uint8 [F, H, W].  `--qpmap DIR` (an addition, needs `--resident`) writes
DIR/<video>/qp.npy, int32 [F, Hb, Wb]: one signed quantiser offset per `--qp-block` x `--qp-block` coding block of every map at
`--size`, lower where the map is salient (P3DSession.video_qpmap, one call per video; the law is include/p3d_hip.h's "QP maps of 8-bit
maps"), limited from frame to frame by `--qp-fall` / `--qp-rise` inside the shots of `--shots`; stats.npy, int32 [F, 4] (the smallest
and largest offset, the area-weighted sums before and after the balance), on `--qp-levels` levels.npy, uint8 [F, Hb, Wb], and qp.txt,
one line a frame: the frame's number from 1, then its Hb * Wb offsets in raster order, separated by spaces.  That layout is this
driver's own; no particular encoder's input format is promised.  `--prefilter DIR` (an addition, needs `--resident`, keeps the decoded
frames on the device) writes DIR/<video>/frame_<k>.png: every frame at its own size, low-pass filtered where its map is not salient
and bit-exact where it is (P3DSession.video_prefilter, the law is include/p3d_hip.h's "Pre-filtering frames by their 8-bit maps"), for
any encoder to take; grid.npy, int32 [F, Hb, Wb], holds the strength 0 .. 64 of every `--pf-block` block, limited from frame to frame
by `--pf-fall` / `--pf-rise` inside the shots of `--shots`.  `--distortion DIR` (an addition, needs `--resident`) compares
DIR/<video>.npy, uint8 [F, H0, W0, 3] in the videos' own channel order -- the frames as an encoder or a filter left them -- with the
decoded frames kept on the device (or with `--dist-ref DIR`'s arrays) under the video's maps at the frames' size
(P3DSession.video_distortion, the law is include/p3d_hip.h's "Distortion of frames under their 8-bit maps") and writes, into `--out`,
<video>_distortion.npy, int64 [F, 20]: the table of integer sums; on `--dist-block` <video>_block_sse.npy, int64 [F, Hb, Wb]; and
<video>_distortion.csv, a line a frame: PSNR and saliency-weighted PSNR of the planes B, G, R, Y, SSIM and weighted SSIM of Y, and the
share of the pixels at or above `--dist-gate` that changed."""
import argparse
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

def preprocess(video_u8, device=0):
    """gen_pred.py:117-121 per frame (RGB - mean, resize to 112, / 255) as one fused GPU pass (csrc/metrics.hip);
    the kernel takes cv2's BGR order, the .npy videos here are RGB."""
    from sap3d_tensorflow_amd import dataflow
    return dataflow.mapf_frames(np.ascontiguousarray(video_u8[..., ::-1]), 112, device=device)


def predict_video(sess, frames, batch):
    """frames [F,112,112,3] normalised -> saliency [F,112,112] with the reference's write-out rule."""
    F = len(frames)
    if F < 16:
        raise ValueError("need at least 16 frames")
    out = np.zeros((F, 112, 112), np.float32)
    starts = list(range(F - 15))
    for i in range(0, len(starts), batch):
        chunk = starts[i:i + batch]
        clips = np.stack([frames[s:s + 16] for s in chunk] + [frames[chunk[-1]:chunk[-1] + 16]] * (batch - len(chunk)))
        maps = sess.predict_windows(clips)[..., 0]       # = B batch-of-1 forwards (gen_pred.py:151), see include/p3d_hip.h
        for k, s in enumerate(chunk):
            if s == 0:
                out[:16] = maps[k]            # first window: all 16 maps
            else:
                out[s + 15] = maps[k, -1]     # later windows: the newest frame only
    return out


def predict_video_images(sess, frames, batch, size=(1080, 960), scale=255.):
    """The image mode of predict_video: the same windows and batches, but every batch's maps are resized and quantised on the
    device (P3DSession.pred_maps_u8 with first_frame 0 for the window at s = 0, 15 for later ones, T for padding).  Yields,
    per batch, (frames, maps): the 0-based frame index of every map and the uint8 maps [n, H, W]."""
    F = len(frames)
    if F < 16:
        raise ValueError("need at least 16 frames")
    starts = list(range(F - 15))
    for i in range(0, len(starts), batch):
        chunk = starts[i:i + batch]
        clips = np.stack([frames[s:s + 16] for s in chunk] + [frames[chunk[-1]:chunk[-1] + 16]] * (batch - len(chunk)))
        sess.predict_windows(clips)
        first = [0 if s == 0 else 15 for s in chunk] + [16] * (batch - len(chunk))
        maps = sess.pred_maps_u8(first, size=size, scale=scale)
        yield [s + t for s, f0 in zip(chunk, first) for t in range(f0, 16)], maps


def window_starts(F, stride):
    """Window starts 0, stride, 2 stride, ... and a last window at F - 16, so that every frame is covered."""
    starts = list(range(0, F - 15, stride))
    if starts[-1] != F - 16:
        starts.append(F - 16)
    return starts


PUT_CHUNK = 64      # frames per upload of the resident path


def predict_video_resident(sess, video_u8, batch, stride=1, overlap="newest", times=None, keep_source=False, shot_windows=None):
    """video_u8 [F,H0,W0,3] uint8 RGB -> the open video on the device, every window predicted (P3DSession.open_video /
    video_put_u8 / video_predict); read it with sess.video_maps / video_maps_u8.  times (a dict or None) collects the HIP-event
    milliseconds of the window cuts and map folds.  keep_source: the decoded frames stay on the device too, for video_render.
    shot_windows (--shot-windows; a callable F -> the shot starts, which installs the video's shot table once the frames are put):
    the windows are dataflow.shot_window_starts' and stay inside their shots (video_predict_shots)."""
    F = len(video_u8)
    if F < 16:
        raise ValueError("need at least 16 frames")
    sess.open_video(F, overlap)
    if keep_source:
        sess.video_keep_source(True)
    for i in range(0, F, PUT_CHUNK):
        sess.video_put_u8(i, video_u8[i:i + PUT_CHUNK, ..., ::-1])       # the kernel takes cv2's BGR order
    if shot_windows is not None:
        from sap3d_tensorflow_amd import dataflow
        starts, predict = dataflow.shot_window_starts(shot_windows(F), F, stride), sess.video_predict_shots
    else:
        starts, predict = window_starts(F, stride), sess.video_predict
    for i in range(0, len(starts), batch):
        predict(starts[i:i + batch])
        if times is not None:
            ms = sess.video_last_ms()
            times["gather"] = times.get("gather", 0.0) + ms["gather"]
            times["scatter"] = times.get("scatter", 0.0) + ms["scatter"]
            times["batches"] = times.get("batches", 0) + 1
    return F


class ChunkWriter:
    """Encodes chunks of images on `writers` threads (PIL releases the GIL while it compresses) while the device runs the next
    chunk.  hand_over(frames, images) waits for the chunk in flight, encoded while this one ran on the device, then submits
    write_one(frame, image) for every pair; leaving the `with` block waits for the last chunk.  So at most two chunks of images
    are held, and an exception of write_one surfaces in the caller at the next hand_over or at the block's end.  encode_ms: the
    thread time spent in write_one."""

    def __init__(self, writers, write_one):
        import threading
        from concurrent.futures import ThreadPoolExecutor
        self.pool, self.lock = ThreadPoolExecutor(max_workers=writers), threading.Lock()
        self.write_one, self.held, self.encode_ms = write_one, [], 0.0

    def _write(self, f, m):
        t0 = time.perf_counter()
        self.write_one(f, m)
        with self.lock:
            self.encode_ms += (time.perf_counter() - t0) * 1e3

    def wait(self):
        held, self.held = self.held, []
        for fut in held:
            fut.result()

    def hand_over(self, frames, images):
        self.wait()
        self.held = [self.pool.submit(self._write, f, m) for f, m in zip(frames, images)]

    def __enter__(self):
        return self

    def __exit__(self, kind, *_):
        try:
            if kind is None:
                self.wait()
        finally:
            self.pool.shutdown(wait=True)


def write_video_images_resident(sess, F, video_dir, ext, size=(1080, 960), writers=4):
    """write_video_images for the open video: its maps leave the device 16 at a time (video_maps_u8) while the previous 16 are
    encoded.  Returns the same dict; gpu is the wall time of the map stages alone."""
    t = dict(gpu=0.0, device=0.0, d2h=0.0, encode=0.0, files=0)
    with ChunkWriter(writers, lambda f, m: save_image(os.path.join(video_dir, "frame_%d.%s" % (f + 1, ext)), m, ext)) as w:
        for first in range(0, F, 16):
            n = min(16, F - first)
            t0 = time.perf_counter()
            maps = sess.video_maps_u8(first, n, size=size)
            t["gpu"] += (time.perf_counter() - t0) * 1e3
            t["device"] += sess.last_maps_ms["device"]
            t["d2h"] += sess.last_maps_ms["d2h"]
            w.hand_over(range(first, first + n), maps)
            t["files"] += n
    t["encode"] = w.encode_ms
    return t


def render_video_resident(sess, F, video_dir, render, writers=4):
    """--render: the open video's frames with their maps laid over them (P3DSession.video_render on the kept source, at the
    video's own size), 16 at a time while the previous 16 are encoded -> <video_dir>/frame_<k>.png, k = 1..F, colour.  render:
    the keyword arguments of video_render.  Returns milliseconds: gpu (wall time of the calls), the three device stages, encode
    (thread time), and the number of files."""
    t = dict(gpu=0.0, upload=0.0, device=0.0, render=0.0, encode=0.0, files=0)
    with ChunkWriter(writers, lambda f, m: save_color_image(os.path.join(video_dir, "frame_%d.png" % (f + 1)), m)) as w:
        for first in range(0, F, 16):
            n = min(16, F - first)
            t0 = time.perf_counter()
            images = sess.video_render(first, n, timed=True, **render)
            t["gpu"] += (time.perf_counter() - t0) * 1e3
            for k in ("upload", "device", "render"):
                t[k] += sess.last_render_ms[k]
            w.hand_over(range(first, first + n), images)
            t["files"] += n
    t["encode"] = w.encode_ms
    return t


def aspect_window(H, W, a, b):
    """--reframe-aspect a:b (width : height): the largest window (hc, wc) of that aspect that fits an H x W frame -- the full width
    where W / a <= H / b, else the full height, the other side the floor of the exact ratio -- each side rounded down to an even
    number (a side of one pixel stays one)."""
    if W * b <= H * a:
        hc, wc = W * b // a, W
    else:
        hc, wc = H, H * a // b
    return max(hc // 2 * 2, 1), max(wc // 2 * 2, 1)


TRACK_COLUMNS = ("y", "x", "raw_y", "raw_x", "mass_best", "mass_smoothed", "mass_total")      # a row of track.npy


def reframe_video_resident(sess, F, video_dir, reframe, writers=4):
    """--reframe: the open video's frames cut to the window that follows their saliency (P3DSession.video_reframe on the kept
    source, at the video's own size) -> <video_dir>/frame_<k>.png, k = 1..F, colour, and <video_dir>/track.npy, int64 [F, 7] in
    TRACK_COLUMNS' order.  ONE call for the whole video: the track's filter sees every frame.  reframe: dict(size=(hc, wc) or
    aspect=(a, b), gate, smooth).  Returns milliseconds: gpu (wall time of the call), the three device stages, encode (thread
    time), the number of files and the window."""
    t = dict(gpu=0.0, upload=0.0, device=0.0, reframe=0.0, encode=0.0, files=0)
    H0, W0 = sess.video_source_info()["size"]
    crop = tuple(reframe["size"]) if reframe.get("size") else aspect_window(H0, W0, *reframe["aspect"])
    if not (1 <= crop[0] <= H0 and 1 <= crop[1] <= W0):
        raise ValueError("--reframe: a %d x %d window does not fit the video's %d x %d frames" % (crop + (H0, W0)))

    t0 = time.perf_counter()
    res = sess.video_reframe(0, F, crop, gate=reframe["gate"], smooth=reframe["smooth"], with_raw=True, with_mass=True, timed=True)
    t["gpu"] = (time.perf_counter() - t0) * 1e3
    for k in ("upload", "device", "reframe"):
        t[k] = sess.last_reframe_ms[k]
    np.save(os.path.join(video_dir, "track.npy"), np.concatenate([res["track"], res["raw"], res["mass"]], axis=1).astype(np.int64))
    with ChunkWriter(writers, lambda f, m: save_color_image(os.path.join(video_dir, "frame_%d.png" % (f + 1)), m)) as w:
        for first in range(0, F, 16):
            w.hand_over(range(first, min(first + 16, F)), res["crop"][first:first + 16])
    t["encode"], t["files"], t["window"] = w.encode_ms, F, crop
    return t


SCORE_CHUNK = 64     # frames per scoring call of --truth
SCORE_NAMES = ("cc", "sim", "judd", "kl", "nss")       # the columns of a row of scores, in order


def load_truth(truth_dir, name, F, size):
    """--truth's arrays of one video: <name>_density.npy and <name>_fixation.npy, uint8 [F, H, W] at --size."""
    out = []
    for what in ("density", "fixation"):
        path = os.path.join(truth_dir, "%s_%s.npy" % (name, what))
        a = np.load(path)
        if a.dtype != np.uint8 or a.shape != (F,) + tuple(size):
            raise ValueError("--truth: %s is %s %s, the video needs uint8 %s" % (path, a.dtype, a.shape, (F,) + tuple(size)))
        out.append(a)
    return out


def nan_means(scores):
    """Column means of [F, 5] scores with the NaN rows of a column dropped (np.nanmean; a column of NaN stays NaN)."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanmean(np.asarray(scores, np.float64).reshape(-1, len(SCORE_NAMES)), axis=0)


def format_means(means):
    return ", ".join("%s=%r" % (k, float(v)) for k, v in zip(SCORE_NAMES, means))


def sauc_ids(rng, P, c0, c1, M, own):
    """The pool slots whose union frames c0 .. c1 - 1 sample shuffled AUC's locations from, int32 [c1 - c0, M], drawn row by row in
    frame order (repeats allowed).  own: the pool is the video's own P fixation maps, slot = frame, and a frame never draws itself:
    randint over the P - 1 others."""
    ids = np.empty((c1 - c0, M), np.int32)
    for f in range(c0, c1):
        if own:
            r = rng.randint(0, P - 1, M)
            ids[f - c0] = r + (r >= f)
        else:
            ids[f - c0] = rng.randint(0, P, M)
    return ids


def score_video_resident(sess, F, density, fixation, size, columns, ties, auc=None, video_dir=None, ext=None, writers=4):
    """Scores the open video against its ground truth on the device, SCORE_CHUNK frames a call -> (scores float64 [F, 5], auc,
    times).  auc None: P3DSession.video_score; the 8-bit maps stay on the device unless video_dir asks for the images: then each
    call also returns its bytes and they are encoded as write_video_images_resident encodes them, while the next call runs.
    auc, a dict(borji, sauc, pool_size, own_pool, n_rep, step, seed): AUC-Borji and / or shuffled AUC of the same bytes as well
    (P3DSession.video_score_auc; --score-borji, --score-sauc M) -> auc float64 [F, 2]: the Borji and shuffled means per frame, NaN
    where not asked.  One RandomState(seed) per video; per chunk of SCORE_CHUNK frames it draws, in this order: the rows of pool
    slots in frame order (sauc_ids), [video_shuffled_begin], Borji's randint per frame with fixations (metrics.borji_draws_u8),
    metrics.shuffled_draws.  With video_dir the images then come from video_maps_u8, one more run of the maps' chain per chunk."""
    from sap3d_tensorflow_amd import metrics
    scores = np.full((F, len(SCORE_NAMES)), np.nan, np.float64)
    means = np.full((F, 2), np.nan, np.float64) if auc else None
    t = dict(upload=0.0, device=0.0, score=0.0, files=0, **(dict(auc=0.0) if auc else {}))
    rng = np.random.RandomState(auc["seed"]) if auc else None
    with ChunkWriter(writers, lambda f, m: save_image(os.path.join(video_dir, "frame_%d.%s" % (f + 1, ext)), m, ext)) as w:
        for first in range(0, F, SCORE_CHUNK):
            n = min(SCORE_CHUNK, F - first)
            den, fix, maps = density[first:first + n], fixation[first:first + n], None
            if not auc:
                got = sess.video_score(first, n, den, fix, size=size, columns=columns, ties=ties, with_maps=video_dir is not None)
                if video_dir is not None:
                    got, maps = got
            else:
                n_other = bidx = ranks = n_rows = None
                if auc["sauc"]:
                    n_other = sess.video_shuffled_begin(sauc_ids(rng, auc["pool_size"], first, first + n, auc["sauc"], auc["own_pool"]))
                nf = np.count_nonzero(fix.reshape(n, -1) >= 128, axis=1)
                if auc["borji"]:
                    bidx, nf = metrics.borji_draws_u8(fix, auc["n_rep"], rng)
                if auc["sauc"]:
                    ranks, n_rows = metrics.shuffled_draws(nf, n_other, auc["n_rep"], rng)
                res = sess.video_score_auc(first, n, den, fix, size=size, columns=columns, ties=ties, borji_idx=bidx, shuffled_ranks=ranks,
                                           n_rows=n_rows, n_rep=auc["n_rep"], step_size=auc["step"])
                got = res["scores"]
                if auc["borji"]:
                    means[first:first + n, 0] = [np.mean(r) for r in res["borji"]]
                if auc["sauc"]:
                    means[first:first + n, 1] = [np.mean(r) for r in res["shuffled"]]
            for k, ms in sess.last_score_ms.items():
                t[k] += ms
            scores[first:first + n] = got
            if video_dir is not None:
                w.hand_over(range(first, first + n), sess.video_maps_u8(first, n, size=size) if auc else maps)
                t["files"] += n
    return scores, means, t


def auc_means(auc):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanmean(np.asarray(auc, np.float64).reshape(-1, 2), axis=0)


def format_auc(means):
    return "borji=%r, sauc=%r" % (float(means[0]), float(means[1]))


def save_image(path, m, ext):
    """One 8-bit map with PIL: PNG at compress_level 1 (lossless: the level changes the file size, not the pixels), JPEG at
    quality 95 (cv2.IMWRITE_JPEG_QUALITY's default)."""
    from PIL import Image
    if m.dtype != np.uint8 or m.ndim != 2:
        raise ValueError("expected a [H, W] uint8 map")
    if ext == "png":
        Image.fromarray(m).save(path, format="PNG", compress_level=1)
    else:
        Image.fromarray(m).save(path, format="JPEG", quality=95)


def save_color_image(path, bgr):
    """One rendered frame [H, W, 3] uint8 in B, G, R order as a colour PNG (compress_level 1, lossless)."""
    from PIL import Image
    if bgr.dtype != np.uint8 or bgr.ndim != 3 or bgr.shape[2] != 3:
        raise ValueError("expected a [H, W, 3] uint8 image")
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(path, format="PNG", compress_level=1)


def write_video_images(sess, frames, batch, video_dir, ext, size=(1080, 960), writers=4):
    """<video_dir>/frame_<k>.<ext>, k = 1..F (gen_pred.py:159,165).  A batch's files are encoded on a pool of `writers`
    threads (PIL releases the GIL while it compresses) while the device runs the next batch; at most two batches of maps are
    held.  Returns milliseconds: gpu (wall time of the forward passes and map stages), device / d2h (pred_maps_u8's device
    times), encode (thread time spent encoding), and the number of files."""
    t = dict(gpu=0.0, device=0.0, d2h=0.0, encode=0.0, files=0)
    with ChunkWriter(writers, lambda f, m: save_image(os.path.join(video_dir, "frame_%d.%s" % (f + 1, ext)), m, ext)) as w:
        batches = predict_video_images(sess, frames, batch, size=size)
        while True:
            t0 = time.perf_counter()
            nxt = next(batches, None)
            t["gpu"] += (time.perf_counter() - t0) * 1e3
            if nxt is None:
                break
            idx, maps = nxt
            ms = getattr(sess, "last_maps_ms", None) or {}
            t["device"] += ms.get("device", 0.0)
            t["d2h"] += ms.get("d2h", 0.0)
            w.hand_over(idx, maps)
            t["files"] += len(idx)
    t["encode"] = w.encode_ms
    return t


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--model", type=str, default="", help="checkpoint: a directory with a TF `checkpoint` state file (gen_pred.py:57-64), "
                   "a TF bundle prefix, or an .npz keyed by TF variable names")
    p.add_argument("--ema", action="store_true", help="[addition] predict with the moving averages of the checkpoint: every trainable "
                   "is restored from <var>/ExponentialMovingAverage (train.py --ema-decay; P3DSession.restore ema_as_weights)")
    p.add_argument("--structure", type=str, default="unet++ds",
                   help="graph to build: unet++ds = p3d_unetplusplus_ds, the buildable form of what gen_pred.py:46 constructs; or unet, "
                        "concat, unet++nonsa, gn_p3d, gn_p3d_concat, gn_p3d_decoder")
    p.add_argument("--videos", type=str, required=True, help="folder with <name>.npy videos [F,H,W,3] uint8 RGB")
    p.add_argument("--out", type=str, default="pred")
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--gpu", type=str, default="0")
    p.add_argument("--write", choices=("npy", "png", "jpg"), default="npy",
                   help="npy: one float32 [F,112,112] array per video; png / jpg: the reference's 8-bit frame_<k> images per video "
                        "(gen_pred.py:154-168), resized and quantised on the GPU.  PNG pixels are exactly the bytes cv2.imwrite "
                        "would encode; JPEG is PIL's encoder at quality 95, not byte-identical to cv2's")
    p.add_argument("--size", type=int, nargs=2, default=(1080, 960), metavar=("H", "W"), help="image size for png / jpg")
    p.add_argument("--blur-sigma", type=float, default=0., metavar="S", help="[addition] png / jpg: smooth every map at --size with a "
                   "Gaussian of S pixels before it is quantised (P3DSession.set_postprocess; the resize is then the float32 one)")
    p.add_argument("--blur-radius", type=int, default=0, metavar="R", help="[addition] the Gaussian's radius in pixels, at most 255; "
                   "0: cv2's rule, (int(rint(8 S + 1)) | 1) // 2")
    p.add_argument("--normalize", choices=("none", "max", "range"), default="none",
                   help="[addition] png / jpg: scale every (smoothed) map by its maximum, or to its range, before it is quantised")
    p.add_argument("--match-hist", type=str, default="", metavar="FILE.npz", help="[addition] png / jpg: match the histogram of every "
                   "(smoothed) map to the table of FILE.npz (`cdf`, `bin_centers`) before it is normalised and quantised "
                   "(utils/metric_utils.py match_hist; P3DSession.set_hist_match)")
    p.add_argument("--match-bins", type=int, default=256, metavar="N", help="[addition] bins of --match-hist's histograms, 2 .. 1024")
    p.add_argument("--prior", type=str, default="", metavar="FILE.npy", help="[addition] png / jpg: combine every (smoothed) map at --size "
                   "with the prior map of this .npy, float32 [H, W] at --size, before it is matched, normalised and quantised "
                   "(P3DSession.set_prior_stage; drivers/test.py builds such a map from fixations)")
    p.add_argument("--prior-mode", choices=("mul", "mix"), default="mul", help="[addition] v ((1 - A) g + A), or (1 - A) v + A g")
    p.add_argument("--prior-weight", type=float, default=0., metavar="A", help="[addition] the weight A in [0, 1]")
    p.add_argument("--writers", type=int, default=4, help="encoder threads for png / jpg (at most 16)")
    p.add_argument("--resident", action="store_true", help="[addition] keep every video on the device: frames go up once as uint8, "
                   "windows are cut there and the maps are read once per video (P3DSession.open_video)")
    p.add_argument("--stride", type=int, default=1, metavar="N", help="[addition] a window every N frames (and a last one at F - 16); "
                   "1 is the reference's.  Other values imply --resident")
    p.add_argument("--overlap", choices=("newest", "mean"), default="newest", help="[addition] a frame's map: that of the first window "
                   "that holds it (at stride 1 the reference's rule), or the mean of every window that predicted it (implies --resident)")
    p.add_argument("--temporal", choices=("off", "gauss", "ema"), default="off", help="[addition] smooth the maps along the frame axis on "
                   "the device as they are read (P3DSession.set_video_temporal): a Gaussian over the whole video with reflected ends, or "
                   "the causal moving average (implies --resident)")
    p.add_argument("--temporal-sigma", type=float, default=0., metavar="S", help="[addition] --temporal gauss: the Gaussian's sigma in frames, > 0")
    p.add_argument("--temporal-radius", type=int, default=0, metavar="R", help="[addition] --temporal gauss: the radius in frames, at most "
                   "24 and at most F - 1; 0: cv2's rule, (int(rint(8 S + 1)) | 1) // 2")
    p.add_argument("--temporal-alpha", type=float, default=0., metavar="A", help="[addition] --temporal ema: m_f = A m_{f-1} + (1 - A) v_f, "
                   "A in [0, 1)")
    p.add_argument("--truth", type=str, default="", metavar="DIR", help="[addition] score every frame's 8-bit map at --size on the device "
                   "against DIR/<name>_density.npy and DIR/<name>_fixation.npy, uint8 [F, H, W] at --size (fixated: byte >= 128): the "
                   "arithmetic of utils/matlab_metric/metric_video_base.m (P3DSession.video_score).  Writes <out>/<name>_scores.npy, "
                   "[F, 5]: CC, SIM, AUC_Judd, KL, NSS, and prints the means (implies --resident)")
    p.add_argument("--score-columns", type=str, nargs="+", default=["cc", "sim", "judd"], choices=("cc", "sim", "judd", "kl", "nss", "matlab"),
                   metavar="COLUMN", help="[addition] --truth: the columns to compute, of cc sim judd kl nss; the others are NaN.  The "
                   "default, also spelled matlab, is the .m file's masks")
    p.add_argument("--score-ties", choices=("reference", "expected"), default="expected", help="[addition] --truth: AUC_Judd on equal bytes: "
                   "utils/metrics.py with jitter=False, or its mean over every order of the tied pixels (what the default jitter does "
                   "to an 8-bit map, without a draw)")
    p.add_argument("--score-borji", action="store_true", help="[addition] --truth: also AUC-Borji of every frame, metric_video_base.m's "
                   "sixth column, on the device (P3DSession.video_score_auc).  Writes <out>/<name>_auc.npy, [F, 2]: the Borji and "
                   "shuffled-AUC means per frame, NaN where not asked, and prints their means")
    p.add_argument("--score-sauc", type=int, default=0, metavar="M", help="[addition] --truth: also shuffled AUC of every frame, its random "
                   "locations the fixations of M other maps of the pool (1 .. 64)")
    p.add_argument("--sauc-pool", type=str, default="", metavar="FILE.npy", help="[addition] --score-sauc: uint8 [P, H, W] fixation maps of other "
                   "videos at --size.  Without it the pool is the video's own frames, and a frame never draws itself")
    p.add_argument("--score-rep", type=int, default=100, metavar="N", help="[addition] --score-borji / --score-sauc: random splits per frame")
    p.add_argument("--score-step", type=float, default=0.1, metavar="S", help="[addition] --score-borji / --score-sauc: the threshold step, "
                   "at most 1024 thresholds")
    p.add_argument("--score-seed", type=int, default=0, metavar="N", help="[addition] --score-borji / --score-sauc: the seed of every video's "
                   "numpy RandomState, which makes all draws")
    p.add_argument("--render", type=str, default="", metavar="DIR", help="[addition] needs --resident: keep every video's decoded frames on "
                   "the device and write DIR/<video>/frame_<k>.png, the frame at its own size with its 8-bit map laid over it, colour-"
                   "mapped and blended on the device (every read-out setting the maps follow applies)")
    p.add_argument("--render-colormap", choices=("grey", "hot", "jet"), default="jet", help="[addition] --render: the colour of a level")
    p.add_argument("--render-alpha", type=float, default=0.6, metavar="A", help="[addition] --render: the overlay's weight in [0, 1]")
    p.add_argument("--render-opacity", choices=("ramp", "constant"), default="ramp", help="[addition] --render: a level's opacity, "
                   "A * level / 255 or A at every level")
    p.add_argument("--render-gate", type=int, default=0, metavar="LEVEL", help="[addition] --render: levels below it are transparent")
    p.add_argument("--render-contour", type=int, default=0, metavar="LEVEL", help="[addition] --render: draw the iso-line of this level, "
                   "1 .. 255 (0: none)")
    p.add_argument("--render-thickness", type=int, default=1, metavar="T", help="[addition] --render-contour: the line's width, 1 .. 4 pixels")
    p.add_argument("--render-contour-color", type=str, default="255,255,255", metavar="R,G,B", help="[addition] --render-contour: the line's colour")
    p.add_argument("--reframe", type=str, default="", metavar="DIR", help="[addition] needs --resident: keep every video's decoded frames on "
                   "the device and write DIR/<video>/frame_<k>.png, the frame cut to the window of the most saliency on a smoothed "
                   "track (not resized), and DIR/<video>/track.npy; may be given together with --render")
    p.add_argument("--reframe-size", type=int, nargs=2, default=None, metavar=("HC", "WC"), help="[addition] --reframe: the window's rows and columns")
    p.add_argument("--reframe-aspect", type=str, default="", metavar="A:B", help="[addition] --reframe: width : height of the window; the largest "
                   "such window that fits the frame, each side rounded down to an even number (default 9:16)")
    p.add_argument("--reframe-gate", type=int, default=0, metavar="LEVEL", help="[addition] --reframe: map levels below it weigh nothing, 0 .. 255")
    p.add_argument("--reframe-smooth", type=int, default=0, metavar="R", help="[addition] --reframe: the track is averaged over R frames to "
                   "either side, 0 .. 255 (0: the raw track)")
    p.add_argument("--regions", type=str, default="", metavar="DIR", help="[addition] needs --resident: label the connected regions of every "
                   "map's pixels at or above --regions-gate on the device (P3DSession.video_regions, one call per video, at --size) and "
                   "write DIR/<video>/regions.npy, int32 [F, K, 15], and counts.npy, int32 [F, 3]")
    p.add_argument("--regions-gate", type=int, default=128, metavar="LEVEL", help="[addition] --regions: a pixel is foreground at or above it, 1 .. 255 (128)")
    p.add_argument("--regions-connectivity", type=int, default=8, metavar="C", help="[addition] --regions: 4 or 8 neighbours (8)")
    p.add_argument("--regions-min-area", type=int, default=1, metavar="PIXELS", help="[addition] --regions: smaller regions are not kept (1)")
    p.add_argument("--regions-max", type=int, default=64, metavar="K", help="[addition] --regions: the K heaviest regions a frame are kept, 1 .. 64 (64)")
    p.add_argument("--regions-link", action="store_true", help="[addition] --regions: regions carry an ID from frame to frame by overlap, "
                   "inside the shots of --shots")
    p.add_argument("--regions-labels", action="store_true", help="[addition] --regions: also write DIR/<video>/labels.npy, uint8 [F, H, W]: a "
                   "region's rank, 255 elsewhere")
    p.add_argument("--qpmap", type=str, default="", metavar="DIR", help="[addition] needs --resident: one signed quantiser offset per coding "
                   "block of every map, lower where the map is salient, on the device (P3DSession.video_qpmap, one call per video, at "
                   "--size); writes DIR/<video>/qp.npy, int32 [F, Hb, Wb], stats.npy, int32 [F, 4], and qp.txt, one line a frame: the frame's "
                   "number from 1, then its Hb * Wb offsets in raster order, separated by spaces.  The layout is this driver's own: no "
                   "particular encoder's input format is promised.  Uses the table of --shots when one is set")
    p.add_argument("--qp-block", type=int, default=16, metavar="B", help="[addition] --qpmap: the coding block's side, 8, 16, 32, 64 or 128 pixels (16)")
    p.add_argument("--qp-peak-weight", type=int, default=128, metavar="Q8", help="[addition] --qpmap: a block's level is Q8 / 256 of its largest "
                   "byte and the rest its mean, 0 .. 256 (128)")
    p.add_argument("--qp-dilate", type=int, default=0, metavar="BLOCKS", help="[addition] --qpmap: a block takes the largest level within this "
                   "many blocks, 0 .. 8 (0)")
    p.add_argument("--qp-fall", type=int, default=0, metavar="STEP", help="[addition] --qpmap: a block's offset falls by at most STEP a frame, "
                   "0 .. 254, 0: unlimited (0)")
    p.add_argument("--qp-rise", type=int, default=0, metavar="STEP", help="[addition] --qpmap: a block's offset rises by at most STEP a frame, "
                   "0 .. 254, 0: unlimited (0)")
    p.add_argument("--qp-min", type=int, default=-12, metavar="Q", help="[addition] --qpmap: the offset of the most salient level, and the clamp's "
                   "lower end, -127 .. 127 (-12)")
    p.add_argument("--qp-max", type=int, default=6, metavar="Q", help="[addition] --qpmap: the offset of the levels below --qp-gate, and the clamp's "
                   "upper end, -127 .. 127 (6)")
    p.add_argument("--qp-gate", type=int, default=0, metavar="LEVEL", help="[addition] --qpmap: levels below it take --qp-max, 0 .. 254 (0)")
    p.add_argument("--qp-gamma", type=float, default=1.0, metavar="G", help="[addition] --qpmap: the law's exponent, > 0 (1: a straight line "
                   "from --qp-max at the gate to --qp-min at level 255)")
    p.add_argument("--qp-no-balance", action="store_true", help="[addition] --qpmap: do not shift every frame's offsets so that their "
                   "area-weighted mean is 0")
    p.add_argument("--qp-levels", action="store_true", help="[addition] --qpmap: also write DIR/<video>/levels.npy, uint8 [F, Hb, Wb]: the "
                   "blocks' dilated levels")
    p.add_argument("--prefilter", type=str, default="", metavar="DIR", help="[addition] needs --resident: keep every video's decoded frames on "
                   "the device and write DIR/<video>/frame_<k>.png, the frame low-pass filtered where its map is not salient and bit-exact "
                   "where it is, on the device (P3DSession.video_prefilter, one call per video, at the frames' own size), and grid.npy, "
                   "int32 [F, Hb, Wb]: the strength 0 .. 64 of every block.  Uses the table of --shots when one is set")
    p.add_argument("--pf-block", type=int, default=16, metavar="B", help="[addition] --prefilter: the side of a strength block, 8, 16, 32, 64 or 128 pixels (16)")
    p.add_argument("--pf-radius", type=int, default=4, metavar="R", help="[addition] --prefilter: a box pass reaches R pixels either way, 1 .. 16 (4)")
    p.add_argument("--pf-passes", type=int, default=2, metavar="P", help="[addition] --prefilter: box passes, 1 .. 3 (2)")
    p.add_argument("--pf-gate", type=int, default=128, metavar="LEVEL", help="[addition] --prefilter: levels from it on are left alone, 0 .. 255 (128)")
    p.add_argument("--pf-full", type=int, default=16, metavar="LEVEL", help="[addition] --prefilter: levels up to it get --pf-strength, 0 .. --pf-gate (16)")
    p.add_argument("--pf-gamma", type=float, default=1.0, metavar="G", help="[addition] --prefilter: the law's exponent between the two, > 0 (1: a straight line)")
    p.add_argument("--pf-strength", type=int, default=64, metavar="S", help="[addition] --prefilter: the largest strength, 0 .. 64 (64: the full low-pass)")
    p.add_argument("--pf-dilate", type=int, default=1, metavar="BLOCKS", help="[addition] --prefilter: a block takes the largest level within this "
                   "many blocks, 0 .. 8 (1)")
    p.add_argument("--pf-peak-weight", type=int, default=128, metavar="Q8", help="[addition] --prefilter: a block's level is Q8 / 256 of its largest "
                   "byte and the rest its mean, 0 .. 256 (128)")
    p.add_argument("--pf-rise", type=int, default=0, metavar="STEP", help="[addition] --prefilter: a block's strength rises by at most STEP a frame, "
                   "0 .. 64, 0: unlimited (0)")
    p.add_argument("--pf-fall", type=int, default=0, metavar="STEP", help="[addition] --prefilter: a block's strength falls by at most STEP a frame, "
                   "0 .. 64, 0: unlimited (0)")
    p.add_argument("--distortion", type=str, default="", metavar="DIR", help="[addition] needs --resident: compare DIR/<video>.npy, uint8 "
                   "[F, H0, W0, 3] (the decoded or filtered frames, in the videos' channel order), with the video's own frames under its maps "
                   "on the device (P3DSession.video_distortion, %d frames a call) and write <video>_distortion.npy (int64 [F, 20], the integer "
                   "sums), <video>_distortion.csv (PSNR, weighted PSNR, SSIM, weighted SSIM a frame) and, on --dist-block, "
                   "<video>_block_sse.npy into --out" % SCORE_CHUNK)
    p.add_argument("--dist-gate", type=int, default=0, metavar="LEVEL", help="[addition] --distortion: pixels at or above it count as salient, and "
                   "levels below it weigh --dist-floor, 0 .. 255 (0: off)")
    p.add_argument("--dist-block", type=int, default=0, metavar="B", help="[addition] --distortion: also write the squared error of every B x B "
                   "block, 8, 16, 32, 64 or 128 (0: no block map)")
    p.add_argument("--dist-gamma", type=float, default=1.0, metavar="G", help="[addition] --distortion: the weight of level v is 255 (v / 255)^G, "
                   "> 0 (1: the level itself)")
    p.add_argument("--dist-floor", type=int, default=0, metavar="W", help="[addition] --distortion: the weight of the levels below --dist-gate, 0 .. 255 (0)")
    p.add_argument("--dist-ref", type=str, default="", metavar="DIR", help="[addition] --distortion: DIR/<video>.npy, uint8 [F, H0, W0, 3], is the "
                   "reference instead of the video's own frames")
    p.add_argument("--shots", type=str, default="", metavar="detect|FILE.npy", help="[addition] needs --resident: a shot table for every video, "
                   "installed before its maps are read (P3DSession.video_set_shots) -- --temporal then filters inside the shots and --reframe "
                   "smooths its track inside them.  detect: the hard cuts found on the device in the decoded frames "
                   "(P3DSession.video_detect_shots; the frames are kept on the device); FILE.npy: the shot starts, ascending from 0.  "
                   "Writes <out>/<video>_shots.npy and, under detect, <out>/<video>_cutsignal.npy")
    p.add_argument("--shot-windows", action="store_true", help="[addition] needs --shots: install the table before the windows are cut and keep "
                   "every window inside its shot (P3DSession.video_predict_shots) -- per shot a window every --stride frames and a last one "
                   "at the shot's end; a shot shorter than 16 frames takes one window, filled by reflecting inside the shot")
    p.add_argument("--shots-grid", type=int, nargs=2, default=None, metavar=("GY", "GX"), help="[addition] --shots detect: cells of histograms a frame, 1 .. 4 each (2 2)")
    p.add_argument("--shots-threshold", type=int, default=None, metavar="PERMILLE", help="[addition] --shots detect: a cut's distance is at least "
                   "this many permille of the largest possible, 1 .. 1000 (250)")
    p.add_argument("--shots-window", type=int, default=None, metavar="FRAMES", help="[addition] --shots detect: the peak rule looks this far to either side, 0 .. 32 (2)")
    p.add_argument("--shots-ratio", type=int, default=None, metavar="Q8", help="[addition] --shots detect: a cut's distance is at least Q8 / 256 times "
                   "every other within the window, 256 .. 65535 (512)")
    p.add_argument("--shots-min-length", type=int, default=None, metavar="FRAMES", help="[addition] --shots detect: the shortest shot, at least 1 (3)")
    p.add_argument("--shots-gradual", action="store_true", help="[addition] --shots detect: find dissolves and fades as well "
                   "(P3DSession.video_detect_transitions); also writes <out>/<video>_shotkinds.npy (0 first, 1 cut, 2 fade, 3 dissolve), "
                   "_lagsignal.npy and _spread.npy")
    p.add_argument("--shots-lag", type=int, default=None, metavar="FRAMES", help="[addition] --shots-gradual: a dissolve is looked for in the distance "
                   "of a frame from the one this many before it, 2 .. 64, 0: no dissolves (12)")
    p.add_argument("--shots-high", type=int, default=None, metavar="PERMILLE", help="[addition] --shots-gradual: that distance is at least this many "
                   "permille of the largest possible through a dissolve, 1 .. 1000 (250)")
    p.add_argument("--shots-dip", type=int, default=None, metavar="Q8", help="[addition] --shots-gradual: the spread of a dissolve's frames falls to "
                   "Q8 / 256 of its ends', 1 .. 256, 256: not asked (230)")
    p.add_argument("--shots-mono", type=int, default=None, metavar="Q8", help="[addition] --shots-gradual: a frame is monochrome up to a spread of "
                   "Q8 / 256 a pixel, 0 .. 65535 (768)")
    p.add_argument("--shots-mono-min", type=int, default=None, metavar="FRAMES", help="[addition] --shots-gradual: the shortest monochrome run that "
                   "ends a shot, 0: no fades (2)")
    p.add_argument("--base", type=int, default=64, help=argparse.SUPPRESS)
    p.add_argument("--blocks", type=str, default="3,8,36", help=argparse.SUPPRESS)
    p.add_argument("--time", action="store_true", help="print per-video wall times (png / jpg: also the device stage and the host encode)")
    args = p.parse_args(argv)
    if not 1 <= args.writers <= 16:
        p.error("--writers must be in 1..16")
    if args.stride < 1:
        p.error("--stride must be at least 1")
    if args.stride != 1 or args.overlap != "newest":
        args.resident = True
    temporal_args(args, p.error)
    if args.temporal != "off":
        args.resident = True
    if args.truth:
        args.resident = True
    elif args.score_columns != ["cc", "sim", "judd"] or args.score_ties != "expected":
        p.error("--score-columns / --score-ties need --truth DIR")
    args.score_auc = bool(args.score_borji or args.score_sauc)
    if not args.truth and (args.score_auc or args.sauc_pool or args.score_rep != 100 or args.score_step != 0.1 or args.score_seed != 0):
        p.error("--score-borji / --score-sauc / --sauc-pool / --score-rep / --score-step / --score-seed need --truth DIR")
    if not 0 <= args.score_sauc <= 64:
        p.error("--score-sauc takes 1 .. 64 other maps")
    if args.sauc_pool and not args.score_sauc:
        p.error("--sauc-pool needs --score-sauc M")
    if args.score_rep < 1 or not args.score_step > 0. or 1. / args.score_step > 1024:
        p.error("--score-rep is at least 1, --score-step positive and at least 1 / 1024")
    if args.truth:
        pass                                          # the stages below shape the scored maps too: --write npy may have them
    elif args.write == "npy" and (args.blur_sigma != 0. or args.blur_radius != 0 or args.normalize != "none"):
        p.error("--blur-sigma / --blur-radius / --normalize shape the images: they need --write png or jpg (npy stays the raw 112x112 maps)")
    if args.write == "npy" and args.match_hist and not args.truth:
        p.error("--match-hist shapes the images: it needs --write png or jpg (npy stays the raw 112x112 maps)")
    if args.match_hist == "density":
        p.error("--match-hist density needs a ground truth: it belongs to drivers/test.py; here it takes FILE.npz")
    if not 2 <= args.match_bins <= 1024:
        p.error("--match-bins must be in 2..1024")
    render_args(args, p.error)
    reframe_args(args, p.error)
    regions_args(args, p.error)
    qpmap_args(args, p.error)
    prefilter_args(args, p.error)
    distortion_args(args, p.error)
    shots_args(args, p.error)
    return args


SHOTS_DEFAULTS = dict(grid=(2, 2), threshold=250, window=2, ratio=512, min_length=3)
GRADUAL_DEFAULTS = dict(lag=12, high=250, dip=230, mono=768, mono_min=2)


def shots_args(args, error):
    """Checks --shots and its values as P3DSession.video_detect_shots would refuse them, before anything runs; error(message) does not
    return.  Leaves dict(detect=dict(grid, threshold, window, ratio, min_length) or None, starts=array or None) in args.shots_kw (None
    without --shots); under --shots-gradual also gradual=dict(lag, high, dip, mono, mono_min), checked as
    P3DSession.video_detect_transitions would refuse it."""
    args.shots_kw = None
    given = dict(grid=args.shots_grid, threshold=args.shots_threshold, window=args.shots_window, ratio=args.shots_ratio, min_length=args.shots_min_length)
    shaped = any(v is not None for v in given.values())
    gradual = dict(lag=args.shots_lag, high=args.shots_high, dip=args.shots_dip, mono=args.shots_mono, mono_min=args.shots_mono_min)
    if args.shots != "detect" and args.shots_gradual:
        error("--shots-gradual needs --shots detect")
    if not args.shots_gradual and any(v is not None for v in gradual.values()):
        error("--shots-lag / -high / -dip / -mono / -mono-min need --shots-gradual")
    if not args.shots:
        if shaped:
            error("--shots-grid / -threshold / -window / -ratio / -min-length need --shots detect")
        if args.shot_windows:
            error("--shot-windows needs --shots detect|FILE.npy: the windows stay inside the table's shots")
        return
    if not args.resident:
        error("--shots needs --resident: the table belongs to a video on the device")
    if args.shots != "detect":
        if shaped:
            error("--shots-grid / -threshold / -window / -ratio / -min-length belong to --shots detect")
        try:
            starts = np.load(args.shots)
        except Exception as e:
            error("--shots %s: %s" % (args.shots, e))
        if starts.ndim != 1 or starts.size < 1 or starts.dtype.kind not in "iu" or starts[0] != 0 or (np.diff(starts.astype(np.int64)) <= 0).any():
            error("--shots %s: the shot starts are integers ascending strictly from 0" % args.shots)
        args.shots_kw = dict(detect=None, starts=starts.astype(np.int32))
        return
    kw = dict((k, SHOTS_DEFAULTS[k] if v is None else v) for k, v in given.items())
    kw["grid"] = tuple(kw["grid"])
    if not all(1 <= g <= 4 for g in kw["grid"]):
        error("--shots-grid is GY GX, 1 .. 4 each")
    if not 1 <= kw["threshold"] <= 1000:
        error("--shots-threshold is 1 .. 1000 permille")
    if not 0 <= kw["window"] <= 32:
        error("--shots-window is 0 .. 32 frames")
    if not 256 <= kw["ratio"] <= 65535:
        error("--shots-ratio is 256 .. 65535 (256: equal neighbours pass)")
    if kw["min_length"] < 1:
        error("--shots-min-length is at least 1 frame")
    args.shots_kw = dict(detect=kw, starts=None)
    if args.shots_gradual:
        g = dict((k, GRADUAL_DEFAULTS[k] if v is None else v) for k, v in gradual.items())
        if g["lag"] != 0 and not 2 <= g["lag"] <= 64:
            error("--shots-lag is 2 .. 64 frames, or 0 for no dissolves")
        if not 1 <= g["high"] <= 1000:
            error("--shots-high is 1 .. 1000 permille")
        if not 1 <= g["dip"] <= 256:
            error("--shots-dip is 1 .. 256 (256: not asked)")
        if not 0 <= g["mono"] <= 65535:
            error("--shots-mono is 0 .. 65535")
        if g["mono_min"] < 0:
            error("--shots-mono-min is a number of frames, or 0 for no fades")
        args.shots_kw["gradual"] = g


def shots_video_resident(sess, F, out_dir, name, shots):
    """--shots: installs the open video's shot table before any map is read and writes <out>/<name>_shots.npy (and _cutsignal.npy
    under detect; _shotkinds.npy, _lagsignal.npy and _spread.npy as well under --shots-gradual).  -> the starts."""
    if shots.get("gradual") is not None:      # --shots-gradual: dissolves and fades as well, the kinds beside the starts
        kw = dict(shots["detect"], **shots["gradual"])
        starts, kinds, D, E, v = sess.video_detect_transitions(install=True, with_signals=True, **kw)
        for suffix, what in (("_cutsignal.npy", D), ("_lagsignal.npy", E), ("_spread.npy", v), ("_shotkinds.npy", np.asarray(kinds, np.int32))):
            np.save(os.path.join(out_dir, name + suffix), what)
    elif shots["detect"] is not None:
        starts, D = sess.video_detect_shots(install=True, with_signal=True, **shots["detect"])
        np.save(os.path.join(out_dir, name + "_cutsignal.npy"), D)
    else:
        starts = shots["starts"]
        if starts[-1] >= F:
            raise ValueError("--shots: a shot starts at frame %d, the video has %d frames" % (starts[-1], F))
        sess.video_set_shots(starts)
    np.save(os.path.join(out_dir, name + "_shots.npy"), np.asarray(starts, np.int32))
    return starts


def regions_args(args, error):
    """Checks --regions and its values as P3DSession.video_regions would refuse them, before anything runs; error(message) does not
    return.  Leaves dict(gate, connectivity, min_area, max_regions, link, labels) in args.regions_kw (None without --regions)."""
    args.regions_kw = None
    shaped = (args.regions_gate != 128 or args.regions_connectivity != 8 or args.regions_min_area != 1 or args.regions_max != 64 or
              args.regions_link or args.regions_labels)
    if not args.regions:
        if shaped:
            error("--regions-gate / -connectivity / -min-area / -max / -link / -labels need --regions DIR")
        return
    if not args.resident:
        error("--regions needs --resident: the maps stay on the device")
    if not 1 <= args.regions_gate <= 255:
        error("--regions-gate is a level, 1 .. 255")
    if args.regions_connectivity not in (4, 8):
        error("--regions-connectivity is 4 or 8")
    if args.regions_min_area < 1:
        error("--regions-min-area is at least 1 pixel")
    if not 1 <= args.regions_max <= 64:
        error("--regions-max is 1 .. 64 regions")
    args.regions_kw = dict(gate=args.regions_gate, connectivity=args.regions_connectivity, min_area=args.regions_min_area,
                           max_regions=args.regions_max, link=args.regions_link, labels=args.regions_labels)


def regions_video_resident(sess, F, video_dir, size, regions):
    """--regions: the open video's maps at `size` labelled on the device (P3DSession.video_regions), ONE call for the whole video so
    that the link sees every frame; writes regions.npy, counts.npy and, on request, labels.npy into video_dir.  -> dict(gpu, device,
    regions: ms; kept: regions kept over the video)."""
    t0 = time.perf_counter()
    res = sess.video_regions(0, F, size, regions["gate"], connectivity=regions["connectivity"], min_area=regions["min_area"],
                             max_regions=regions["max_regions"], link=regions["link"], with_labels=regions["labels"], timed=True)
    t = dict(gpu=(time.perf_counter() - t0) * 1e3, device=sess.last_regions_ms["device"], regions=sess.last_regions_ms["regions"],
             kept=int(res["counts"][:, 2].sum()))
    np.save(os.path.join(video_dir, "regions.npy"), res["regions"])
    np.save(os.path.join(video_dir, "counts.npy"), res["counts"])
    if regions["labels"]:
        np.save(os.path.join(video_dir, "labels.npy"), res["labels"])
    return t


QPMAP_DEFAULTS = dict(qp_block=16, qp_peak_weight=128, qp_dilate=0, qp_fall=0, qp_rise=0, qp_min=-12, qp_max=6, qp_gate=0, qp_gamma=1.0,
                      qp_no_balance=False, qp_levels=False)


def qpmap_args(args, error):
    """Checks --qpmap and its values as P3DSession.video_qpmap and dataflow.qp_law would refuse them, before anything runs;
    error(message) does not return.  Leaves dict(block, peak_weight, dilate, fall, rise, lo, hi, gate, gamma, balance, levels) in
    args.qpmap_kw (None without --qpmap).  The balance's target is 0 where [--qp-min, --qp-max] holds it, else the nearer end."""
    args.qpmap_kw = None
    if not args.qpmap:
        if any(getattr(args, k) != v for k, v in QPMAP_DEFAULTS.items()):
            error("--qp-block / -peak-weight / -dilate / -fall / -rise / -min / -max / -gate / -gamma / -no-balance / -levels need --qpmap DIR")
        return
    if not args.resident:
        error("--qpmap needs --resident: the maps stay on the device")
    if args.qp_block not in (8, 16, 32, 64, 128):
        error("--qp-block is 8, 16, 32, 64 or 128")
    if not 0 <= args.qp_peak_weight <= 256:
        error("--qp-peak-weight is 0 .. 256")
    if not 0 <= args.qp_dilate <= 8:
        error("--qp-dilate is 0 .. 8 blocks")
    if not 0 <= args.qp_fall <= 254 or not 0 <= args.qp_rise <= 254:
        error("--qp-fall and --qp-rise are 0 .. 254")
    if not -127 <= args.qp_min <= args.qp_max <= 127:
        error("-127 <= --qp-min <= --qp-max <= 127")
    if not 0 <= args.qp_gate <= 254:
        error("--qp-gate is a level, 0 .. 254")
    if not (np.isfinite(args.qp_gamma) and args.qp_gamma > 0.):
        error("--qp-gamma is finite and above 0")
    args.qpmap_kw = dict(block=args.qp_block, peak_weight=args.qp_peak_weight, dilate=args.qp_dilate, fall=args.qp_fall, rise=args.qp_rise,
                         lo=args.qp_min, hi=args.qp_max, gate=args.qp_gate, gamma=args.qp_gamma, balance=not args.qp_no_balance,
                         levels=args.qp_levels)


PREFILTER_DEFAULTS = dict(pf_block=16, pf_radius=4, pf_passes=2, pf_gate=128, pf_full=16, pf_gamma=1.0, pf_strength=64, pf_dilate=1,
                          pf_peak_weight=128, pf_rise=0, pf_fall=0)


def prefilter_args(args, error):
    """Checks --prefilter and its values as P3DSession.video_prefilter and dataflow.prefilter_law would refuse them, before anything
    runs; error(message) does not return.  Leaves the keyword arguments of prefilter_video_resident in args.prefilter_kw (None without
    --prefilter)."""
    args.prefilter_kw = None
    if not args.prefilter:
        if any(getattr(args, k) != v for k, v in PREFILTER_DEFAULTS.items()):
            error("--pf-block / -radius / -passes / -gate / -full / -gamma / -strength / -dilate / -peak-weight / -rise / -fall need --prefilter DIR")
        return
    if not args.resident:
        error("--prefilter needs --resident: the frames and the maps stay on the device")
    if args.pf_block not in (8, 16, 32, 64, 128):
        error("--pf-block is 8, 16, 32, 64 or 128")
    if not 1 <= args.pf_radius <= 16 or not 1 <= args.pf_passes <= 3:
        error("--pf-radius is 1 .. 16 and --pf-passes 1 .. 3")
    if not 0 <= args.pf_full <= args.pf_gate <= 255:
        error("0 <= --pf-full <= --pf-gate <= 255")
    if not (np.isfinite(args.pf_gamma) and args.pf_gamma > 0.):
        error("--pf-gamma is finite and > 0")
    if not 0 <= args.pf_strength <= 64:
        error("--pf-strength is 0 .. 64")
    if not 0 <= args.pf_peak_weight <= 256:
        error("--pf-peak-weight is 0 .. 256")
    if not 0 <= args.pf_dilate <= 8:
        error("--pf-dilate is 0 .. 8 blocks")
    if not 0 <= args.pf_fall <= 64 or not 0 <= args.pf_rise <= 64:
        error("--pf-fall and --pf-rise are 0 .. 64 (0: unlimited)")
    args.prefilter_kw = dict(block=args.pf_block, radius=args.pf_radius, passes=args.pf_passes, gate=args.pf_gate, full=args.pf_full,
                             gamma=args.pf_gamma, strength=args.pf_strength, dilate=args.pf_dilate, peak_weight=args.pf_peak_weight,
                             rise=args.pf_rise, fall=args.pf_fall)


def prefilter_video_resident(sess, F, video_dir, prefilter, writers=4):
    """--prefilter: the open video's frames low-pass filtered away from their saliency on the device (P3DSession.video_prefilter on
    the kept source, at the video's own size) -> <video_dir>/frame_<k>.png, k = 1..F, colour, and <video_dir>/grid.npy, int32
    [F, Hb, Wb].  ONE call for the whole video: the limiter sees every frame.  Returns milliseconds: gpu (wall time of the call), the
    device stages, encode (thread time), the number of files, and strength: the area-weighted mean of g / 64 over the video,
    computed here on the host from the grid."""
    from sap3d_tensorflow_amd import dataflow
    H0, W0 = sess.video_source_info()["size"]
    B = prefilter["block"]
    law = dataflow.prefilter_law(prefilter["gate"], prefilter["full"], prefilter["gamma"], prefilter["strength"])
    t0 = time.perf_counter()
    out, grid, _, ms = sess.video_prefilter(0, F, H0, W0, law, block=B, peak_weight=prefilter["peak_weight"], dilate=prefilter["dilate"],
                                            fall=prefilter["fall"], rise=prefilter["rise"], radius=prefilter["radius"], passes=prefilter["passes"])
    t = dict(gpu=(time.perf_counter() - t0) * 1e3, device=ms["device"], prefilter=ms["prefilter"], files=F)
    np.save(os.path.join(video_dir, "grid.npy"), grid)
    hs = np.minimum(H0, (np.arange(grid.shape[1]) + 1) * B) - np.arange(grid.shape[1]) * B
    ws = np.minimum(W0, (np.arange(grid.shape[2]) + 1) * B) - np.arange(grid.shape[2]) * B
    t["strength"] = float((grid.astype(np.float64) * (hs[:, None] * ws[None, :])[None]).sum() / (64.0 * F * H0 * W0))
    with ChunkWriter(writers, lambda f, m: save_color_image(os.path.join(video_dir, "frame_%d.png" % (f + 1)), m)) as w:
        for first in range(0, F, 16):
            w.hand_over(range(first, min(F, first + 16)), out[first:first + 16])
    t["encode"] = w.encode_ms
    return t


DISTORTION_DEFAULTS = dict(dist_gate=0, dist_block=0, dist_gamma=1.0, dist_floor=0, dist_ref="")
DISTORTION_PLANES = ("b", "g", "r", "y")


def distortion_args(args, error):
    """Checks --distortion and its values as P3DSession.video_distortion and dataflow.distortion_law would refuse them, before
    anything is opened; error(message) does not return.  Leaves the keyword arguments of distortion_video_resident in
    args.distortion_kw (None without --distortion)."""
    args.distortion_kw = None
    if not args.distortion:
        if any(getattr(args, k) != v for k, v in DISTORTION_DEFAULTS.items()):
            error("--dist-gate / -block / -gamma / -floor / -ref need --distortion DIR")
        return
    if not args.resident:
        error("--distortion needs --resident: the frames and the maps stay on the device")
    if not 0 <= args.dist_gate <= 255:
        error("--dist-gate is 0 .. 255")
    if args.dist_block not in (0, 8, 16, 32, 64, 128):
        error("--dist-block is 0, 8, 16, 32, 64 or 128")
    if not (np.isfinite(args.dist_gamma) and args.dist_gamma > 0.):
        error("--dist-gamma is finite and > 0")
    if not 0 <= args.dist_floor <= 255:
        error("--dist-floor is 0 .. 255")
    args.distortion_kw = dict(gate=args.dist_gate, block=args.dist_block, gamma=args.dist_gamma, floor=args.dist_floor, ref=args.dist_ref)


def load_distortion_frames(frames_dir, name, F, size, flag):
    """DIR/<name>.npy of --distortion or --dist-ref: uint8 [F, H0, W0, 3] in the videos' channel order; size None: the array names it."""
    path = os.path.join(frames_dir, name + ".npy")
    a = np.load(path)
    if size is None and a.ndim == 4:
        size = a.shape[1:3]
    if a.dtype != np.uint8 or size is None or a.shape != (F,) + tuple(size) + (3,):
        raise ValueError("%s: %s is %s %s, not uint8 %s" % (flag, path, a.dtype, a.shape, (F,) + (tuple(size) if size else ("H0", "W0")) + (3,)))
    return a


def distortion_video_resident(sess, F, out_dir, name, test_dir, distortion):
    """--distortion: the open video's frames against <test_dir>/<name>.npy under the video's maps, on the device
    (P3DSession.video_distortion at the video's own size, SCORE_CHUNK frames a call; the reference is the kept source, or
    --dist-ref's array) -> <out_dir>/<name>_distortion.npy, int64 [F, 20], <name>_distortion.csv and, with a block,
    <name>_block_sse.npy, int64 [F, Hb, Wb].  Returns the report (dataflow.distortion_report), the milliseconds of the calls (gpu:
    wall time) and of the device stages, and the files written."""
    from sap3d_tensorflow_amd import dataflow
    ref = None
    if distortion["ref"]:      # no source is kept: the reference names the size
        ref = load_distortion_frames(distortion["ref"], name, F, None, "--dist-ref")
        H0, W0 = ref.shape[1:3]
    else:
        H0, W0 = sess.video_source_info()["size"]
    test = load_distortion_frames(test_dir, name, F, (H0, W0), "--distortion")
    law = dataflow.distortion_law(distortion["gate"], distortion["gamma"], distortion["floor"])
    tables, blocks = [], []
    t = dict(gpu=0.0, upload=0.0, device=0.0, distortion=0.0)
    for first in range(0, F, SCORE_CHUNK):
        n = min(SCORE_CHUNK, F - first)
        t0 = time.perf_counter()
        table, bs, _, ms = sess.video_distortion(first, n, test[first:first + n, ..., ::-1], law, block=distortion["block"], gate=distortion["gate"],
                                                 ref=None if ref is None else ref[first:first + n, ..., ::-1], size=(H0, W0))       # the kernel takes cv2's BGR order
        t["gpu"] += (time.perf_counter() - t0) * 1e3
        for k in ("upload", "device", "distortion"):
            t[k] += ms[k]
        tables.append(table)
        blocks.append(bs)
    table = np.concatenate(tables)
    files = [name + "_distortion.npy", name + "_distortion.csv"]
    np.save(os.path.join(out_dir, files[0]), table)
    if distortion["block"]:
        files.append(name + "_block_sse.npy")
        np.save(os.path.join(out_dir, files[-1]), np.concatenate(blocks))
    rep = dataflow.distortion_report(table, H0 * W0)
    with open(os.path.join(out_dir, files[1]), "w") as f:
        f.write("frame," + ",".join(["psnr_" + c for c in DISTORTION_PLANES] + ["wpsnr_" + c for c in DISTORTION_PLANES]) +
                ",ssim,wssim,changed_salient_share\n")
        for k in range(F):
            row = list(rep["psnr"][k]) + list(rep["wpsnr"][k]) + [rep["ssim"][k], rep["wssim"][k], rep["changed_salient_share"][k]]
            f.write("%d,%s\n" % (k + 1, ",".join(repr(float(v)) for v in row)))
    t.update(report=rep, files=files)
    return t


def format_distortion_means(rep):
    """The video's means of the Y plane's figures; frames without a figure (NaN) and frames equal to their reference (+inf) aside."""
    def mean(v):
        v = v[np.isfinite(v)]
        return float(v.mean()) if v.size else float("nan")
    return "psnr_y %.4f wpsnr_y %.4f ssim %.6f wssim %.6f changed_salient_share %.6f" % (
        mean(rep["psnr"][:, 3]), mean(rep["wpsnr"][:, 3]), mean(rep["ssim"]), mean(rep["wssim"]), mean(rep["changed_salient_share"]))


def write_qp_text(path, qp):
    """qp.txt: one line a frame -- the frame's number from 1, then its offsets in raster order, separated by spaces."""
    with open(path, "w") as f:
        for k, q in enumerate(qp):
            f.write("%d %s\n" % (k + 1, " ".join("%d" % v for v in q.ravel())))


def qpmap_video_resident(sess, F, video_dir, size, qpmap):
    """--qpmap: the open video's maps at `size` turned into quantiser offsets per coding block on the device (P3DSession.video_qpmap),
    ONE call for the whole video so that the limiter sees every frame; writes qp.npy, stats.npy, qp.txt and, on request, levels.npy
    into video_dir.  -> dict(gpu, device, qpmap: ms; grid: (Hb, Wb); lo, hi: the smallest and largest offset written)."""
    from sap3d_tensorflow_amd import dataflow
    law = dataflow.qp_law(qpmap["lo"], qpmap["hi"], qpmap["gate"], qpmap["gamma"])
    t0 = time.perf_counter()
    res = sess.video_qpmap(0, F, size, law, block=qpmap["block"], peak_weight=qpmap["peak_weight"], dilate=qpmap["dilate"], fall=qpmap["fall"],
                           rise=qpmap["rise"], balance=qpmap["balance"], target=min(max(0, qpmap["lo"]), qpmap["hi"]), lo=qpmap["lo"],
                           hi=qpmap["hi"], with_levels=qpmap["levels"], with_stats=True, timed=True)
    t = dict(gpu=(time.perf_counter() - t0) * 1e3, device=sess.last_qpmap_ms["device"], qpmap=sess.last_qpmap_ms["qpmap"],
             grid=res["qp"].shape[1:], lo=int(res["stats"][:, 0].min()), hi=int(res["stats"][:, 1].max()))
    np.save(os.path.join(video_dir, "qp.npy"), res["qp"])
    np.save(os.path.join(video_dir, "stats.npy"), res["stats"])
    if qpmap["levels"]:
        np.save(os.path.join(video_dir, "levels.npy"), res["levels"])
    write_qp_text(os.path.join(video_dir, "qp.txt"), res["qp"])
    return t


def reframe_args(args, error):
    """Checks --reframe and its values as P3DSession.video_reframe would refuse them, before anything runs; error(message) does not
    return.  Leaves dict(size or aspect, gate, smooth) in args.reframe_kw (None without --reframe)."""
    args.reframe_kw = None
    shaped = args.reframe_size is not None or args.reframe_aspect or args.reframe_gate != 0 or args.reframe_smooth != 0
    if not args.reframe:
        if shaped:
            error("--reframe-size / -aspect / -gate / -smooth need --reframe DIR")
        return
    if not args.resident:
        error("--reframe needs --resident: the frames and the maps stay on the device")
    if args.reframe_size is not None and args.reframe_aspect:
        error("--reframe-size and --reframe-aspect both set the window: give one")
    kw = dict(size=None, aspect=None, gate=args.reframe_gate, smooth=args.reframe_smooth)
    if args.reframe_size is not None:
        if min(args.reframe_size) < 1:
            error("--reframe-size is HC WC, each at least 1")
        kw["size"] = tuple(args.reframe_size)
    else:
        try:
            a, b = (int(v) for v in (args.reframe_aspect or "9:16").split(":"))
        except ValueError:
            a = b = 0
        if a < 1 or b < 1:
            error("--reframe-aspect is A:B, two positive integers (width : height)")
        kw["aspect"] = (a, b)
    if not 0 <= args.reframe_gate <= 255:
        error("--reframe-gate is a level, 0 .. 255")
    if not 0 <= args.reframe_smooth <= 255:
        error("--reframe-smooth is 0 .. 255 frames")
    args.reframe_kw = kw


def render_args(args, error):
    """Checks --render and its values as P3DSession.video_render would refuse them, before anything runs; error(message) does not
    return.  Leaves the keyword arguments of video_render in args.render_kw (None without --render)."""
    args.render_kw = None
    shaped = (args.render_colormap != "jet" or args.render_alpha != 0.6 or args.render_opacity != "ramp" or args.render_gate != 0 or
              args.render_contour != 0 or args.render_thickness != 1 or args.render_contour_color != "255,255,255")
    if not args.render:
        if shaped:
            error("--render-colormap / -alpha / -opacity / -gate / -contour / -thickness / -contour-color need --render DIR")
        return
    if not args.resident:
        error("--render needs --resident: the frames and the maps stay on the device")
    try:
        color = tuple(int(v) for v in args.render_contour_color.split(","))
    except ValueError:
        color = ()
    if len(color) != 3 or min(color) < 0 or max(color) > 255:
        error("--render-contour-color is R,G,B, three bytes")
    if not 0. <= args.render_alpha <= 1.:
        error("--render-alpha is in [0, 1]")
    if not 0 <= args.render_gate <= 256:
        error("--render-gate is a level, 0 .. 256")
    if not 0 <= args.render_contour <= 255:
        error("--render-contour is a level, 1 .. 255 (0: none)")
    if not 1 <= args.render_thickness <= 4:
        error("--render-thickness is 1 .. 4")
    args.render_kw = dict(colormap=args.render_colormap, alpha=args.render_alpha, opacity=args.render_opacity, gate=args.render_gate,
                          contour=args.render_contour or None, thickness=args.render_thickness, contour_color=color)


TEMPORAL_MAX_RADIUS = 24


def temporal_args(args, error):
    """Checks --temporal and its values as P3DSession.set_video_temporal would refuse them, before anything runs; error(message)
    does not return."""
    import math
    s, r, a = args.temporal_sigma, args.temporal_radius, args.temporal_alpha
    if args.temporal == "off":
        if s != 0. or r != 0 or a != 0.:
            error("--temporal-sigma / --temporal-radius / --temporal-alpha need --temporal gauss or ema")
    elif args.temporal == "gauss":
        if a != 0.:
            error("--temporal-alpha belongs to --temporal ema")
        if not (math.isfinite(s) and s > 0.):
            error("--temporal gauss needs --temporal-sigma S with S > 0")
        if not 0 <= r <= TEMPORAL_MAX_RADIUS:
            error("--temporal-radius must be in 0..%d" % TEMPORAL_MAX_RADIUS)
        if r == 0:
            k = round(8. * float(np.float32(s)) + 1.)               # (rint: round half to even, as Python's round)
            if k > 2 * TEMPORAL_MAX_RADIUS + 1:
                error("--temporal-sigma %g asks for a radius above %d; give --temporal-radius" % (s, TEMPORAL_MAX_RADIUS))
            if (int(k) | 1) // 2 < 1:
                error("--temporal-sigma %g asks for radius 0; give --temporal-radius" % s)
    else:
        if s != 0. or r != 0:
            error("--temporal-sigma / --temporal-radius belong to --temporal gauss")
        if not (math.isfinite(a) and 0. <= a < 1.):
            error("--temporal-alpha must be in [0, 1)")


def prior_stage_args(args):
    """(file, mode, weight) of --prior, or None without it.  Exits on flags that cannot be served, before anything runs."""
    if not args.prior:
        if args.prior_mode != "mul" or args.prior_weight != 0.:
            raise SystemExit("--prior-mode / --prior-weight need --prior FILE.npy")
        return None
    if args.write == "npy" and not args.truth:
        raise SystemExit("--prior shapes the images: it needs --write png or jpg (npy stays the raw 112x112 maps)")
    if not 0. <= args.prior_weight <= 1.:
        raise SystemExit("--prior-weight: the weight must be in [0, 1]")
    return args.prior, args.prior_mode, float(args.prior_weight)


def load_prior(path, size):
    """--prior's map: float32 [H, W] of an .npy, of the images' size."""
    g = np.asarray(np.load(path), np.float32)
    if g.shape != tuple(size):
        raise ValueError("--prior: the map %s is %s, the images are %s" % (path, g.shape, tuple(size)))
    return g


def match_target(args):
    """What --match-hist asks for, as P3DSession.set_hist_match takes it: "off", or the table of an .npz."""
    if not args.match_hist:
        return "off"
    from sap3d_tensorflow_amd import dataflow
    return dataflow.load_match_table(args.match_hist)


def run(sess, args):
    os.makedirs(args.out, exist_ok=True)
    video_means = []
    args.auc_means = []
    for path in sorted(glob.glob(os.path.join(args.videos, "*.npy"))):
        if args.resident:
            means = run_resident(sess, args, path)
            if means is not None:
                video_means.append(means)
            continue
        if args.write == "npy":
            t0 = time.perf_counter()
            sal = predict_video(sess, preprocess(np.load(path)), args.batch)
            np.save(os.path.join(args.out, os.path.basename(path)), sal)
            print(os.path.basename(path), sal.shape, float(sal.mean()))
            if args.time:
                print("  %s: wall %.1f ms" % (os.path.basename(path), (time.perf_counter() - t0) * 1e3))
            continue
        name = os.path.splitext(os.path.basename(path))[0]
        video_dir = os.path.join(args.out, name)
        if os.path.exists(video_dir):                 # gen_pred.py:83-86: a video already written is skipped
            print(name, "skipped: %s exists" % video_dir)
            continue
        os.mkdir(video_dir)
        t0 = time.perf_counter()
        t = write_video_images(sess, preprocess(np.load(path)), args.batch, video_dir, args.write, size=tuple(args.size),
                               writers=args.writers)
        wall = (time.perf_counter() - t0) * 1e3
        print(name, "%d %s files in %s" % (t["files"], args.write, video_dir))
        if args.time:
            print("  %s: wall %.1f ms | forward + maps %.1f ms (device resize/quantise %.2f ms, d2h %.2f ms) | encode %.1f ms "
                  "thread time on %d writers" % (name, wall, t["gpu"], t["device"], t["d2h"], t["encode"], args.writers))


    if args.truth and video_means:
        print("mean over %d videos: %s" % (len(video_means), format_means(nan_means(np.stack(video_means)))))
    if args.truth and args.auc_means:
        print("auc mean over %d videos: %s" % (len(args.auc_means), format_auc(auc_means(np.stack(args.auc_means)))))


def run_resident(sess, args, path):
    """One video of run() on the resident path.  -> the video's column means under --truth, else None."""
    name = os.path.splitext(os.path.basename(path))[0]
    video_dir = os.path.join(args.out, name)
    if args.write != "npy":
        if os.path.exists(video_dir):                 # gen_pred.py:83-86: a video already written is skipped
            print(name, "skipped: %s exists" % video_dir)
            return
        os.mkdir(video_dir)
    render_dir = os.path.join(args.render, name) if args.render else None
    if render_dir:
        os.makedirs(render_dir, exist_ok=True)
    t0 = time.perf_counter()
    times = {}
    reframe_dir = os.path.join(args.reframe, name) if args.reframe else None
    if reframe_dir:
        os.makedirs(reframe_dir, exist_ok=True)
    detect = bool(args.shots_kw and args.shots_kw["detect"])
    prefilter_dir = os.path.join(args.prefilter, name) if args.prefilter else None
    if prefilter_dir:
        os.makedirs(prefilter_dir, exist_ok=True)
    keep = bool(render_dir or reframe_dir or detect or prefilter_dir or (args.distortion_kw and not args.distortion_kw["ref"]))
    if args.shot_windows:      # the table goes in before the windows are cut, and they stay inside its shots
        F = predict_video_resident(sess, np.load(path), args.batch, args.stride, args.overlap, times, keep_source=keep,
                                   shot_windows=lambda F: shots_video_resident(sess, F, args.out, name, args.shots_kw))
        starts = sess.video_shots()
    else:
        F = predict_video_resident(sess, np.load(path), args.batch, args.stride, args.overlap, times, keep_source=keep)
        starts = shots_video_resident(sess, F, args.out, name, args.shots_kw) if args.shots_kw else None
    if args.shots_kw:
        print(name, "%d shots, starting at frames %s%s" % (len(starts), " ".join(str(int(v)) for v in starts[:12]), " ..." if len(starts) > 12 else ""))
    t1 = time.perf_counter()
    means = ts = None
    if args.truth:
        density, fixation = load_truth(args.truth, name, F, args.size)
        auc = None
        if args.score_auc:
            auc = dict(borji=args.score_borji, sauc=args.score_sauc, pool_size=0, own_pool=not args.sauc_pool, n_rep=args.score_rep,
                       step=args.score_step, seed=args.score_seed)
        if args.score_sauc:
            pool_maps = fixation
            if args.sauc_pool:
                pool_maps = np.load(args.sauc_pool)
                if pool_maps.dtype != np.uint8 or pool_maps.ndim != 3 or pool_maps.shape[1:] != tuple(args.size):
                    raise ValueError("--sauc-pool: %s is %s %s, not uint8 [P, %d, %d]" % ((args.sauc_pool, pool_maps.dtype, pool_maps.shape) + tuple(args.size)))
            elif F < 2:
                raise ValueError("--score-sauc: a video of one frame has no other frame to draw from; give --sauc-pool")
            auc["pool_size"] = len(pool_maps)
            sess.open_fixation_pool(tuple(args.size), len(pool_maps))
            sess.fixation_pool_put(0, pool_maps)
        scores, auc, ts = score_video_resident(sess, F, density, fixation, tuple(args.size), tuple(args.score_columns), args.score_ties, auc,
                                               video_dir if args.write != "npy" else None, args.write, args.writers)
        if args.score_sauc:
            sess.close_fixation_pool()
        np.save(os.path.join(args.out, name + "_scores.npy"), scores)
        if auc is not None:
            np.save(os.path.join(args.out, name + "_auc.npy"), auc)
        means = nan_means(scores)
        print("%s scores over %d frames: %s" % (name, F, format_means(means)))
        if auc is not None:
            print("%s auc over %d frames: %s" % (name, F, format_auc(auc_means(auc))))
            args.auc_means.append(auc_means(auc))
    if args.write == "npy":
        sal = sess.video_maps(0, F)
        np.save(os.path.join(args.out, os.path.basename(path)), sal)
        print(os.path.basename(path), sal.shape, float(sal.mean()))
    elif ts is not None:
        t = dict(gpu=ts["upload"] + ts["device"] + ts["score"], device=ts["device"], d2h=0.0, encode=0.0, files=ts["files"])
        print(name, "%d %s files in %s" % (t["files"], args.write, video_dir))
    else:
        t = write_video_images_resident(sess, F, video_dir, args.write, size=tuple(args.size), writers=args.writers)
        print(name, "%d %s files in %s" % (t["files"], args.write, video_dir))
    tr = None
    if render_dir:
        tr = render_video_resident(sess, F, render_dir, args.render_kw, writers=args.writers)
        print(name, "%d rendered png files in %s" % (tr["files"], render_dir))
    tf = None
    if reframe_dir:
        tf = reframe_video_resident(sess, F, reframe_dir, args.reframe_kw, writers=args.writers)
        print(name, "%d reframed %d x %d png files and track.npy in %s" % ((tf["files"],) + tf["window"] + (reframe_dir,)))
    tg = None
    if args.regions_kw:
        regions_dir = os.path.join(args.regions, name)
        os.makedirs(regions_dir, exist_ok=True)
        tg = regions_video_resident(sess, F, regions_dir, tuple(args.size), args.regions_kw)
        print(name, "%d regions over %d frames: regions.npy, counts.npy%s in %s" % (tg["kept"], F, ", labels.npy" if args.regions_kw["labels"] else "", regions_dir))
    tq = None
    if args.qpmap_kw:
        qpmap_dir = os.path.join(args.qpmap, name)
        os.makedirs(qpmap_dir, exist_ok=True)
        tq = qpmap_video_resident(sess, F, qpmap_dir, tuple(args.size), args.qpmap_kw)
        print(name, "%d x %d offsets in [%d, %d] over %d frames: qp.npy, stats.npy, qp.txt%s in %s"
              % (tq["grid"] + (tq["lo"], tq["hi"], F, ", levels.npy" if args.qpmap_kw["levels"] else "", qpmap_dir)))
    tp = None
    if prefilter_dir:
        tp = prefilter_video_resident(sess, F, prefilter_dir, args.prefilter_kw, writers=args.writers)
        print(name, "%d pre-filtered png files and grid.npy in %s, mean strength %.4f" % (tp["files"], prefilter_dir, tp["strength"]))
    td = None
    if args.distortion_kw:
        td = distortion_video_resident(sess, F, args.out, name, args.distortion, args.distortion_kw)
        print(name, "distortion over %d frames: %s; %s in %s" % (F, format_distortion_means(td["report"]), ", ".join(td["files"]), args.out))
    temporal_ms = sess.video_temporal_last_ms() if args.temporal != "off" and args.time else None
    sess.close_video()
    if args.time:
        print("  %s: wall %.1f ms | resident, stride %d%s, overlap %s: %d forward passes in %.1f ms (window cuts %.3f ms, map folds %.3f ms "
              "on the device)" % (os.path.basename(path), (time.perf_counter() - t0) * 1e3, args.stride, " inside the shots" if args.shot_windows else "",
                                  args.overlap, times["batches"], (t1 - t0) * 1e3, times["gather"], times["scatter"]))
        if temporal_ms is not None:
            print("  %s: temporal %s: %.3f ms on the device in the last read-out" % (name, args.temporal, temporal_ms))
        if ts is not None:
            print("  %s: scoring: uploads %.2f ms, maps %.2f ms, scoring launches %.3f ms on the device" % (name, ts["upload"], ts["device"], ts["score"]))
            if "auc" in ts:
                print("  %s: scoring: select + sweeps %.3f ms on the device" % (name, ts["auc"]))
        if args.write != "npy" and ts is None:
            print("  %s: maps %.1f ms (device resize/quantise %.2f ms, d2h %.2f ms) | encode %.1f ms thread time on %d writers"
                  % (name, t["gpu"], t["device"], t["d2h"], t["encode"], args.writers))
        if tr is not None:
            print("  %s: render %.1f ms (uploads %.2f ms, maps %.2f ms, render launches %.3f ms on the device) | encode %.1f ms thread "
                  "time on %d writers" % (name, tr["gpu"], tr["upload"], tr["device"], tr["render"], tr["encode"], args.writers))
        if tf is not None:
            print("  %s: reframe %.1f ms (uploads %.2f ms, maps %.2f ms, reframe launches %.3f ms on the device) | encode %.1f ms thread "
                  "time on %d writers" % (name, tf["gpu"], tf["upload"], tf["device"], tf["reframe"], tf["encode"], args.writers))
        if tg is not None:
            print("  %s: regions %.1f ms (maps %.2f ms, regions launches %.3f ms on the device)" % (name, tg["gpu"], tg["device"], tg["regions"]))
        if tq is not None:
            print("  %s: qpmap %.1f ms (maps %.2f ms, qpmap launches %.3f ms on the device)" % (name, tq["gpu"], tq["device"], tq["qpmap"]))
        if tp is not None:
            print("  %s: prefilter %.1f ms (maps %.2f ms, prefilter launches %.3f ms on the device) | encode %.1f ms thread time on %d writers"
                  % (name, tp["gpu"], tp["device"], tp["prefilter"], tp["encode"], args.writers))
        if td is not None:
            print("  %s: distortion %.1f ms (uploads %.2f ms, maps %.2f ms, distortion launches %.3f ms on the device)"
                  % (name, td["gpu"], td["upload"], td["device"], td["distortion"]))
    return means


def main(argv=None):
    args = parse_args(argv)
    stage = prior_stage_args(args)                                          # refused before anything runs
    prior = load_prior(stage[0], args.size) if stage else None
    from sap3d_tensorflow_amd import P3DSession
    blocks = tuple(int(v) for v in args.blocks.split(","))
    sess = P3DSession(args.structure, batch=args.batch, device=int(args.gpu), seed=0, base=args.base, blocks=blocks)
    if args.model:
        sess.restore(args.model, ema_as_weights=args.ema)
    sess.set_postprocess(args.blur_sigma, args.blur_radius, args.normalize)
    sess.set_hist_match(match_target(args), args.match_bins)
    sess.set_video_temporal(args.temporal, args.temporal_sigma, args.temporal_radius, args.temporal_alpha)
    if stage:
        sess.set_prior_map(prior)
        sess.set_prior_stage(stage[1], stage[2])
    run(sess, args)
    sess.close()


if __name__ == "__main__":
    main()
