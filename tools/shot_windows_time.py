"""Device time of the slot gather of p3d_video_predict_shots (csrc/video.hip, video_gather_slots_kernel) beside the contiguous
video_gather_kernel of p3d_video_predict, on the same windows of the same resident video: batch 8 at 112 x 112, 64 frames, a table of
one shot, stride 1 (49 windows: six full calls and one of a single window, whose seven padding clips repeat it).  Both kernels move the
same bytes.  The two paths alternate, REPS rounds after one warm-up round; per call p3d_video_last_ms gives the HIP-event time of the
gather and of the scatter, and a host clock around the synchronised call the time of the whole call, forward pass included.  Writes
profiles/shot_windows_gather.json (--out): per path and per call position the median and the extremes over the rounds.  A report:
nothing is asserted but that both paths leave the same maps."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sap3d_tensorflow_amd import P3DSession, dataflow      # noqa: E402

F, BATCH, SIZE, T, REPS = 64, 8, 112, 16, 10


def stats(ms):
    ms = np.asarray(ms, np.float64)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shot_windows_gather.json"))
    ap.add_argument("--structure", default="unet")
    ap.add_argument("--reps", type=int, default=REPS)
    a = ap.parse_args()
    sess = P3DSession(a.structure, batch=BATCH, frames=T, height=SIZE, width=SIZE, seed=1)
    frames = np.random.default_rng(0).normal(0.0, 0.5, (F, SIZE, SIZE, 3)).astype(np.float32)
    starts = dataflow.shot_window_starts([0], F, 1, T)
    calls = [starts[i:i + BATCH] for i in range(0, len(starts), BATCH)]
    rows = {"video_predict": [], "video_predict_shots": []}
    maps = {}
    for rep in range(a.reps + 1):
        for path in rows:
            sess.open_video(F, "newest")
            sess.video_put(0, frames)
            sess.video_set_shots([0])
            predict = sess.video_predict if path == "video_predict" else sess.video_predict_shots
            one = []
            for chunk in calls:
                t0 = time.perf_counter()
                predict(chunk)
                wall = (time.perf_counter() - t0) * 1e3
                ms = sess.video_last_ms()
                one.append((ms["gather"], ms["scatter"], wall))
            maps[path] = sess.video_maps(0, F)
            if rep:
                rows[path].append(one)
    assert np.array_equal(maps["video_predict"].view(np.uint32), maps["video_predict_shots"].view(np.uint32))
    sess.close_video()
    sess.close()
    nbytes = BATCH * T * SIZE * SIZE * 3 * 8      # read and written, a call
    out = dict(tool="tools/shot_windows_time.py", structure=a.structure, batch=BATCH, frames=F, size=SIZE, stride=1, reps=a.reps,
               windows_per_call=[len(c) for c in calls], gather_bytes_per_call=nbytes,
               note="gather, scatter: HIP events round the launch (p3d_video_last_ms); call: host clock round the synchronised call, "
                    "the table uploads and the forward pass included", paths={})
    for path, reps in rows.items():
        r = np.asarray(reps, np.float64)      # [reps, calls, 3]
        g = r[:, :, 0]
        out["paths"][path] = dict(gather=stats(g.ravel()), gather_gb_per_s=nbytes / float(np.median(g)) / 1e6, scatter=stats(r[:, :, 1].ravel()),
                                  call=stats(r[:, :, 2].ravel()), gather_per_call_position=[stats(g[:, i]) for i in range(g.shape[1])],
                                  gather_spread_between_rounds_ms=float(np.median(g, axis=1).max() - np.median(g, axis=1).min()))
        print(path, json.dumps(out["paths"][path]), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
