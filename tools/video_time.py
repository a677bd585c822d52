"""Wall time per video of drivers/gen_pred.py's two inference paths in one process, at the reference geometry (unet++ds,
16x112x112, batch 8) on a synthetic 200-frame 360x640 uint8 video (profiles/r17_video_time.json):
  host      preprocess (frames normalised on the device, copied back) + predict_video (windows stacked on the host, uploaded,
            every map downloaded);
  resident  predict_video_resident + video_maps (frames up once as uint8, windows cut on the device, maps read once),
            with the HIP-event time of the window cuts and map folds per batch (P3DSession.video_last_ms).
The two alternate, PASSES times each, after one warm-up of both; medians.  Then the resident path at stride 1, 4 and 16, newest and
mean.  Every timed region ends in a device-to-host copy that waits for the stream.  A report: nothing is asserted but that host
and resident agree bit for bit at stride 1."""
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sap3d_tensorflow_amd import P3DSession      # noqa: E402

F, H0, W0, BATCH, PASSES = 200, 360, 640, 8, 5


def gen_pred():
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


def median(v):
    return float(np.median(np.asarray(v)))


def main():
    small = "--small" in sys.argv      # a rehearsal size: the figures mean nothing
    gp = gen_pred()
    frames = 24 if small else F
    video = np.random.default_rng(0).integers(0, 256, (frames, H0, W0, 3)).astype(np.uint8)
    sess = P3DSession("unet++ds", batch=BATCH, seed=0, **(dict(base=16, blocks=(1, 1, 1)) if small else {}))

    def host():
        t0 = time.perf_counter()
        sal = gp.predict_video(sess, gp.preprocess(video), BATCH)
        return (time.perf_counter() - t0) * 1e3, sal, None

    def resident(stride=1, overlap="newest"):
        t0 = time.perf_counter()
        times = {}
        n = gp.predict_video_resident(sess, video, BATCH, stride, overlap, times)
        sal = sess.video_maps(0, n)
        ms = (time.perf_counter() - t0) * 1e3
        sess.close_video()
        return ms, sal, times

    _, a, _ = host()
    _, b, _ = resident()
    same = bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
    wall = {"host": [], "resident": []}
    cuts = []
    for _ in range(PASSES):
        wall["host"].append(host()[0])
        ms, _, t = resident()
        wall["resident"].append(ms)
        cuts.append((t["gather"] / t["batches"], t["scatter"] / t["batches"]))
    out = {"tool": "tools/video_time.py", "structure": "unet++ds", "batch": BATCH, "frames": frames, "frame_size": [H0, W0], "passes": PASSES,
           "stride1_resident_equals_host_bit_for_bit": same,
           "host_wall_ms": round(median(wall["host"]), 2), "host_wall_ms_all": [round(v, 2) for v in wall["host"]],
           "resident_wall_ms": round(median(wall["resident"]), 2), "resident_wall_ms_all": [round(v, 2) for v in wall["resident"]],
           "resident_gather_ms_per_batch": round(median([c[0] for c in cuts]), 4),
           "resident_scatter_ms_per_batch": round(median([c[1] for c in cuts]), 4),
           "host_gather_scatter_ms_per_batch": None,      # the host path cuts and keeps its windows in numpy: no device launches to time
           "strides": []}
    for stride in (1, 4, 16):
        for overlap in ("newest", "mean"):
            runs = [resident(stride, overlap) for _ in range(PASSES)]
            t = runs[-1][2]
            row = {"stride": stride, "overlap": overlap, "forward_passes": t["batches"], "wall_ms": round(median([r[0] for r in runs]), 2),
                   "gather_ms_per_batch": round(median([r[2]["gather"] / r[2]["batches"] for r in runs]), 4),
                   "scatter_ms_per_batch": round(median([r[2]["scatter"] / r[2]["batches"] for r in runs]), 4)}
            print(json.dumps(row), flush=True)
            out["strides"].append(row)
    sess.close()
    print(json.dumps(out))
    if not same:
        raise SystemExit("the resident path at stride 1 differs from the host path")


if __name__ == "__main__":
    main()
