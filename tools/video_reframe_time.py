"""Device time of reframing a resident video around its saliency (P3DSession.video_reframe): 64 frames at 1080 x 960, the frames
kept on the device as they were put (video_keep_source), a 1080 x 608 window (9:16 of the frame's height: one row of 353 positions)
and a 540 x 480 one (541 x 481 positions), the track smoothed over 12 frames to either side; beside it video_render's stage on the
same frames, the nearest launch that existed before: it too reads the maps and reads and writes frame bytes.  Writes
profiles/reframe_stage_ms.json (--out): per window the HIP-event times of one call (last_reframe_ms: the upload, the maps' chain,
the reframe launches together), the median of REPS calls after WARM warm-up calls, and the plan of the launches.
--trace-only runs WARM + REPS calls a window for `rocprofv3 --kernel-trace --stats` in a run of its own; --kernel-stats FILE.csv
adds each reframe kernel's calls and average from that run's statistics (both windows together).  The maps' values matter little
to the time, so the network is a small one (unet, base 16, one block per stage).  A report: nothing is asserted but that the
device's track equals dataflow.reframe_track's on the same bytes."""
import argparse
import csv
import importlib.util
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sap3d_tensorflow_amd import P3DSession, dataflow      # noqa: E402

F, SIZE, BATCH, STRIDE, WARM, REPS, SMOOTH = 64, (1080, 960), 8, 8, 3, 20, 12
WINDOWS = [("1080x608: one row of positions", (1080, 608)), ("540x480: many positions", (540, 480))]


def gen_pred():
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


def kernel_stats(path):
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            m = re.search(r"reframe_\w+|render_kernel<[^>]*>", row.get("Name", ""))
            if m:
                rows.append({"kernel": m.group(0), "calls": int(row["Calls"]), "average_ms": round(float(row["AverageNs"]) * 1e-6, 4),
                             "min_ms": round(float(row["MinNs"]) * 1e-6, 4), "max_ms": round(float(row["MaxNs"]) * 1e-6, 4)})
    if not rows:
        raise SystemExit("%s has no row of a reframe kernel" % path)
    return rows


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--small", action="store_true", help="a rehearsal size: the figures mean nothing")
    p.add_argument("--trace-only", action="store_true", help="only the calls, for a kernel trace")
    p.add_argument("--kernel-stats", default="", metavar="FILE.csv", help="the kernel statistics of a --trace-only run under rocprofv3")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "reframe_stage_ms.json"))
    args = p.parse_args()
    frames, size, reps, windows = (16, (90, 80), 2, [("a", (90, 50)), ("b", (44, 40))]) if args.small else (F, SIZE, REPS, WINDOWS)
    gp = gen_pred()
    video = np.random.default_rng(0).integers(0, 256, (frames,) + size + (3,), dtype=np.uint8)      # R, G, B as the driver reads it
    sess = P3DSession("unet", batch=BATCH, seed=0, base=16, blocks=(1, 1, 1))
    sess.set_postprocess(0., 0, "range")            # an untrained net's maps are flat: stretch them
    gp.predict_video_resident(sess, video, BATCH, STRIDE, "newest", keep_source=True)
    out = {"tool": "tools/video_reframe_time.py", "frames": frames, "size": list(size), "smooth": SMOOTH, "warm": WARM, "reps": reps,
           "source": sess.video_source_info(), "reframe": [], "render": None}
    for name, crop in windows:
        ms = {"upload": [], "device": [], "reframe": []}
        res = None
        for i in range(WARM + reps):
            res = sess.video_reframe(0, frames, crop, smooth=SMOOTH, with_raw=True, with_mass=True, with_maps=(i == 0), timed=True)
            if i == 0:
                maps = res["maps"]
            if i >= WARM:
                for k in ms:
                    ms[k].append(sess.last_reframe_ms[k])
        if args.trace_only:
            continue
        row = {"window": name, "crop": list(crop), "positions": (size[0] - crop[0] + 1) * (size[1] - crop[1] + 1),
               "plan": dataflow.reframe_plan(size[0], size[1], crop, frames)}
        for k in ms:
            row[k + "_median_ms"] = round(float(np.median(ms[k])), 4)
        row["reframe_min_ms"], row["reframe_max_ms"] = round(min(ms["reframe"]), 4), round(max(ms["reframe"]), 4)
        want = dataflow.reframe_track(maps, crop, smooth=SMOOTH)
        if not (np.array_equal(res["track"], want[0]) and np.array_equal(res["raw"], want[1]) and np.array_equal(res["mass"], want[2])):
            raise SystemExit("the device's track differs from the host statement of the law")
        row["distinct_raw_positions"] = int(len(np.unique(res["raw"], axis=0)))
        print(json.dumps(row), flush=True)
        out["reframe"].append(row)
    table = dataflow.render_table("jet", 0.6, "ramp")
    ms = {"upload": [], "device": [], "render": []}
    for i in range(WARM + reps):
        sess.video_render(0, frames, table=table, timed=True)
        if i >= WARM:
            for k in ms:
                ms[k].append(sess.last_render_ms[k])
    sess.close_video()
    sess.close()
    if args.trace_only:
        return
    out["render"] = {"what": "video_render on the same frames and kept source, no contour: one launch, 7 bytes a pixel"}
    for k in ms:
        out["render"][k + "_median_ms"] = round(float(np.median(ms[k])), 4)
    out["render"]["render_min_ms"], out["render"]["render_max_ms"] = round(min(ms["render"]), 4), round(max(ms["render"]), 4)
    if args.kernel_stats:
        out["kernels"] = {"source": "rocprofv3 --kernel-trace --stats of a --trace-only run: both windows, %d calls each" % (WARM + reps),
                          "rows": kernel_stats(args.kernel_stats)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
