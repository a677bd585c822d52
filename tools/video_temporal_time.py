"""Device time of the temporal stage of a resident video's read-out (P3DSession.set_video_temporal) at the workload's own size:
16x112x112 windows, a video of F = 300 frames, mode "mean" at stride 4, the full read video_maps(0, F).  Writes
profiles/video_temporal.json (--out):
  temporal   for GAUSS r = 4, GAUSS r = 24 and EMA: the HIP-event time of the temporal launch (P3DSession.video_temporal_last_ms),
             the median of REPS reads after WARM warm-up reads, with the bytes its launch description claims
             (dataflow.temporal_desc) and the GB/s that follow;
  off_read   the cost of the same read with the stage off, video_mean_kernel touching every map once.  The stage off issues no
             timed launch, so this comes from a kernel trace of `--off-only` (REPS + WARM reads and nothing else, which also runs
             on a commit from before the stage): rocprofv3 --kernel-trace -d DIR -o off -- python tools/video_temporal_time.py
             --off-only, its DIR/.../off_kernel_trace.csv given here as --off-trace.
The maps' values do not matter to the time, so the network is a small one (unet, base 16, one block per stage).  A report:
nothing is asserted but that a filtered read differs from the unfiltered one."""
import argparse
import csv
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sap3d_tensorflow_amd import P3DSession      # noqa: E402

F, H0, W0, BATCH, STRIDE, WARM, REPS = 300, 120, 160, 8, 4, 5, 50
SETTINGS = [("gauss_r4", dict(kind="gauss", sigma=1.5, radius=4)), ("gauss_r24", dict(kind="gauss", sigma=8.0, radius=24)),
            ("ema", dict(kind="ema", alpha=0.75))]


def gen_pred():
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


def mean_kernel_us(trace_csv, warm):
    """Durations (microseconds) of video_mean_kernel's launches in a rocprofv3 kernel trace, the first `warm` dropped."""
    with open(trace_csv, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "video_mean_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows][warm:]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--small", action="store_true", help="a rehearsal size: the figures mean nothing")
    p.add_argument("--off-only", action="store_true", help="only the reads with the stage off, for a kernel trace")
    p.add_argument("--off-trace", default="", metavar="CSV", help="rocprofv3's kernel trace of an --off-only run")
    p.add_argument("--off-commit", default="", help="the commit the --off-only run was made on, recorded with its figures")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_temporal.json"))
    args = p.parse_args()
    frames, reps = (40, 3) if args.small else (F, REPS)
    gp = gen_pred()
    video = np.random.default_rng(0).integers(0, 256, (frames, H0, W0, 3)).astype(np.uint8)
    sess = P3DSession("unet", batch=BATCH, seed=0, base=16, blocks=(1, 1, 1))
    gp.predict_video_resident(sess, video, BATCH, STRIDE, "mean")
    hw = 112 * 112
    if args.off_only:
        for _ in range(WARM + reps):
            sess.video_maps(0, frames)
        sess.close_video()
        sess.close()
        return
    from sap3d_tensorflow_amd import dataflow
    off = sess.video_maps(0, frames)
    out = {"tool": "tools/video_temporal_time.py", "frames": frames, "map": [112, 112], "mode": "mean", "stride": STRIDE,
           "read": [0, frames], "warm": WARM, "reps": reps, "temporal": [], "off_read": None}
    for name, setting in SETTINGS:
        sess.set_video_temporal(**setting)
        ms = []
        for i in range(WARM + reps):
            on = sess.video_maps(0, frames)
            if i >= WARM:
                ms.append(sess.video_temporal_last_ms())
        if np.array_equal(on.view(np.uint32), off.view(np.uint32)):
            raise SystemExit("%s: the filtered read equals the unfiltered one" % name)
        d = dataflow.temporal_desc(F=frames, hw=hw, mode="mean", **setting)
        ppb, fpb, lds = dataflow.temporal_plan(setting["kind"], setting.get("radius", 0), hw, frames)
        med = float(np.median(ms))
        row = {"name": name, "setting": setting, "kernel": d["kernel"], "pixels_per_block": ppb, "frames_per_block": fpb, "lds_bytes": lds,
               "median_us": round(med * 1e3, 2), "min_us": round(min(ms) * 1e3, 2), "max_us": round(max(ms) * 1e3, 2),
               "claimed_bytes": d["bytes"], "gb_per_s": round(d["bytes"] / (med * 1e-3) / 1e9, 1)}
        print(json.dumps(row), flush=True)
        out["temporal"].append(row)
    sess.set_video_temporal("off")
    sess.close_video()
    sess.close()
    if args.off_trace:
        us = mean_kernel_us(args.off_trace, WARM)
        med = float(np.median(us))
        nbytes = frames * hw * 8.0      # p3d_video_mean_desc: every sum read, every map written
        out["off_read"] = {"kernel": "video_mean_kernel", "source": "rocprofv3 --kernel-trace of --off-only", "commit": args.off_commit,
                           "launches": len(us), "median_us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
                           "claimed_bytes": nbytes, "gb_per_s": round(nbytes / (med * 1e-6) / 1e9, 1)}
        for row in out["temporal"]:
            row["times_off_read"] = round(row["median_us"] / med, 2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
