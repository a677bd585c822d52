"""Device time of rendering a resident video's saliency maps over its frames (P3DSession.video_render): 64 frames at 1080 x 1920,
the frames kept on the device as they were put (video_keep_source), beside the route that existed before for the same frames --
video_maps_u8 to the host plus the numpy blend of tests/render_ref.py on those bytes.  Writes profiles/video_render.json (--out):
  render      per variant -- plain, a contour at t = 1 and at t = 4 -- the HIP-event times of one call (last_render_ms: the upload,
              the maps' chain, the render launch), the median of REPS calls after WARM warm-up calls; the launch also as GB/s of
              its 7 bytes a pixel, beside the ≈6300 GB/s a streaming read reaches on this machine;
  heat_map    the launch without frames exists at op level only, which has no events of its own: --trace-only runs WARM + REPS
              op-level calls for `rocprofv3 --kernel-trace --stats`, and --kernel-stats FILE.csv takes the kernel's average from
              that run's statistics (4 bytes a pixel);
  upload      the same plain call with the frames given on the host instead of the kept source: what the source store saves;
  download    wall time of a kept-source call less its three device stages: the copy back of the images, and the host's share;
  host_route  wall time of video_maps_u8 in calls of 16 frames plus render_ref.render on those bytes, 4 frames at a time.
The maps' values matter little to the time, so the network is a small one (unet, base 16, one block per stage).  A report: nothing
is asserted but that both routes render the same bytes."""
import argparse
import csv
import importlib.util
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_ref                                                   # noqa: E402
from sap3d_tensorflow_amd import P3DSession, dataflow      # noqa: E402

F, SIZE, BATCH, STRIDE, WARM, REPS, HOST_REPS = 64, (1080, 1920), 8, 8, 3, 20, 2
STREAM_GB_PER_S = 6300.0
VARIANTS = [("plain", dict()), ("contour t=1", dict(contour=128, thickness=1)), ("contour t=4", dict(contour=128, thickness=4))]


def gen_pred():
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


def rate(pixels, bytes_per_pixel, ms):
    return round(pixels * bytes_per_pixel / (ms * 1e-3) / 1e9, 1)


def heat_from_stats(path, pixels):
    """The average of render_kernel<false, false> out of a rocprofv3 kernel statistics file."""
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if re.search(r"render_kernel<\s*false,\s*false\s*>", row.get("Name", "")):
                ms = float(row["AverageNs"]) * 1e-6
                return {"variant": "heat map (no frames)", "source": "rocprofv3 --kernel-trace --stats, average of %s calls" % row.get("Calls", "?"),
                        "render_average_ms": round(ms, 4), "render_min_ms": round(float(row["MinNs"]) * 1e-6, 4),
                        "render_max_ms": round(float(row["MaxNs"]) * 1e-6, 4), "bytes_per_pixel": 4, "gb_per_s": rate(pixels, 4, ms)}
    raise SystemExit("%s has no row for render_kernel<false, false>" % path)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--small", action="store_true", help="a rehearsal size: the figures mean nothing")
    p.add_argument("--trace-only", action="store_true", help="only op-level heat-map calls, for a kernel trace")
    p.add_argument("--kernel-stats", default="", metavar="FILE.csv", help="the kernel statistics of a --trace-only run under rocprofv3")
    p.add_argument("--no-host", action="store_true", help="skip the host route")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_render.json"))
    args = p.parse_args()
    frames, size, reps = (16, (90, 160), 2) if args.small else (F, SIZE, REPS)
    pixels = frames * size[0] * size[1]
    table = dataflow.render_table("jet", 0.6, "ramp")
    if args.trace_only:
        sal = render_ref.blob(1, *size)[0]
        sal = np.ascontiguousarray(np.broadcast_to(sal, (frames,) + size))
        for _ in range(WARM + reps):
            dataflow.render_overlay(sal, None, table)
        return
    gp = gen_pred()
    video = np.random.default_rng(0).integers(0, 256, (frames,) + size + (3,), dtype=np.uint8)      # R, G, B as the driver reads it
    sess = P3DSession("unet", batch=BATCH, seed=0, base=16, blocks=(1, 1, 1))
    sess.set_postprocess(0., 0, "range")            # an untrained net's maps are flat: stretch them so that level 128 has an edge
    gp.predict_video_resident(sess, video, BATCH, STRIDE, "newest", keep_source=True)
    bgr = video[..., ::-1]
    out = {"tool": "tools/video_render_time.py", "frames": frames, "size": list(size), "warm": WARM, "reps": reps,
           "streaming_read_gb_per_s": STREAM_GB_PER_S, "source": sess.video_source_info(),
           "plan": {"plain": dataflow.render_plan(*size, n=frames), "contour": dataflow.render_plan(*size, n=frames, thickness=1)},
           "render": [], "heat_map": None}
    images = None
    walls = []
    for name, kw in VARIANTS:
        ms = {"upload": [], "device": [], "render": []}
        for i in range(WARM + reps):
            t0 = time.perf_counter()
            images = sess.video_render(0, frames, table=table, timed=True, **kw)
            wall = (time.perf_counter() - t0) * 1e3
            if i >= WARM:
                for k in ms:
                    ms[k].append(sess.last_render_ms[k])
                if name == "plain":
                    walls.append(wall - sum(sess.last_render_ms.values()))
        row = {"variant": name}
        for k in ms:
            row[k + "_median_ms"] = round(float(np.median(ms[k])), 4)
        row["render_min_ms"], row["render_max_ms"] = round(min(ms["render"]), 4), round(max(ms["render"]), 4)
        row["bytes_per_pixel"] = 7
        row["gb_per_s"] = rate(pixels, 7, row["render_median_ms"])
        row["of_streaming_read"] = round(row["gb_per_s"] / STREAM_GB_PER_S, 3)
        print(json.dumps(row), flush=True)
        out["render"].append(row)
    out["download"] = {"what": "wall time of a plain kept-source call less its device stages: the copy back of %d MB of images, pageable" % (pixels * 3 // 2 ** 20),
                       "median_ms": round(float(np.median(walls)), 2)}
    up = []
    for i in range(WARM + reps):
        sess.video_render(0, frames, frames=bgr, table=table, timed=True)
        if i >= WARM:
            up.append(sess.last_render_ms["upload"])
    out["upload"] = {"what": "the frames given on the host (%d MB, pageable) instead of the kept source, which uploads nothing" % (pixels * 3 // 2 ** 20),
                     "median_ms": round(float(np.median(up)), 2)}
    if args.kernel_stats:
        out["heat_map"] = heat_from_stats(args.kernel_stats, pixels)
    wall, maps_ms, blend_ms, host = [], [], [], None
    for _ in range(0 if args.no_host else 1 if args.small else HOST_REPS):
        t0 = time.perf_counter()
        maps = np.concatenate([sess.video_maps_u8(f, min(16, frames - f), size=size) for f in range(0, frames, 16)])
        t1 = time.perf_counter()
        host = np.concatenate([render_ref.render(maps[f:f + 4], bgr[f:f + 4], table, 128, 4) for f in range(0, frames, 4)])
        t2 = time.perf_counter()
        wall.append((t2 - t0) * 1e3)
        maps_ms.append((t1 - t0) * 1e3)
        blend_ms.append((t2 - t1) * 1e3)
    if host is not None:
        out["host_route"] = {"what": "video_maps_u8 in calls of 16 frames + tests/render_ref.py's numpy blend and contour (t = 4) on the bytes; wall time",
                             "reps": len(wall), "median_ms": round(float(np.median(wall)), 1), "maps_u8_median_ms": round(float(np.median(maps_ms)), 1),
                             "render_ref_median_ms": round(float(np.median(blend_ms)), 1)}
        if not np.array_equal(host, images):
            raise SystemExit("the two routes render different bytes")
        out["agreement"] = "the host route's bytes equal the device's (contour t = 4)"
    sess.close_video()
    sess.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
