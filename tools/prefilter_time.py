"""Device time of the pre-filter of a resident video (P3DSession.video_prefilter): 64 frames at 1080 x 1920 from the kept source
(random bytes), blocks of 16, at (radius, passes) = (4, 1), (8, 2) and (16, 3); a blob field planted through the prior stage ("mix",
weight 1: every map IS the prior), so the maps come out of the same chain as a network's.  Per setting: the HIP-event times of the
maps' chain and of the prefilter launches (grid and filter together), the median of REPS calls after WARM warm-up calls; the grid
launches alone, timed as P3DSession.video_qpmap's with the strength grid's configuration (the same launch sequence); the filter
launches as the difference; the plan.  Beside them, in the same process, a device-to-device copy of the same n * H * W * 3 bytes
(dataflow.shots_time's third column), which reads and writes exactly what the filter must: the filter's frame bytes per second are
reported as a share of the copy's, and held against nothing else.  A second map, 255 in the left half and 0 in the right, shows what
the tile skipping buys.  Writes profiles/prefilter_time.json (--out).  --only R,P runs one setting alone, for `rocprofv3
--kernel-trace --stats`.  A report: nothing is asserted but that the device's frames equal the replay's on a window of the first
frame."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prefilter_ref as pr                                  # noqa: E402
import qpmap_ref as qr                                      # noqa: E402
from sap3d_tensorflow_amd import P3DSession, dataflow      # noqa: E402

F, SIZE, BATCH, STRIDE, WARM, REPS, BLOCK = 64, (1080, 1920), 8, 8, 2, 10, 16
SETTINGS = ((4, 1), (8, 2), (16, 3))
GRID = dict(peak_weight=128, dilate=1, fall=2, rise=4)


def gen_pred():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


def check_window(out, maps, video, law, R, P, y0, rows=24):
    """The first frame's rows y0 .. y0 + rows - 1 against the replay: grid and weights whole, the low-pass with a margin of R P rows."""
    H, W = maps.shape[1:]
    g = pr.grid(maps[:1], law, block=BLOCK, **GRID)
    wn = pr.weight(g[0], H, W, BLOCK)[y0:y0 + rows]
    m = R * P
    low = pr.low_pass(video[0, y0 - m:y0 + rows + m], R, P)[m:-m]
    want, _ = pr.blend(video[0, y0:y0 + rows], low, wn, BLOCK)
    return bool(np.array_equal(out[0, y0:y0 + rows], want.astype(np.uint8)))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--small", action="store_true", help="a rehearsal size: the figures mean nothing")
    p.add_argument("--only", type=str, default="", metavar="R,P", help="one setting alone, for a kernel trace")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefilter_time.json"))
    args = p.parse_args()
    frames, size, reps = (16, (120, 200), 2) if args.small else (F, SIZE, REPS)
    only = tuple(int(v) for v in args.only.split(",")) if args.only else None
    H, W = size
    n_bytes = frames * H * W * 3
    blobs = qr.blobs(1, H, W, seed=7, count=24)[0]
    half = np.zeros(size, np.uint8)
    half[:, :W // 2] = 255
    law = dataflow.prefilter_law(gate=128, full=16)
    gp = gen_pred()
    video = np.random.default_rng(0).integers(0, 256, (frames,) + size + (3,), dtype=np.uint8)
    sess = P3DSession("unet", batch=BATCH, seed=0, base=16, blocks=(1, 1, 1))
    gp.predict_video_resident(sess, video, BATCH, STRIDE, "newest", keep_source=True)
    out = {"tool": "tools/prefilter_time.py", "frames": frames, "size": list(size), "block": BLOCK, "frame_bytes": n_bytes, "grid_settings": GRID,
           "warm": WARM, "reps": reps, "settings": []}
    if not only:
        copy = dataflow.shots_time(video, (1, 1), reps)[2]      # as many bytes, copied device to device: each read once and written once
        out["copy_median_ms"] = round(float(np.median(copy)), 4)
        out["copy_read_plus_write_GBps"] = round(2 * n_bytes / np.median(copy) / 1e6, 1)
        print(json.dumps({k: out[k] for k in ("copy_median_ms", "copy_read_plus_write_GBps")}), flush=True)
    for name, content in (("blobs", blobs), ("left_half_salient", half)):
        sess.set_prior_map((content.astype(np.float32) + 0.25) / 255.)      # a quarter above the byte: rounded or cut, the byte comes back
        sess.set_prior_stage("mix", 1.0)
        for R, P in SETTINGS:
            if only and (R, P) != only:
                continue
            ms = {"device": [], "prefilter": [], "grid": []}
            for i in range(WARM + reps):
                res = sess.video_prefilter(0, frames, H, W, law, block=BLOCK, radius=R, passes=P, **GRID)
                sess.video_qpmap(0, frames, size, law, block=BLOCK, balance=False, target=0, lo=0, hi=64, timed=True, **GRID)
                if i >= WARM:
                    ms["device"].append(res[3]["device"])
                    ms["prefilter"].append(res[3]["prefilter"])
                    ms["grid"].append(sess.last_qpmap_ms["qpmap"])
            if not check_window(res[0], res[2], video[:1, ..., ::-1], law, R, P, y0=(H - 24) // 2):      # the kept source is B, G, R
                raise SystemExit("%s, R = %d, P = %d: the device's frames differ from the replay's" % (name, R, P))
            row = {"maps": name, "radius": R, "passes": P, "planted_exactly": bool((res[2] == content[None]).all()),
                   "mean_strength": round(float(res[1].mean()) / 64., 4), "plan": dataflow.prefilter_plan(H, W, BLOCK, R, P, frames)}
            for k in ms:
                row[k + "_median_ms"] = round(float(np.median(ms[k])), 4)
            row["filter_median_ms"] = round(row["prefilter_median_ms"] - row["grid_median_ms"], 4)
            row["prefilter_min_ms"], row["prefilter_max_ms"] = round(min(ms["prefilter"]), 4), round(max(ms["prefilter"]), 4)
            row["filter_read_plus_write_GBps"] = round(2 * n_bytes / row["filter_median_ms"] / 1e6, 1)
            if "copy_median_ms" in out:
                row["filter_share_of_copy"] = round(out["copy_median_ms"] / row["filter_median_ms"], 4)
            print(json.dumps(row), flush=True)
            out["settings"].append(row)
    sess.close_video()
    sess.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
