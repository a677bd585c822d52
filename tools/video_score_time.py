"""Device time of scoring a resident video's 8-bit maps against ground truth (P3DSession.video_score) at the size result tables
are built at: 64 frames at 1080 x 960, once with the .m file's masks (CC, SIM, AUC-Judd) and once with all five columns, beside the
route that existed before the stage for the same frames -- video_maps_u8 (the bytes to the host) and metrics.evaluate_maps (a
float32 chain that sorts every map for AUC-Judd).  Writes profiles/video_score.json (--out):
  score      per column set: the HIP-event times of one call (last_score_ms: uploads, the maps' chain, the scoring launches), the
             median of REPS calls after WARM warm-up calls.  "cc" alone runs the table pass (pass A) and nothing else, so its
             scoring time is the memset of the tables plus score_count_kernel; its 3 bytes a pixel over that time is the rate
             to hold against the HBM roof;
  host_route wall time (the calls end synchronised) of video_maps_u8 in calls of 16 frames plus evaluate_maps on those bytes in
             calls of 16 maps, AUC-Borji cut to one split: the median of a few repetitions.
--trace-only runs WARM + REPS calls with all five columns and nothing else, for rocprofv3 --kernel-trace --stats.
The maps' values matter little to the time, so the network is a small one (unet, base 16, one block per stage); the ground truth
is blobs plus noise with a few hundred fixations.  A report: nothing is asserted but that both routes score the same bytes."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sap3d_tensorflow_amd import P3DSession, metrics      # noqa: E402

F, H0, W0, BATCH, STRIDE, WARM, REPS, HOST_REPS = 64, 120, 160, 8, 8, 3, 20, 3
SETS = [("cc", ("cc",)), ("matlab", ("cc", "sim", "judd")), ("all", ("cc", "sim", "judd", "kl", "nss"))]


def gen_pred():
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


def truth(n, H, W, seed=1):
    """density and fixation uint8 [n, H, W]: three blobs plus noise, cubed (skewed, as density images are); 300 fixations."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    den, fix = np.empty((n, H, W), np.uint8), np.zeros((n, H * W), np.uint8)
    for i in range(n):
        m = np.zeros((H, W), np.float32)
        for _ in range(3):
            cy, cx, sg = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.08, 0.25) * max(H, W)
            m += np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * sg * sg))
        m = np.clip(m / m.max() + 0.01 * rng.standard_normal((H, W)).astype(np.float32), 0.0, 1.0)
        den[i] = np.rint(255.0 * m ** 3)
        fix[i, rng.choice(H * W, 300, replace=False)] = 255
    return den, fix.reshape(n, H, W)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--small", action="store_true", help="a rehearsal size: the figures mean nothing")
    p.add_argument("--trace-only", action="store_true", help="only scoring calls with all five columns, for a kernel trace")
    p.add_argument("--no-host", action="store_true", help="skip the host route (for an A/B of the scoring launches alone)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_score.json"))
    args = p.parse_args()
    frames, size, reps = (16, (48, 40), 2) if args.small else (F, (1080, 960), REPS)
    gp = gen_pred()
    video = np.random.default_rng(0).integers(0, 256, (frames, H0, W0, 3)).astype(np.uint8)
    sess = P3DSession("unet", batch=BATCH, seed=0, base=16, blocks=(1, 1, 1))
    gp.predict_video_resident(sess, video, BATCH, STRIDE, "newest")
    den, fix = truth(frames, *size)
    if args.trace_only:
        for _ in range(WARM + reps):
            sess.video_score(0, frames, den, fix, size=size, columns=SETS[-1][1])
        sess.close_video()
        sess.close()
        return
    n_pix = size[0] * size[1]
    blocks, chunk, products = metrics.score_plan(n_pix, frames)
    out = {"tool": "tools/video_score_time.py", "frames": frames, "size": list(size), "warm": WARM, "reps": reps,
           "plan": {"blocks_per_map": blocks, "pixels_per_block": chunk, "products_per_lane": products}, "score": [], "host_route": None}
    scores = None
    for name, columns in SETS:
        ms = {"upload": [], "device": [], "score": []}
        for i in range(WARM + reps):
            scores = sess.video_score(0, frames, den, fix, size=size, columns=columns)
            if i >= WARM:
                for k in ms:
                    ms[k].append(sess.last_score_ms[k])
        row = {"columns": name}
        for k in ms:
            row[k + "_median_ms"] = round(float(np.median(ms[k])), 4)
        row["score_min_ms"], row["score_max_ms"] = round(min(ms["score"]), 4), round(max(ms["score"]), 4)
        if name == "cc":
            row["pass_a_bytes"] = 3.0 * frames * n_pix
            row["pass_a_gb_per_s"] = round(row["pass_a_bytes"] / (row["score_median_ms"] * 1e-3) / 1e9, 1)
        print(json.dumps(row), flush=True)
        out["score"].append(row)
    wall, maps_ms, eval_ms, host = [], [], [], None
    for _ in range(0 if args.no_host else 1 if args.small else HOST_REPS):
        t0 = time.perf_counter()
        maps = np.concatenate([sess.video_maps_u8(f, min(16, frames - f), size=size) for f in range(0, frames, 16)])
        t1 = time.perf_counter()
        host = np.concatenate([metrics.evaluate_maps(maps[f:f + 16].astype(np.float32), den[f:f + 16], fix[f:f + 16], n_rep=1,
                                                     rng=np.random.RandomState(0)) for f in range(0, frames, 16)])
        t2 = time.perf_counter()
        wall.append((t2 - t0) * 1e3)
        maps_ms.append((t1 - t0) * 1e3)
        eval_ms.append((t2 - t1) * 1e3)
    if args.no_host:
        print(json.dumps(out))
        return
    out["host_route"] = {"what": "video_maps_u8 in calls of 16 frames + metrics.evaluate_maps on the bytes as float32, n_rep = 1; wall time",
                         "reps": len(wall), "median_ms": round(float(np.median(wall)), 2), "maps_u8_median_ms": round(float(np.median(maps_ms)), 2),
                         "evaluate_maps_median_ms": round(float(np.median(eval_ms)), 2)}
    # the same bytes either way: CC and NSS agree closely (float32 normalisation on one side), AUC-Judd up to the jitter's effect on ties
    out["agreement"] = {"cc_max_abs": float(np.nanmax(np.abs(host[:, 0] - scores[:, 0]))), "sim_max_abs": float(np.nanmax(np.abs(host[:, 1] - scores[:, 1]))),
                        "judd_max_abs": float(np.nanmax(np.abs(host[:, 2] - scores[:, 2]))), "nss_max_abs": float(np.nanmax(np.abs(host[:, 4] - scores[:, 4])))}
    if not out["agreement"]["cc_max_abs"] < 1e-3:
        raise SystemExit("the two routes disagree on CC: %r" % (out["agreement"],))
    sess.close_video()
    sess.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
