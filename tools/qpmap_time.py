"""Device time of the QP maps of a resident video (P3DSession.video_qpmap): 64 maps at 1080 x 960 with blocks of 16 and of 64, a blob
field planted through the prior stage ("mix", weight 1: every map IS the prior), so the maps come out of the same chain as a
network's.  Per block size: the HIP-event times of one call (last_qpmap_ms: the maps' chain, the qpmap launches together), the median
of REPS calls after WARM warm-up calls, the plan, and the map bytes per second of the qpmap launches.  Beside them the time of a
device-to-device copy of as many bytes (dataflow.shots_time's third column), which reads and writes each once: the streaming rate a
read-once pass is held against.  Writes profiles/qpmap_time.json (--out).  --only B runs one block size alone, for `rocprofv3
--kernel-trace --stats`.  A report: nothing is asserted but that the device's tables equal the replay's on the first two frames."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qpmap_ref as qr                                      # noqa: E402
from sap3d_tensorflow_amd import P3DSession, dataflow      # noqa: E402

F, SIZE, BATCH, STRIDE, WARM, REPS = 64, (1080, 960), 8, 8, 3, 20
SETTINGS = dict(peak_weight=128, dilate=1, fall=1, rise=3, lo=-12, hi=6)


def gen_pred():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--small", action="store_true", help="a rehearsal size: the figures mean nothing")
    p.add_argument("--only", type=int, default=0, metavar="B", help="one block size alone, for a kernel trace")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "qpmap_time.json"))
    args = p.parse_args()
    frames, size, reps = (16, (90, 80), 2) if args.small else (F, SIZE, REPS)
    H, W = size
    n_bytes = frames * H * W
    content = qr.blobs(1, H, W, seed=7, count=24)[0]
    law = dataflow.qp_law(SETTINGS["lo"], SETTINGS["hi"], gate=16)
    gp = gen_pred()
    video = np.random.default_rng(0).integers(0, 256, (frames,) + size + (3,), dtype=np.uint8)
    sess = P3DSession("unet", batch=BATCH, seed=0, base=16, blocks=(1, 1, 1))
    gp.predict_video_resident(sess, video, BATCH, STRIDE, "newest")
    sess.set_prior_map((content.astype(np.float32) + 0.25) / 255.)      # a quarter above the byte: rounded or cut, the byte comes back
    sess.set_prior_stage("mix", 1.0)
    out = {"tool": "tools/qpmap_time.py", "frames": frames, "size": list(size), "map_bytes": n_bytes, "settings": SETTINGS, "warm": WARM,
           "reps": reps, "blocks": []}
    if not args.only:
        # as many bytes as the maps, copied device to device: each read once and written once
        third = video[:, :, :W // 3]
        copy = dataflow.shots_time(third, (1, 1), reps)[2]
        out["copy_bytes"] = int(third.size)
        out["copy_median_ms"] = round(float(np.median(copy)), 4)
        out["copy_read_plus_write_GBps"] = round(2 * third.size / np.median(copy) / 1e6, 1)
        print(json.dumps({k: out[k] for k in ("copy_bytes", "copy_median_ms", "copy_read_plus_write_GBps")}), flush=True)
    for B in (16, 64):
        if args.only and B != args.only:
            continue
        ms = {"device": [], "qpmap": []}
        for i in range(WARM + reps):
            res = sess.video_qpmap(0, frames, size, law, block=B, with_levels=True, with_stats=True, with_maps=(i == 0), timed=True, **SETTINGS)
            if i == 0:
                maps = res["maps"]
            if i >= WARM:
                for k in ms:
                    ms[k].append(sess.last_qpmap_ms[k])
        want = qr.qpmap(maps[:2], law, B, SETTINGS["peak_weight"], SETTINGS["dilate"], SETTINGS["fall"], SETTINGS["rise"], 1, 0,
                        SETTINGS["lo"], SETTINGS["hi"])
        if not all(np.array_equal(res[k][:2], w) for k, w in zip(("qp", "levels", "stats"), want)):
            raise SystemExit("block %d: the device's tables differ from the replay's" % B)
        row = {"block": B, "grid": list(res["qp"].shape[1:]), "planted_exactly": bool((maps == content[None]).all()),
               "plan": dataflow.qpmap_plan(H, W, B, frames)}
        for k in ms:
            row[k + "_median_ms"] = round(float(np.median(ms[k])), 4)
        row["qpmap_min_ms"], row["qpmap_max_ms"] = round(min(ms["qpmap"]), 4), round(max(ms["qpmap"]), 4)
        row["qpmap_over_chain"] = round(row["qpmap_median_ms"] / row["device_median_ms"], 4)
        row["qpmap_map_GBps"] = round(n_bytes / row["qpmap_median_ms"] / 1e6, 1)
        print(json.dumps(row), flush=True)
        out["blocks"].append(row)
    sess.close_video()
    sess.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
