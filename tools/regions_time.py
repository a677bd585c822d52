"""Device time of labelling the salient regions of a resident video (P3DSession.video_regions): 128 maps at 1080 x 960, K = 64,
linked, with three contents -- blob fields (tests/regions_ref.py's generator, gate 128, c = 8), a checkerboard at c = 4 (the most
components a map can hold) and a serpentine at c = 4 (the longest union chain).  The contents are planted through the prior stage
("mix", weight 1: every map IS the prior), so the maps come out of the same chain as a network's; every frame of a call holds the
same map.  Per content: the HIP-event times of one call (last_regions_ms: the maps' chain, the regions launches together), the
median of REPS calls after WARM warm-up calls, the plan of the launches, and beside them what a user has today: the maps copied to
the host and scipy.ndimage.label plus statistics per frame (timed on HOST_FRAMES frames, scaled to the call's).  Writes
profiles/regions_time.json (--out).  --only CONTENT runs one content alone, for `rocprofv3 --kernel-trace --stats`.  A report: nothing is asserted but that the device's tables equal the replay's on one frame."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import regions_ref as rr                                    # noqa: E402
from sap3d_tensorflow_amd import P3DSession, dataflow      # noqa: E402

F, SIZE, BATCH, STRIDE, WARM, REPS, HOST_FRAMES = 128, (1080, 960), 8, 8, 3, 10, 4


def gen_pred():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


def host_baseline(maps, gate, conn):
    """ms a frame of scipy.ndimage.label + area, mass, peak, box and centre on the host, or None without scipy."""
    try:
        from scipy import ndimage as ndi
    except ImportError:
        return None
    structure = np.ones((3, 3), int) if conn == 8 else ndi.generate_binary_structure(2, 1)
    t0 = time.perf_counter()
    for s in maps:
        lab, count = ndi.label(s >= gate, structure=structure)
        idx = np.arange(1, count + 1)
        ndi.sum(s, lab, idx); ndi.sum(np.ones_like(s), lab, idx); ndi.maximum(s, lab, idx)
        ndi.find_objects(lab)
        ndi.center_of_mass(s, lab, idx)
    return (time.perf_counter() - t0) * 1e3 / len(maps)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--small", action="store_true", help="a rehearsal size: the figures mean nothing")
    p.add_argument("--only", default="", metavar="CONTENT", help="one content alone (blobs, checkerboard, serpentine), for a kernel trace")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions_time.json"))
    args = p.parse_args()
    frames, size, reps = (16, (90, 80), 2) if args.small else (F, SIZE, REPS)
    H, W = size
    contents = [("blobs", rr.blobs(1, H, W, seed=7, count=24)[0], 128, 8), ("checkerboard", rr.checkerboard(H, W), 1, 4),
                ("serpentine", rr.serpentine(H, W), 1, 4)]
    contents = [c for c in contents if not args.only or c[0] == args.only]
    gp = gen_pred()
    video = np.random.default_rng(0).integers(0, 256, (frames,) + size + (3,), dtype=np.uint8)
    sess = P3DSession("unet", batch=BATCH, seed=0, base=16, blocks=(1, 1, 1))
    gp.predict_video_resident(sess, video, BATCH, STRIDE, "newest")
    out = {"tool": "tools/regions_time.py", "frames": frames, "size": list(size), "max_regions": 64, "link": True, "warm": WARM, "reps": reps,
           "host_frames_timed": HOST_FRAMES, "contents": []}
    for name, content, gate, conn in contents:
        sess.set_prior_map((content.astype(np.float32) + 0.25) / 255.)      # a quarter above the byte: rounded or cut, the byte comes back
        sess.set_prior_stage("mix", 1.0)
        ms = {"device": [], "regions": []}
        for i in range(WARM + reps):
            res = sess.video_regions(0, frames, size, gate, connectivity=conn, link=True, with_maps=(i == 0), timed=True)
            if i == 0:
                maps = res["maps"]
            if i >= WARM:
                for k in ms:
                    ms[k].append(sess.last_regions_ms[k])
        if name == "checkerboard" and not args.small:      # (half a million components are slow to replay: their number and the K roots)
            ok = res["counts"][0].tolist() == [(H * W + 1) // 2, (H * W + 1) // 2, 64] and res["regions"][0, :, rr.ROOT].tolist() == list(range(0, 128, 2))
        else:
            want = rr.regions(maps[:1], gate, conn, 1, 64)
            ok = np.array_equal(res["counts"][:1], want[1]) and np.array_equal(res["regions"][0, :, :rr.ID], want[0][0, :, :rr.ID])
        if not ok:
            raise SystemExit("%s: the device's table differs from the replay's" % name)
        row = {"content": name, "gate": gate, "connectivity": conn, "planted_exactly": bool((maps == content[None]).all()),
               "counts_frame0": res["counts"][0].tolist(), "plan": dataflow.regions_plan(H, W, frames, 64, True, False)}
        for k in ms:
            row[k + "_median_ms"] = round(float(np.median(ms[k])), 4)
        row["regions_min_ms"], row["regions_max_ms"] = round(min(ms["regions"]), 4), round(max(ms["regions"]), 4)
        row["regions_over_chain"] = round(row["regions_median_ms"] / row["device_median_ms"], 4)
        host = host_baseline(maps[:HOST_FRAMES], gate, conn)
        if host is not None:
            row["host_scipy_ms"] = round(host * frames, 2)
            row["host_over_regions"] = round(host * frames / row["regions_median_ms"], 2)
        print(json.dumps(row), flush=True)
        out["contents"].append(row)
    sess.close_video()
    sess.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
