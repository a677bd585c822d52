"""Device time of the distortion stage of a resident video (P3DSession.video_distortion): 64 frames at 1080 x 1920 against the kept
source (random bytes), the test frames the source with about half of its bytes moved by a few levels, the maps a blob field planted
through the prior stage ("mix", weight 1: every map IS the prior), so they come out of the same chain as a network's.  Per setting --
without the block map and with blocks of 16 -- the HIP-event times of the test frames' upload, of the maps' chain and of the
distortion launches, the median of REPS calls after WARM warm-up calls, and the plan.  The contract has no switch for SSIM, so the
stage is not timed without it; --only BLOCK runs one setting alone for `rocprofv3 --kernel-trace --stats`, whose rows split the
stage's time between distortion_sums and distortion_ssim.  Beside them, in the same process, a device-to-device copy of n * H * W * 3
bytes (dataflow.shots_time's third column): the stage must read 7 bytes a pixel (the map, the reference, the test frame) and
writes next to nothing, and its compulsory bytes per second are reported as a share of the copy's read-plus-write rate, and held
against nothing else.  Writes profiles/distortion_time.json (--out).  A report: nothing is asserted but that the first frame's record
equals the replay's."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import distortion_ref as dr                                 # noqa: E402
import qpmap_ref as qr                                      # noqa: E402
from sap3d_tensorflow_amd import P3DSession, dataflow      # noqa: E402

F, SIZE, BATCH, STRIDE, WARM, REPS, GATE = 64, (1080, 1920), 8, 8, 2, 10, 128
BLOCKS = (0, 16)


def gen_pred():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--small", action="store_true", help="a rehearsal size: the figures mean nothing")
    p.add_argument("--only", type=int, default=None, metavar="BLOCK", help="one setting alone, for a kernel trace")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "distortion_time.json"))
    args = p.parse_args()
    frames, size, reps = (16, (120, 200), 2) if args.small else (F, SIZE, REPS)
    H, W = size
    pixels = frames * H * W
    blobs = qr.blobs(1, H, W, seed=7, count=24)[0]
    law = dataflow.distortion_law(gate=GATE // 2, floor=1)
    gp = gen_pred()
    rng = np.random.default_rng(0)
    video = rng.integers(0, 256, (frames,) + size + (3,), dtype=np.uint8)
    step = rng.integers(-6, 7, video.shape, dtype=np.int16) * (rng.random(video.shape, dtype=np.float32) < 0.5)
    test_bgr = np.ascontiguousarray(np.clip(video[..., ::-1].astype(np.int16) + step, 0, 255).astype(np.uint8))      # the kept source is B, G, R
    del step
    sess = P3DSession("unet", batch=BATCH, seed=0, base=16, blocks=(1, 1, 1))
    gp.predict_video_resident(sess, video, BATCH, STRIDE, "newest", keep_source=True)
    out = {"tool": "tools/distortion_time.py", "frames": frames, "size": list(size), "gate": GATE, "pixels": pixels,
           "compulsory_read_bytes": 7 * pixels, "warm": WARM, "reps": reps, "settings": []}
    if args.only is None:
        copy = dataflow.shots_time(video, (1, 1), reps)[2]      # 3 bytes a pixel copied device to device: each read once and written once
        out["copy_median_ms"] = round(float(np.median(copy)), 4)
        out["copy_read_plus_write_GBps"] = round(2 * 3 * pixels / np.median(copy) / 1e6, 1)
        print(json.dumps({k: out[k] for k in ("copy_median_ms", "copy_read_plus_write_GBps")}), flush=True)
    sess.set_prior_map((blobs.astype(np.float32) + 0.25) / 255.)      # a quarter above the byte: rounded or cut, the byte comes back
    sess.set_prior_stage("mix", 1.0)
    for block in BLOCKS:
        if args.only is not None and block != args.only:
            continue
        ms = {"upload": [], "device": [], "distortion": []}
        for i in range(WARM + reps):
            table, bs, maps, t = sess.video_distortion(0, frames, test_bgr, law, block=block, gate=GATE)
            if i >= WARM:
                for k in ms:
                    ms[k].append(t[k])
        want = dr.distortion(maps[:1], video[:1, ..., ::-1], test_bgr[:1], law, block=block, gate=GATE)
        if not np.array_equal(table[0], want[0][0]) or (block and not np.array_equal(bs[0], want[1][0])):
            raise SystemExit("block = %d: the device's record of the first frame differs from the replay's" % block)
        rep = dataflow.distortion_report(table, H * W)
        row = {"block": block, "ssim": True, "planted_exactly": bool((maps == blobs[None]).all()), "plan": dataflow.distortion_plan(H, W, block, frames),
               "mean_psnr_y": round(float(rep["psnr"][:, 3].mean()), 4), "mean_wpsnr_y": round(float(rep["wpsnr"][:, 3].mean()), 4),
               "mean_ssim": round(float(rep["ssim"].mean()), 6), "mean_wssim": round(float(rep["wssim"].mean()), 6)}
        for k in ms:
            row[k + "_median_ms"] = round(float(np.median(ms[k])), 4)
        row["distortion_min_ms"], row["distortion_max_ms"] = round(min(ms["distortion"]), 4), round(max(ms["distortion"]), 4)
        row["compulsory_read_GBps"] = round(7 * pixels / row["distortion_median_ms"] / 1e6, 1)
        if "copy_median_ms" in out:
            row["read_rate_share_of_copy"] = round(row["compulsory_read_GBps"] / out["copy_read_plus_write_GBps"], 4)
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
