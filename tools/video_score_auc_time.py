"""Device time of AUC-Borji and shuffled AUC beside the five columns of a resident video (P3DSession.video_score_auc): 64 frames at
1080 x 960 with 300 fixations each, n_rep = 100 splits, step 0.1, the pool the video's own fixation maps (M = 10 others a frame).
Writes profiles/video_score_auc.json (--out):
  auc        HIP-event times of one call (last_score_ms: uploads, the maps' chain, the five-column launches with pass A, the
             preparation + select + sweeps), medians of REPS calls after WARM warm-up calls, for both sweeps, Borji alone and
             shuffled alone; the sweeps alone without the five columns (pass A then reads no density) as "sweeps_only";
  float_route  wall time of metrics.AUC_Borji (the route that existed before: one launch of auc_borji_kernel on the map as float32,
             with its copies and synchronisations) on ONE of those maps with that frame's indices, median of a few calls.
The maps' values matter little to the time, so the network is a small one (unet, base 16, one block per stage).  A report: nothing
is asserted but that the two routes agree on that one map to 1e-6."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sap3d_tensorflow_amd import P3DSession, metrics      # noqa: E402
from video_score_time import BATCH, F, H0, STRIDE, W0, gen_pred, truth      # noqa: E402

WARM, REPS, HOST_REPS, N_REP, STEP, M = 3, 20, 5, 100, 0.1, 10
COLUMNS = ("cc", "sim", "judd", "kl", "nss")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--small", action="store_true", help="a rehearsal size: the figures mean nothing")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_score_auc.json"))
    args = p.parse_args()
    frames, size, reps = (16, (48, 40), 2) if args.small else (F, (1080, 960), REPS)
    gp = gen_pred()
    video = np.random.default_rng(0).integers(0, 256, (frames, H0, W0, 3)).astype(np.uint8)
    sess = P3DSession("unet", batch=BATCH, seed=0, base=16, blocks=(1, 1, 1))
    gp.predict_video_resident(sess, video, BATCH, STRIDE, "newest")
    den, fix = truth(frames, *size)
    sess.open_fixation_pool(size, frames)
    sess.fixation_pool_put(0, fix)
    rng = np.random.RandomState(0)
    n_other = sess.video_shuffled_begin(gp.sauc_ids(rng, frames, 0, frames, M, True))
    bidx, nf = metrics.borji_draws_u8(fix, N_REP, rng)
    ranks, n_rows = metrics.shuffled_draws(nf, n_other, N_REP, rng)
    out = {"tool": "tools/video_score_auc_time.py", "frames": frames, "size": list(size), "n_rep": N_REP, "step": STEP, "others": M,
           "n_fix": int(nf[0]), "warm": WARM, "reps": reps, "auc": []}
    got = None
    for name, kw in (("borji + shuffled", dict(borji_idx=bidx, shuffled_ranks=ranks, n_rows=n_rows)), ("borji", dict(borji_idx=bidx)),
                     ("shuffled", dict(shuffled_ranks=ranks, n_rows=n_rows)),
                     ("sweeps_only", dict(borji_idx=bidx, shuffled_ranks=ranks, n_rows=n_rows, columns=()))):
        ms = {"upload": [], "device": [], "score": [], "auc": []}
        call = dict(size=size, columns=COLUMNS, n_rep=N_REP, step_size=STEP)
        call.update(kw)
        for i in range(WARM + reps):
            r = sess.video_score_auc(0, frames, None if call["columns"] == () else den, fix, **call)
            got = r if name == "borji + shuffled" else got
            if i >= WARM:
                for k in ms:
                    ms[k].append(sess.last_score_ms[k])
        row = {"what": name}
        for k in ms:
            row[k + "_median_ms"] = round(float(np.median(ms[k])), 4)
        row["auc_min_ms"], row["auc_max_ms"] = round(min(ms["auc"]), 4), round(max(ms["auc"]), 4)
        print(json.dumps(row), flush=True)
        out["auc"].append(row)
    maps = sess.video_maps_u8(0, 1, size=size)[0].astype(np.float32)
    idx0 = bidx[:int(nf[0]) * N_REP].reshape(int(nf[0]), N_REP)
    wall, val = [], None
    for _ in range(1 if args.small else HOST_REPS):
        t0 = time.perf_counter()
        val = metrics.AUC_Borji(maps, fix[0] / 255.0, n_rep=N_REP, step_size=STEP, rand_idx=idx0)
        wall.append((time.perf_counter() - t0) * 1e3)
    out["float_route"] = {"what": "metrics.AUC_Borji on ONE map as float32 with the same indices; wall time, the call ends synchronised",
                          "reps": len(wall), "median_ms": round(float(np.median(wall)), 3), "min_ms": round(min(wall), 3)}
    out["agreement_abs"] = abs(val - float(np.mean(got["borji"][0])))
    if not out["agreement_abs"] < 1e-6:
        raise SystemExit("the two routes disagree on AUC-Borji of frame 0: %r against %r" % (val, float(np.mean(got["borji"][0]))))
    sess.close_video()
    sess.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
