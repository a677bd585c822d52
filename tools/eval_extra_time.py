"""Device time of `evaluate`'s metric stage with and without `set_eval_extra`, HIP events through p3d_eval_last_frames' own
stage_ms, one process (profiles/r19_eval_extra_time.json): the unet at batch 2, 1080x960 maps, the settings off / KL / KL + IG /
off in turn, medians of REPS calls each (one more call first, not counted).

The quantity to read the added time against is the byte floor of the one launch the option adds: per pixel it reads the float32
prediction and the float32 density for KL (8 bytes), and the fixation byte and the float32 baseline as well with IG (13 bytes), at a
given bandwidth (`--tbs`, default 6.2 TB/s: what adam_kernel reaches).  The launch also takes a double-precision
division and a log per pixel (two log2 more per fixated pixel), so it is not expected on that floor: the ratio is reported, not
tuned to.

  --off-only          the option-off stage alone (no entry point of the option is touched)
  --root DIR          import the package from another checkout, e.g. the parent commit's, for a same-box A/B of --off-only
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
from sap3d_tensorflow_amd import P3DSession, synthetic      # noqa: E402

T, S, REPS, SIZE, BATCH = 16, 112, 7, (1080, 960), 2


def prior(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return (0.1 + np.exp(-(((y - 0.45 * H) / (0.3 * H)) ** 2 + ((x - 0.55 * W) / (0.3 * W)) ** 2))).astype(np.float32)


def measure(s, x, dens, fix):
    dev = []
    for _ in range(REPS + 1):
        s.evaluate(x, dens, fix, size=SIZE, rng=np.random.RandomState(0))
        dev.append(s.last_eval_ms["device"])
    return float(np.median(np.asarray(dev[1:])))


def main():
    tbs = float(sys.argv[sys.argv.index("--tbs") + 1]) if "--tbs" in sys.argv else 6.2
    x, dens, fix = synthetic.synthetic_test_set(2, BATCH, size=SIZE)
    s = P3DSession("unet", batch=BATCH, frames=T, height=S, width=S, seed=1)
    if "--off-only" in sys.argv:
        row = {"tool": "tools/eval_extra_time.py --off-only", "root": os.path.basename(ROOT), "batch": BATCH, "size": list(SIZE),
               "reps": REPS, "device_ms": round(measure(s, x, dens, fix), 4)}
        print(json.dumps(row))
        s.close()
        return
    px = BATCH * SIZE[0] * SIZE[1]
    floor = {"off": 0.0, "kl": px * 8 / (tbs * 1e12) * 1e3, "kl+ig": px * 13 / (tbs * 1e12) * 1e3}
    out = {"tool": "tools/eval_extra_time.py", "batch": BATCH, "size": list(SIZE), "reps": REPS, "tbs": tbs, "runs": []}
    base = prior(*SIZE)
    for setting in ("off", "kl", "kl+ig", "off"):
        if setting == "off":
            s.set_eval_extra(False)
        else:
            s.set_eval_extra(kldiv=True, info_gain=setting == "kl+ig", baseline=base if setting == "kl+ig" else None)
        row = {"setting": setting, "device_ms": round(measure(s, x, dens, fix), 4), "floor_ms": round(floor[setting], 5)}
        if setting != "off":
            row["last_eval_extra"] = s.last_eval_extra().tolist()
        print(json.dumps(row), flush=True)
        out["runs"].append(row)
    s.close()
    off = float(np.mean([r["device_ms"] for r in out["runs"] if r["setting"] == "off"]))
    out["off_ms"] = round(off, 4)
    for r in out["runs"]:
        if r["setting"] != "off":
            r["added_ms"] = round(r["device_ms"] - off, 4)
            r["added_over_floor"] = round((r["device_ms"] - off) / r["floor_ms"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
