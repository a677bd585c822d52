"""Device time of the output stage with and without `set_postprocess`, HIP events through the entry points' own stage_ms, one
process (profiles/r16_postprocess_time.json):
  pred_maps_u8 at 1080x960 on a batch of 8 -- eight later windows (one map each) and one first window (16 maps) -- with the
  option off, sigma 8, and sigma 32 with range normalisation;  evaluate at batch 2, off and on.
Medians of REPS calls.  Under `rocprofv3 --kernel-trace --stats -- python tools/postprocess_time.py` the stats table holds the
per-launch times of blur_h_kernel / blur_v_kernel / minmax_kernel / apply_kernel beside resize_f32_kernel and resize_u8_kernel
(not recorded yet).  The byte floor printed beside them is 8 bytes per pixel per pass at a given bandwidth
(`--tbs`, default 6.2 TB/s: what adam_kernel reaches): a prediction, not a gate."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sap3d_tensorflow_amd import P3DSession, synthetic      # noqa: E402

T, S, REPS, SIZE = 16, 112, 7, (1080, 960)
SETTINGS = (None, dict(sigma=8.0, radius=0, norm="none"), dict(sigma=32.0, radius=0, norm="range"))


def median(v):
    return float(np.median(np.asarray(v)))


def main():
    tbs = float(sys.argv[sys.argv.index("--tbs") + 1]) if "--tbs" in sys.argv else 6.2
    out = {"tool": "tools/postprocess_time.py", "size": list(SIZE), "reps": REPS, "pred_maps_u8": [], "evaluate": []}
    s = P3DSession("unet", batch=8, frames=T, height=S, width=S, seed=1)
    s.predict_windows(synthetic.synthetic_clip(0, (8, T, S, S, 3)))
    for post in SETTINGS:
        s.set_postprocess(**post) if post else s.set_postprocess(None)
        for name, first in (("8 later windows", [15] * 8), ("1 first window", [0] + [T] * 7)):
            dev, d2h = [], []
            for _ in range(REPS + 1):
                s.pred_maps_u8(first, size=SIZE)
                dev.append(s.last_maps_ms["device"])
                d2h.append(s.last_maps_ms["d2h"])
            maps = sum(T - f for f in first)
            row = {"postprocess": post, "maps": name, "device_ms": round(median(dev[1:]), 4), "d2h_ms": round(median(d2h[1:]), 4),
                   "floor_ms_per_blur_pass": round(maps * SIZE[0] * SIZE[1] * 8 / (tbs * 1e12) * 1e3, 4)}
            print(json.dumps(row), flush=True)
            out["pred_maps_u8"].append(row)
    s.close()
    x, dens, fix = synthetic.synthetic_test_set(2, 2, size=SIZE)
    s = P3DSession("unet", batch=2, frames=T, height=S, width=S, seed=1)
    for post in (None, SETTINGS[2], None, SETTINGS[2]):
        s.set_postprocess(**post) if post else s.set_postprocess(None)
        dev, fwd = [], []
        for _ in range(REPS + 1):
            s.evaluate(x, dens, fix, size=SIZE, rng=np.random.RandomState(0))
            dev.append(s.last_eval_ms["device"])
            fwd.append(s.last_eval_ms["forward"])
        row = {"postprocess": post, "batch": 2, "device_ms": round(median(dev[1:]), 4), "forward_ms": round(median(fwd[1:]), 3),
               "floor_ms_per_blur_pass": round(2 * SIZE[0] * SIZE[1] * 8 / (tbs * 1e12) * 1e3, 4)}
        print(json.dumps(row), flush=True)
        out["evaluate"].append(row)
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
