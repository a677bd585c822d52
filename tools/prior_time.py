"""Device time of the fixation-prior kernels, HIP events through the entry points' own timings, one process, medians of REPS
calls (profiles/r20_prior_time.json):
  count   P3DSession.prior_add on 1 000 fixation maps at 1080x960 and on 100 000 maps at 112x112 (prior_last_ms: the count
          launches alone, the upload excluded), read against the byte floor of n H W bytes;
  finish  P3DSession.finish_prior at 1080x960 with sigma 32 (conversion, blur, min / max, apply and the read-back of the maximum);
  apply   pred_maps_u8's device stage for 8 and 16 maps at 1080x960, option off / the float32 chain without the stage / with it: the
          difference of the last two is the stage, read against 8 bytes per pixel (the prior's 4 bytes are shared by all maps);
  evaluate at batch 2, stage off / on.
The floors are bytes at a given bandwidth (`--tbs`, default 6.2 TB/s: what adam_kernel reaches): a
prediction, not a gate.  `--small` cuts the two count cases to a tenth (host memory)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sap3d_tensorflow_amd import P3DSession, dataflow, synthetic      # noqa: E402

T, S, REPS, SIZE = 16, 112, 7, (1080, 960)


def median(v):
    return float(np.median(np.asarray(v)))


def main():
    tbs = float(sys.argv[sys.argv.index("--tbs") + 1]) if "--tbs" in sys.argv else 6.2
    small = "--small" in sys.argv
    out = {"tool": "tools/prior_time.py", "reps": REPS, "tbs": tbs, "count": [], "finish": [], "pred_maps_u8": [], "evaluate": []}
    s = P3DSession("unet", batch=8, frames=T, height=S, width=S, seed=1)
    rng = np.random.default_rng(0)
    for n, size in ((100 if small else 1000, SIZE), (10000 if small else 100000, (S, S))):
        one = (rng.random((50,) + size) < 0.01).astype(np.uint8) * 255
        maps = np.ascontiguousarray(np.broadcast_to(one[None], (n // 50, 50) + size).reshape((n,) + size))
        s.open_prior(size, "fixations")
        ms = []
        for k in range(REPS + 1):
            s.prior_add(maps, 1 if k % 2 == 0 else -1)
            ms.append(s.prior_last_ms()[0])
        floor = n * size[0] * size[1] / (tbs * 1e12) * 1e3
        row = {"maps": n, "size": list(size), "plan_words_singles_slices": list(dataflow.prior_count_plan(min(n, (256 << 20) // (size[0] * size[1])), *size)),
               "count_ms": round(median(ms[1:]), 4), "floor_ms": round(floor, 4), "ratio": round(median(ms[1:]) / floor, 2)}
        print(json.dumps(row), flush=True)
        out["count"].append(row)
        if size == SIZE:
            s.prior_add(maps[:50])
            fin = []
            for _ in range(REPS + 1):
                s.finish_prior(32.0)
                fin.append(s.prior_last_ms()[1])
            row = {"size": list(size), "sigma": 32.0, "finish_ms": round(median(fin[1:]), 4)}
            print(json.dumps(row), flush=True)
            out["finish"].append(row)
        del maps
    s.close_prior()
    s.predict_windows(synthetic.synthetic_clip(0, (8, T, S, S, 3)))
    for label in ("off", "chain without the stage (max)", "chain with the stage (mul 0.25, max)"):
        s.set_postprocess(0., 0, "none" if label == "off" else "max")
        s.set_prior_stage("mul" if "with the stage" in label else "off", 0.25)
        for name, first in (("8 later windows", [15] * 8), ("1 first window", [0] + [T] * 7)):
            dev = []
            for _ in range(REPS + 1):
                s.pred_maps_u8(first, size=SIZE)
                dev.append(s.last_maps_ms["device"])
            px = sum(T - f for f in first) * SIZE[0] * SIZE[1]
            row = {"setting": label, "maps": name, "device_ms": round(median(dev[1:]), 4), "floor_ms_apply": round(px * 8 / (tbs * 1e12) * 1e3, 4)}
            print(json.dumps(row), flush=True)
            out["pred_maps_u8"].append(row)
    s.close()
    x, dens, fix = synthetic.synthetic_test_set(2, 2, size=SIZE)
    s = P3DSession("unet", batch=2, frames=T, height=S, width=S, seed=1)
    s.open_prior(SIZE)
    s.prior_add(fix)
    s.finish_prior(32.0)
    for mode in ("off", "mul", "off", "mul"):
        s.set_prior_stage(mode, 0.25)
        dev = []
        for _ in range(REPS + 1):
            s.evaluate(x, dens, fix, size=SIZE, rng=np.random.RandomState(0))
            dev.append(s.last_eval_ms["device"])
        row = {"prior_stage": mode, "batch": 2, "device_ms": round(median(dev[1:]), 4),
               "floor_ms_apply": round(2 * SIZE[0] * SIZE[1] * 8 / (tbs * 1e12) * 1e3, 4)}
        print(json.dumps(row), flush=True)
        out["evaluate"].append(row)
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
