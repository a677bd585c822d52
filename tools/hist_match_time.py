"""Device time of the output stage with and without `set_hist_match`, HIP events through the entry points' own stage_ms, one
process (profiles/r18_hist_match_time.json):
  pred_maps_u8 at 1080x960 on a batch of 8 -- eight later windows (8 maps) and one first window (16 maps) -- with the option
  off, a table match alone, and blur sigma 32 + match + range;  evaluate at batch 2, off against "density".
Medians of REPS calls.  The maps are the net's own prediction on the synthetic clip (no entry point writes the prediction
buffer); `fullest_bin_share` says how skewed they are.  The byte floor printed beside the times is 4 bytes per pixel for the count
pass (one read) and 8 for the remap (one read, one write) at a given bandwidth (`--tbs`, default 6.2 TB/s: what adam_kernel
reaches): a prediction, not a gate.

A uniform against a u**8-skewed map, per launch:  `rocprofv3 --kernel-trace --stats -- python tools/hist_match_time.py --supplied
uniform` (or `skewed`) runs cumulative_distribution and match_hist REPS times on 8 supplied maps of that kind and nothing else;
the stats table then holds hist_count_kernel's and hist_remap_kernel's times for that input."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sap3d_tensorflow_amd import P3DSession, dataflow, synthetic      # noqa: E402

T, S, REPS, SIZE = 16, 112, 7, (1080, 960)


def median(v):
    return float(np.median(np.asarray(v)))


def table():
    """The histogram of a peaked (Gaussian blob) map, 256 entries: what a fixation density looks like."""
    y, x = np.mgrid[0:270, 0:240]
    g = np.exp(-((y - 120.0) ** 2 + (x - 100.0) ** 2) / (2 * 8.0 ** 2)).astype(np.float32)
    return dataflow.cumulative_distribution(g, 256)


def supplied(kind):
    u = np.random.default_rng(0).random((8,) + SIZE)
    maps = (u ** 8 if kind == "skewed" else u).astype(np.float32)
    tab = table()
    for _ in range(REPS):
        dataflow.cumulative_distribution(maps, 256)
        dataflow.match_hist(maps, tab[0], tab[1], 256)
    print(json.dumps({"supplied": kind, "maps": 8, "calls": REPS}))


def main():
    if "--supplied" in sys.argv:
        return supplied(sys.argv[sys.argv.index("--supplied") + 1])
    tbs = float(sys.argv[sys.argv.index("--tbs") + 1]) if "--tbs" in sys.argv else 6.2
    tab = table()
    out = {"tool": "tools/hist_match_time.py", "size": list(SIZE), "reps": REPS, "pred_maps_u8": [], "evaluate": []}
    settings = (("off", "off", None), ("table", tab, None), ("blur 32 + table + range", tab, dict(sigma=32.0, radius=0, norm="range")))
    s = P3DSession("unet", batch=8, frames=T, height=S, width=S, seed=1)
    pred = s.predict_windows(synthetic.synthetic_clip(0, (8, T, S, S, 3)))
    out["fullest_bin_share"] = round(float(np.histogram(pred, 256)[0].max()) / pred.size, 4)
    for label, match, post in settings:
        s.set_postprocess(**post) if post else s.set_postprocess(None)
        s.set_hist_match(match, 256)
        for name, first in (("8 later windows", [15] * 8), ("1 first window", [0] + [T] * 7)):
            dev, d2h = [], []
            for _ in range(REPS + 1):
                s.pred_maps_u8(first, size=SIZE)
                dev.append(s.last_maps_ms["device"])
                d2h.append(s.last_maps_ms["d2h"])
            px = sum(T - f for f in first) * SIZE[0] * SIZE[1]
            row = {"setting": label, "maps": name, "device_ms": round(median(dev[1:]), 4), "d2h_ms": round(median(d2h[1:]), 4),
                   "floor_ms_count": round(px * 4 / (tbs * 1e12) * 1e3, 4), "floor_ms_remap": round(px * 8 / (tbs * 1e12) * 1e3, 4)}
            print(json.dumps(row), flush=True)
            out["pred_maps_u8"].append(row)
    s.close()
    x, dens, fix = synthetic.synthetic_test_set(2, 2, size=SIZE)
    s = P3DSession("unet", batch=2, frames=T, height=S, width=S, seed=1)
    for match in ("off", "density", "off", "density"):
        s.set_hist_match(match, 256)
        dev, fwd = [], []
        for _ in range(REPS + 1):
            s.evaluate(x, dens, fix, size=SIZE, rng=np.random.RandomState(0))
            dev.append(s.last_eval_ms["device"])
            fwd.append(s.last_eval_ms["forward"])
        px = 2 * SIZE[0] * SIZE[1]
        row = {"hist_match": match, "batch": 2, "device_ms": round(median(dev[1:]), 4), "forward_ms": round(median(fwd[1:]), 3),
               "floor_ms_two_counts": round(2 * px * 4 / (tbs * 1e12) * 1e3, 4), "floor_ms_remap": round(px * 8 / (tbs * 1e12) * 1e3, 4)}
        print(json.dumps(row), flush=True)
        out["evaluate"].append(row)
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
