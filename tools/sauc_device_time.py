"""Shuffled AUC's sixth column of drivers/test.py, host path against device path, one process (profiles/sauc_device_time.json):
unet, batch 2 of 16x112x112, maps at 1080x960, M = 10 other clips, n_rep = 100 splits, a 64-clip synthetic set.  Per iteration, on
the same batch: a plain evaluate, then the host path (drivers/test.py's shuffled_auc: download, second chain, union on the host,
one p3d_metric_auc_shuffled per clip), then the device path (shuffled_begin + the armed evaluate); 2 warm-ups, medians of 7.
  wall        the sixth column per batch: the host path's own wall time; the device path's as (begin + armed evaluate) - plain
              evaluate;
  HIP events  pack per map (fixation_pool_put of the 64 maps / 64), union + scan, select, the clean moments + borji
              (fixation_pool_last_ms), beside byte floors at `--tbs` (default 6.2 TB/s, what adam_kernel reaches, DESIGN.md
              section 6): pack reads H W bytes per map, the union reads M nw 8 bytes per clip.
Predictions and ratios, no gates: the launches are expected to be latency bound.  `--clips N` shrinks the set."""
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sap3d_tensorflow_amd import P3DSession, synthetic      # noqa: E402

T, S, SIZE, M, N_REP, WARM, REPS, BATCH = 16, 112, (1080, 960), 10, 100, 2, 7, 2


def median(v):
    return float(np.median(np.asarray(v)))


def main():
    tbs = float(sys.argv[sys.argv.index("--tbs") + 1]) if "--tbs" in sys.argv else 6.2
    clips = int(sys.argv[sys.argv.index("--clips") + 1]) if "--clips" in sys.argv else 64
    spec = importlib.util.spec_from_file_location("p3d_test_driver", os.path.join(ROOT, "drivers", "test.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    x, dens, fix = synthetic.synthetic_test_set(0, clips, size=SIZE)
    s = P3DSession("unet", batch=BATCH, frames=T, height=S, width=S, seed=1)
    s.open_fixation_pool(SIZE, clips)
    pack = []
    for _ in range(3):
        s.fixation_pool_put(0, fix)
        pack.append(s.fixation_pool_last_ms()["pack"] / clips)
    nw = s.fixation_pool_info()["words"]
    wall = {"plain": [], "host": [], "device": []}
    ev = {"union": [], "select": [], "score": []}
    host_rng, dev_rng = np.random.RandomState(0), np.random.RandomState(0)
    for it in range(WARM + REPS):
        lo = (it * BATCH) % (clips - BATCH + 1)
        xb, db, fb = x[lo:lo + BATCH], dens[lo:lo + BATCH], fix[lo:lo + BATCH]
        t0 = time.perf_counter()
        s.evaluate(xb, db, fb, size=SIZE, rng=np.random.RandomState(it))
        t1 = time.perf_counter()
        drv.shuffled_auc(s, fix, lo, M, host_rng)
        t2 = time.perf_counter()
        others = drv.sauc_others(clips, lo, lo + BATCH, M, dev_rng)
        n_other = s.shuffled_begin(others)
        s.evaluate(xb, db, fb, size=SIZE, rng=np.random.RandomState(it), shuffled=dict(others=others, n_other=n_other, rng=dev_rng, n_rep=N_REP))
        s.last_eval_shuffled()
        t3 = time.perf_counter()
        if it >= WARM:
            wall["plain"].append((t1 - t0) * 1e3); wall["host"].append((t2 - t1) * 1e3); wall["device"].append((t3 - t2) * 1e3)
            ms = s.fixation_pool_last_ms()
            for k in ev:
                ev[k].append(ms[k])
    s.close()
    n_pix = SIZE[0] * SIZE[1]
    floor_pack = n_pix / (tbs * 1e12) * 1e3
    floor_union = BATCH * M * nw * 8 / (tbs * 1e12) * 1e3
    dev_col = median(wall["device"]) - median(wall["plain"])
    out = {"tool": "tools/sauc_device_time.py", "clips": clips, "batch": BATCH, "size": list(SIZE), "M": M, "n_rep": N_REP, "warmups": WARM,
           "reps": REPS, "tbs": tbs,
           "wall_ms_per_batch": {"plain_evaluate": round(median(wall["plain"]), 3), "host_sixth_column": round(median(wall["host"]), 3),
                                 "begin_plus_armed_evaluate": round(median(wall["device"]), 3), "device_sixth_column": round(dev_col, 3),
                                 "host_over_device": round(median(wall["host"]) / dev_col, 2) if dev_col > 0 else None},
           "hip_event_ms": {"pack_per_map": round(median(pack), 5), "pack_floor": round(floor_pack, 5), "pack_ratio": round(median(pack) / floor_pack, 1),
                            "union_scan": round(median(ev["union"]), 5), "union_floor": round(floor_union, 5),
                            "union_ratio": round(median(ev["union"]) / floor_union, 1), "select": round(median(ev["select"]), 5),
                            "clean_moments_borji": round(median(ev["score"]), 5)}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
