"""Device time of the signal of gradual transitions beside the cut signal's (dataflow.transitions_time, p3d_debug_transitions_time):
128 frames at 1080 x 1920 -- two chunks of tables, so the carry of K tables is copied once -- and 64 at 112 x 112, resident on the
device, lags 12 and 64, a 4 x 4 grid.  The two alternate, REPS rounds after one warm-up round, HIP events around each.  Frames: a
smooth scene that drifts, with noise of +-2, as decoded video is.  Writes profiles/transitions_signal.json (--out): per case the
medians and extremes in ms and the ratio of the new signal's median to the cut signal's.  A report: nothing is asserted but that
both give the same D."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sap3d_tensorflow_amd import dataflow      # noqa: E402

REPS = 20
CASES = [(64, 112, 112), (128, 1080, 1920)]
LAGS = [12, 64]
GRID = (4, 4)


def frames_of(n, H, W):
    rng = np.random.default_rng([n, H, W])
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    base = np.stack([128. + 100. * np.sin(yy / H * (2. + k)) * np.cos(xx / W * (3. - k)) for k in range(3)], axis=-1).astype(np.int16)
    out = np.empty((n, H, W, 3), np.uint8)
    for f in range(n):
        out[f] = np.clip(np.roll(base, 2 * f, axis=1) + rng.integers(-2, 3, (H, W, 3), dtype=np.int16), 0, 255)
    return out


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transitions_signal.json"))
    ap.add_argument("--reps", type=int, default=REPS)
    a = ap.parse_args()
    cases = []
    for n, H, W in CASES:
        frames = frames_of(n, H, W)
        for lag in LAGS:
            assert np.array_equal(dataflow.shot_signals_u8(frames[:lag + 2], GRID, lag)[0], dataflow.shot_distances(frames[:lag + 2], GRID))
            cut, signal = dataflow.transitions_time(frames, GRID, lag, a.reps)
            row = dict(frames=n, H=H, W=W, grid=list(GRID), lag=lag, bytes=int(frames.nbytes), plan=dataflow.transitions_plan(H, W, GRID, n, lag),
                       cut=stats(cut), signal=stats(signal))
            row["signal_over_cut"] = row["signal"]["median_ms"] / row["cut"]["median_ms"]
            cases.append(row)
            print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/transitions_time.py", reps=a.reps, note="cut: the launches of p3d_shot_distances_u8; signal: those of p3d_shot_signals_u8", cases=cases),
                  f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
