"""Device time of the cut signal of csrc/shots.hip (dataflow.shots_time, p3d_debug_shots_time): 64 frames at 112 x 112 and at
1080 x 1920, resident on the device, counted without and with ballot aggregation, beside a device-to-device copy of the same bytes
in the same process -- the roof of a kernel that reads every byte once.  The three alternate, REPS rounds after one warm-up round,
HIP events around each.  Two kinds of frames: uniform noise (every bin equally likely: the fewest equal bins in a wave) and a
smooth scene (a slow gradient with noise of +-2, as decoded video is: neighbouring bytes share bins).  Writes
profiles/shots_signal.json (--out): per case the median and the extremes in ms, GB/s over the n H W 3 bytes read, and the ratio of
the copy's time to the signal's.  A report: nothing is asserted but that both ways of counting give the same D."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sap3d_tensorflow_amd import dataflow      # noqa: E402

N, REPS = 64, 20
SIZES = [(112, 112), (1080, 1920)]
GRIDS = [(1, 1), (4, 4)]


def frames_of(kind, n, H, W):
    rng = np.random.default_rng([n, H, W])
    if kind == "noise":
        return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.empty((n, H, W, 3), np.uint8)
    for f in range(n):
        for k in range(3):
            g = 128. + 100. * np.sin(yy / H * (2. + k) + 0.05 * f) * np.cos(xx / W * (3. - k) + 0.03 * f)
            out[f, :, :, k] = np.clip(np.rint(g + rng.integers(-2, 3, (H, W))), 0, 255).astype(np.uint8)
    return out


def stats(ms, nbytes):
    med = float(np.median(ms))
    return dict(median_ms=med, min_ms=float(ms.min()), max_ms=float(ms.max()), gb_per_s=nbytes / med / 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shots_signal.json"))
    ap.add_argument("--frames", type=int, default=N)
    ap.add_argument("--reps", type=int, default=REPS)
    a = ap.parse_args()
    cases = []
    for H, W in SIZES:
        for kind in ("noise", "scene"):
            frames = frames_of(kind, a.frames, H, W)
            for grid in GRIDS:
                assert np.array_equal(dataflow.shot_distances(frames[:3], grid, offset=0, ballot=0),
                                      dataflow.shot_distances(frames[:3], grid, offset=0, ballot=1))
                plain, ballot, copy = dataflow.shots_time(frames, grid, a.reps)
                row = dict(frames=a.frames, H=H, W=W, kind=kind, grid=list(grid), bytes=int(frames.nbytes), plan=dataflow.shots_plan(H, W, grid, a.frames),
                           plain=stats(plain, frames.nbytes), ballot=stats(ballot, frames.nbytes), copy=stats(copy, frames.nbytes))
                row["copy_over_plain"] = row["copy"]["median_ms"] / row["plain"]["median_ms"]
                row["copy_over_ballot"] = row["copy"]["median_ms"] / row["ballot"]["median_ms"]
                cases.append(row)
                print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/shots_time.py", reps=a.reps, note="copy: hipMemcpyAsync device to device of the same bytes (it reads and writes them)",
                       cases=cases), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
