"""HIP-event time of the training set's stage at the benchmark's clip shape (8 x 16 x 112 x 112), both frame formats, beside the three
host uploads it replaces (p3d_upload_inputs + p3d_upload_fixations): medians of 25 after 5 warm-up calls -> profiles/trainset_time.json
(or the path given as the first argument)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sap3d_tensorflow_amd import P3DSession, _lib      # noqa: E402

B, T, S = 8, 16, 112
sess = P3DSession("unet", batch=B, frames=T, height=S, width=S, base=16, blocks=(1, 1, 1), seed=1)
hip = C.CDLL(_lib.mapped_rocm_runtimes()["libamdhip64"][0])
ev = [C.c_void_p(), C.c_void_p()]
for e in ev:
    assert hip.hipEventCreate(C.byref(e)) == 0
rng = np.random.default_rng(0)
videos = [300, 300, 300, 300]
F = sum(videos)
bgr = rng.integers(0, 256, (F, S, S, 3)).astype(np.uint8)
den = rng.integers(0, 256, (F, S, S)).astype(np.uint8)
fix = (rng.random((F, S, S)) < 0.01).astype(np.uint8) * 255
out = {"shape": [B, T, S, S], "videos": videos}
for fmt in ("u8", "f32"):
    sess.open_trainset(videos, frame_format=fmt, fixations=True)
    at = 0
    for v, n in enumerate(videos):
        for i in range(0, n, 100):
            sess.trainset_put_frames_u8(v, i, bgr[at + i:at + i + 100])
            sess.trainset_put_density_u8(v, i, den[at + i:at + i + 100])
            sess.trainset_put_fixations(v, i, fix[at + i:at + i + 100])
        at += n
    ms, wall = [], []
    for it in range(30):
        clips = [(int(rng.integers(0, 4)), int(rng.integers(0, 300 - T + 1))) for _ in range(B)]
        t0 = time.perf_counter()
        sess.trainset_stage(clips)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(sess.trainset_last_ms())
    out["stage_" + fmt] = {"event_ms_median": float(np.median(ms[5:])), "event_ms_min": float(np.min(ms[5:])),
                           "wall_ms_median": float(np.median(wall[5:])), "bytes": sess.trainset_info()["bytes"]}
    print(fmt, out["stage_" + fmt], flush=True)
sess.close_trainset()
x = rng.standard_normal((B, T, S, S, 3)).astype(np.float32)
y = rng.random((B, T, S, S)).astype(np.float32)
f = fix[:B * T].reshape(B, T, S, S).copy()
evms, wall = [], []
for it in range(30):
    hip.hipEventRecord(ev[0], None)
    t0 = time.perf_counter()
    sess.upload(x, y, f)
    wall.append((time.perf_counter() - t0) * 1e3)
    hip.hipEventRecord(ev[1], None)
    hip.hipEventSynchronize(ev[1])
    t = C.c_float()
    assert hip.hipEventElapsedTime(C.byref(t), ev[0], ev[1]) == 0
    evms.append(t.value)
out["uploads"] = {"event_ms_median": float(np.median(evms[5:])), "event_ms_min": float(np.min(evms[5:])), "wall_ms_median": float(np.median(wall[5:])),
                  "bytes": int(x.nbytes + y.nbytes + f.nbytes), "host_memory": "pageable numpy arrays"}
print("uploads", out["uploads"], flush=True)
sess.close()
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "trainset_time.json")
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
