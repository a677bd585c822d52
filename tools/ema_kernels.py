"""Ten device-resident train steps per setting at the bench size (unet, 8 clips of 16x112x112) in one process, for
`rocprofv3 --kernel-trace --stats -- python tools/ema_kernels.py` (profiles/r13_ema_kernels.csv): Adam without and with
`set_ema(0.999)`, so that ema_kernel sits beside adam_kernel in one stats table.  From bytes alone (12 against 28 per element)
ema_kernel should take 12/28 of adam_kernel's time: a prediction printed beside the figures, not a gate.  `--time` instead
prints the wall time per step of each setting (no profiler), off / on / off / on in one process
(profiles/r13_ema_bench.json)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sap3d_tensorflow_amd import P3DSession, synthetic      # noqa: E402

B, T, S, STEPS = 8, 16, 112, 10


def main():
    timed = "--time" in sys.argv[1:]
    s = P3DSession("unet", batch=B, frames=T, height=S, width=S, seed=1)
    s.upload(synthetic.synthetic_clip(0, (B, T, S, S, 3)), synthetic.synthetic_target(3, (B, T, S, S)))      # bench.py's inputs
    s.set_adam(1e-9)          # the weights stay where they are: every setting sees the same work
    out = []
    for decay in ((None, 0.999, None, 0.999) if timed else (None, 0.999)):
        s.set_ema(decay)
        for rep in range(2 if timed else 1):          # timed: the first pass warms up
            s.synchronize()
            t0 = time.perf_counter()
            for i in range(STEPS):
                s.train_step_device(0.5, seed=i)
            s.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / STEPS
        print("ema", decay, "loss", s.last_loss(), ("%.3f ms/step" % ms) if timed else "", flush=True)
        out.append({"ema_decay": decay, "steps": STEPS, "ms_per_step": round(ms, 3)})
    if timed:
        print(json.dumps({"tool": "tools/ema_kernels.py --time", "settings": out}))
    else:
        print("prediction from bytes: ema_kernel = 12/28 = %.3f of adam_kernel's time per launch" % (12.0 / 28.0))
    s.close()


if __name__ == "__main__":
    main()
