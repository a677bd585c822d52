"""Ten device-resident train steps per setting at the bench size (unet, 8 clips of 16x112x112) in one process, for
`rocprofv3 --kernel-trace --stats -- python tools/grad_clip_kernels.py` (profiles/r11_grad_clip_kernels.csv): Adam, Momentum and
SGD without clipping and with `set_grad_clip(inf)` (measure only: the same launches as any threshold), so that grad_sumsq_kernel
and the scaled optimiser launches sit beside the unscaled ones in one stats table.  `--time` instead prints the wall time per
step of each setting (no profiler): the price of the first optimiser part's lost overlap."""
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
    for opt in ("adam", "momentum", "sgd"):
        s.set_optimizer(opt, lr=1e-9)          # the weights stay where they are: every setting sees the same work
        for clip in (0.0, float("inf")):
            s.set_grad_clip(clip)
            for rep in range(2 if timed else 1):          # timed: the first pass warms up
                s.synchronize()
                t0 = time.perf_counter()
                for i in range(STEPS):
                    s.train_step_device(0.5, seed=i)
                s.synchronize()
                ms = (time.perf_counter() - t0) * 1e3 / STEPS
            tail = ("gnorm %.9g scale %.9g" % s.last_grad_norm()) if clip else ""
            print(opt, "clip", clip, "loss", s.last_loss(), ("%.3f ms/step" % ms) if timed else "", tail, flush=True)
    s.close()


if __name__ == "__main__":
    main()
