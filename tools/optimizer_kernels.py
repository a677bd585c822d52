"""Ten device-resident train steps under each optimiser (Adam, Momentum, SGD) at the bench size (unet, 8 clips of 16x112x112) in
one process, for `rocprofv3 --kernel-trace --stats -- python tools/optimizer_kernels.py` (profiles/r08_optimizer_kernels.csv):
adam_kernel, momentum_kernel and sgd_kernel sit side by side in one stats table.  Prints one line per optimiser with its last
step's loss."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sap3d_tensorflow_amd import P3DSession, synthetic      # noqa: E402

B, T, S, STEPS = 8, 16, 112, 10


def main():
    s = P3DSession("unet", batch=B, frames=T, height=S, width=S, seed=1)
    s.upload(synthetic.synthetic_clip(0, (B, T, S, S, 3)), synthetic.synthetic_target(3, (B, T, S, S)))      # bench.py's inputs
    for kind in ("adam", "momentum", "sgd"):
        s.set_optimizer(kind, lr=1e-4, momentum=0.9)
        for i in range(STEPS):
            s.train_step_device(0.5, seed=i)
        s.synchronize()
        print(kind, s.last_loss(), flush=True)
    s.close()


if __name__ == "__main__":
    main()
