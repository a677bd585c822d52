"""Ten device-resident train steps per loss (smooth_l1, bce, l1, kld_cc) at the bench size (unet, 8 clips of 16x112x112) in one
process, for `rocprofv3 --kernel-trace --stats -- python tools/loss_kernels.py` (profiles/r06_loss_kernels.csv;
profiles/r07_map_loss_kernels.csv with kld_cc): the loss launches sit side by side in one stats table.  Prints one line per loss with its last step's loss."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sap3d_tensorflow_amd import P3DSession, synthetic      # noqa: E402

B, T, S, STEPS = 8, 16, 112, 10


def main():
    s = P3DSession("unet", batch=B, frames=T, height=S, width=S, seed=1)
    s.upload(synthetic.synthetic_clip(0, (B, T, S, S, 3)), synthetic.synthetic_target(3, (B, T, S, S)))      # bench.py's inputs
    for name in ("smooth_l1", "bce", "l1", "kld_cc"):
        s.set_loss(name)
        for i in range(STEPS):
            s.train_step_device(0.5, seed=i)
        s.synchronize()
        print(name, s.last_loss(), flush=True)
    s.close()


if __name__ == "__main__":
    main()
