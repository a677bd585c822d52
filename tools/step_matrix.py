"""Every loss (smooth_l1, bce, l1, kld_cc) x optimiser (adam, momentum, momentum+nesterov, sgd) x regularisation (off, weight
decay) on unet at the bench size (8 clips of 16x112x112), plus gn_p3d_decoder with L2 (the only net with L2 variables), unet++ds
(the attention blocks' mixing pass, the transposed head) and gn_p3d (every GroupNorm mode, CBAM): three device-resident train
steps from the same seed each, then one line with the combination, repr of the last loss and a SHA-256 over every variable and
optimiser slot.  Two builds of the library (P3D_LIB=<path>) that compute the same print the same lines."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sap3d_tensorflow_amd import P3DSession, synthetic      # noqa: E402

B, T, S, STEPS = 8, 16, 112, 3
LOSSES = ("smooth_l1", "bce", "l1", "kld_cc")
OPTIMIZERS = (("adam", False), ("momentum", False), ("momentum", True), ("sgd", False))


def run(structure, loss, opt, nesterov, terms):
    s = P3DSession(structure, batch=B, frames=T, height=S, width=S, seed=1)
    s.upload(synthetic.synthetic_clip(0, (B, T, S, S, 3)), synthetic.synthetic_target(3, (B, T, S, S)))      # bench.py's inputs
    s.set_loss(loss)
    s.set_optimizer(opt, lr=1e-4, momentum=0.9, use_nesterov=nesterov)
    s.set_regularization(terms)
    for i in range(STEPS):
        s.train_step_device(0.5, seed=i)
    s.synchronize()
    h = hashlib.sha256()
    for name, _, _ in s.variables():
        h.update(s.get_param(name).tobytes())
    for _, slot in sorted(s.optimizer_state().items()):
        h.update(slot.tobytes())
    print(structure, loss, opt + ("+nesterov" if nesterov else ""), "+".join(terms) or "none", repr(s.last_loss()), h.hexdigest(),
          flush=True)
    s.close()


def main():
    for loss in LOSSES:
        for opt, nesterov in OPTIMIZERS:
            for terms in ((), ("weightdecay",)):
                run("unet", loss, opt, nesterov, terms)
    run("gn_p3d_decoder", "smooth_l1", "adam", False, ("l2",))
    run("unet++ds", "smooth_l1", "adam", False, ())
    run("gn_p3d", "smooth_l1", "adam", False, ())


if __name__ == "__main__":
    main()
