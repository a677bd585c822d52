"""Device-resident train steps at the bench size (unet, 8 clips of 16x112x112) in one process, for
`rocprofv3 --kernel-trace --stats -- python tools/grad_accum_kernels.py` (profiles/r14_grad_accum_kernels.csv): Adam with
`set_ema(0.999)` throughout, ten plain steps and then ten cycles of `set_grad_accum(3)`, so that the three modes of
grad_accum_kernel sit beside adam_kernel and ema_kernel in one stats table.  From bytes alone (8 and 12 against Adam's 28 per
element) STORE should take 0.29 and ADD / FINISH 0.43 of adam_kernel's time over the same range, and ADD / FINISH what ema_kernel
takes: predictions printed beside the figures, not gates.  `--time` instead prints wall times (no profiler), off / on / off / on
in one process (profiles/r14_grad_accum_bench.json): per step pipelined, and of single steps each followed by a synchronize,
where an accumulating micro-step and an applying one can be told apart."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sap3d_tensorflow_amd import P3DSession, synthetic      # noqa: E402

B, T, S, STEPS, K = 8, 16, 112, 10, 3


def pipelined(s, n):
    s.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        s.train_step_device(0.5, seed=i)
    s.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def single(s, n):
    """[(pending before the step, ms)] of n steps, each waited for."""
    out = []
    for i in range(n):
        j = s.grad_accum[1]
        s.synchronize()
        t0 = time.perf_counter()
        s.train_step_device(0.5, seed=i)
        s.synchronize()
        out.append((j, (time.perf_counter() - t0) * 1e3))
    return out


def mean(v):
    return round(sum(v) / len(v), 3) if v else None


def main():
    timed = "--time" in sys.argv[1:]
    s = P3DSession("unet", batch=B, frames=T, height=S, width=S, seed=1)
    s.upload(synthetic.synthetic_clip(0, (B, T, S, S, 3)), synthetic.synthetic_target(3, (B, T, S, S)))      # bench.py's inputs
    s.set_adam(1e-9)          # the weights stay where they are: every setting sees the same work
    if not timed:
        s.set_ema(0.999)
        for k, n in ((1, STEPS), (K, STEPS * K)):
            s.set_grad_accum(k)
            for i in range(n):
                s.train_step_device(0.5, seed=i)
            s.synchronize()
            print("grad_accum", k, "steps", n, "loss", s.last_loss(), "updates", s.optimizer_step(), flush=True)
        print("prediction from bytes, per element of the range: STORE 8/28 = %.3f, ADD and FINISH 12/28 = %.3f of adam_kernel; "
              "ADD and FINISH = ema_kernel" % (8.0 / 28.0, 12.0 / 28.0))
        s.close()
        return
    out = []
    for k in (1, K, 1, K):
        s.set_grad_accum(k)
        pipelined(s, k * 2)                                   # warm-up, whole cycles
        ms = pipelined(s, STEPS * k)
        one = single(s, STEPS * k)
        rec = {"grad_accum": k, "steps": STEPS * k, "ms_per_step": round(ms, 3)}
        if k == 1:
            rec["ms_single_step"] = mean([t for _, t in one])
        else:
            rec["ms_single_accumulating"] = mean([t for j, t in one if j < k - 1])
            rec["ms_single_applying"] = mean([t for j, t in one if j == k - 1])
        print(rec, flush=True)
        out.append(rec)
    print(json.dumps({"tool": "tools/grad_accum_kernels.py --time", "settings": out}))
    s.close()


if __name__ == "__main__":
    main()
