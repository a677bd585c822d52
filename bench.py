#!/usr/bin/env python3
"""Headline benchmark: clips/s of the P3D (p3d_unet) train step -- forward + Smooth-L1 loss +
backward + Adam -- on synthetic 16x112x112x3 clips, batch 8 per GPU, fp32, on N MI355X.

  python bench.py --gpus N --steps K --warmup W          (N > 1: starts the N ranks itself, as a child process)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One rank per GPU; each rank owns its shard of clips (weak scaling) and the only exchange is the
gradient all-reduce (RCCL, inside libp3dhip).  Rank 0 prints ONE JSON line.  Inputs are resident
in HBM before the timed region.  After the timed region rank 0 runs one extra, untimed step with
HIP events around every kernel launch (on the launch stream) to fill `roofline`, and -- at N=1
only -- times the numpy oracle on the host cores for `cpu_baseline`.

--dump-outputs DIR: rank 0 writes what the last timed step computed (dump_outputs) as DIR/<name>.npy, before
the untimed steps above run.  Inputs, initial weights and dropout seeds are fixed by the arguments, so two
builds run with the same arguments can be compared output for output; two runs of one build agree bit for
bit (tests/test_gpu_determinism.py).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP32_TFLOPS = 157.3      # MI355X_MICROARCH.md: fp32 vector == fp32 MFMA peak
PEAK_FP16_TFLOPS = 2500.0     # dense fp16 MFMA (MI355X_MICROARCH.md; the headline 5 PF is with 2:1 sparsity)
PEAK_HBM_GBS = 8000.0         # MI355X_MICROARCH.md: HBM3E spec (6.3 TB/s achievable)
FLOP_PER_CLIP_FWD_BWD = 98.59e9   # algorithmic conv/deconv FLOPs per clip
DUMP_CAP_FLOATS = (64 << 20) // 4  # --dump-outputs: at most 64 MB of float32 in all


def dump_sample(a, cap, seed):
    """`a` as float32 when it has at most `cap` elements; otherwise a fixed, seeded sample of `cap` of its elements (flat, in
    index order), the same on every run and every build."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.size <= cap:
        return a
    idx = np.sort(np.random.Generator(np.random.PCG64(seed)).choice(a.size, cap, replace=False))
    return a.reshape(-1)[idx]


def dump_outputs(sess, loss, out_dir):
    """What a caller of the timed train step receives from its last step: the loss, the prediction of its forward pass and the
    variables it left behind (Adam-updated trainables and BatchNorm moving statistics, flattened and concatenated in creation
    order).  float32 .npy files; the prediction gets a quarter and the variables half of DUMP_CAP_FLOATS, sampled when larger."""
    os.makedirs(out_dir, exist_ok=True)
    variables = np.concatenate([sess.get_param(n).reshape(-1) for n, _, _ in sess.variables()])
    outs = {"loss": np.array([loss], np.float32),
            "pred": dump_sample(sess.activation("pred"), DUMP_CAP_FLOATS // 4, seed=1),
            "variables": dump_sample(variables, DUMP_CAP_FLOATS // 2, seed=2)}
    for name, a in outs.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def kernel_table(recs):
    """Aggregate per-launch HIP-event records by kernel symbol."""
    agg = {}
    for r in recs:
        a = agg.setdefault(r["kernel"], dict(kernel=r["kernel"], launches=0, ms=0.0, flops=0.0, bytes=0.0))
        a["launches"] += 1
        a["ms"] += r["ms"]
        a["flops"] += r["flops"]
        a["bytes"] += r["bytes"]
    rows = sorted(agg.values(), key=lambda a: -a["ms"])
    for a in rows:
        a["avg_us"] = 1e3 * a["ms"] / a["launches"]
        a["tflops"] = a["flops"] / (a["ms"] * 1e-3) / 1e12 if a["ms"] > 0 else 0.0
        a["gbs"] = a["bytes"] / (a["ms"] * 1e-3) / 1e9 if a["ms"] > 0 else 0.0
    return rows


def per_layer_table(recs):
    """Per reference layer (stem, pool*, bottleneck i, deconv j, head, loss, optimiser): device time,
    algorithmic FLOPs and bytes of its launches (forward + backward), the roofline that bounds it and the fraction reached.
    A grouped filter-gradient launch is booked on the layer whose backward flushed it."""
    import re
    order, agg = [], {}
    for r in recs:
        name = r["name"]
        layer = name.split("/")[0] if name else "op"
        layer = re.sub(r"_bn$", "", layer)
        if layer not in agg:
            order.append(layer)
            agg[layer] = dict(layer=layer, launches=0, ms=0.0, flops=0.0, bytes=0.0)
        a = agg[layer]
        a["launches"] += 1; a["ms"] += r["ms"]; a["flops"] += r["flops"]; a["bytes"] += r["bytes"]
    rows = []
    ridge = PEAK_FP32_TFLOPS * 1e12 / (PEAK_HBM_GBS * 1e9)
    for layer in order:
        a = agg[layer]
        t = max(a["ms"], 1e-9) * 1e-3
        tf, gb = a["flops"] / t / 1e12, a["bytes"] / t / 1e9
        bound = "mfma" if a["flops"] / max(a["bytes"], 1.0) >= ridge else "hbm"
        # time the layer would need at both roofs; the larger one bounds it
        t_roof = max(a["flops"] / (PEAK_FP32_TFLOPS * 1e12), a["bytes"] / (PEAK_HBM_GBS * 1e9))
        rows.append(dict(layer=layer, launches=a["launches"], ms=round(a["ms"], 4), gflop=round(a["flops"] / 1e9, 3), mbytes=round(a["bytes"] / 1e6, 3),
                         tflops=round(tf, 2), gbs=round(gb, 1), bound=bound, frac=round(t_roof / t, 4)))
    return rows


def measured_traffic(kernel):
    """HBM-side bytes per launch of `kernel` from the committed PMC passes (profiles/*_traffic.json), or None."""
    import glob
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_traffic.json"))):
        try:
            k = json.load(open(f))["kernels"].get(kernel.replace("(grouped)", ""))
        except Exception:
            k = None
        if k:
            best = k["traffic_bytes_per_launch"]
    return best


def roofline_of(rows):
    """The dominant kernel (largest share of device time) against the roofline that bounds it."""
    top = rows[0]
    ai = top["flops"] / max(top["bytes"], 1.0)
    # kernels tagged f16 (--pointwise fp16) multiply on the fp16 matrix cores: price them against the dense fp16 peak
    mfma_peak = PEAK_FP16_TFLOPS if "f16" in top["kernel"] else PEAK_FP32_TFLOPS
    if ai >= mfma_peak * 1e12 / (PEAK_HBM_GBS * 1e9):
        bound, achieved, peak, unit = "mfma", top["tflops"], mfma_peak, "TFLOP/s"
    else:
        bound, achieved, peak, unit = "hbm", top["gbs"], PEAK_HBM_GBS, "GB/s"
    return dict(kernel=top["kernel"], bound=bound, achieved=round(achieved, 3), peak=peak, unit=unit,
                frac=round(achieved / peak, 4), traffic=measured_traffic(top["kernel"]), launches_per_step=top["launches"],
                avg_launch_us=round(top["avg_us"], 2),
                flop_per_launch=round(top["flops"] / top["launches"]), bytes_per_launch=round(top["bytes"] / top["launches"]),
                share_of_device_time=round(top["ms"] / sum(r["ms"] for r in rows), 4))


def usable_cores():
    """Host cores this process may really use: CPU affinity capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0))
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                if q > 0:
                    per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                    n = min(n, max(1, q // per))
        except Exception:
            pass
    return n


def cpu_baseline():
    """The CPU baseline, timed on this box's host cores in child processes (`python -m oracle.cpu_time`, the only use of
    oracle/ here): the torch-CPU (oneDNN) composition of the same train step -- the stronger stand-in for the reference's
    TF-CPU path, BASELINE.md section 3 -- on a bounded sample of 16 clips (one batch), and the numpy restatement on 2 clips next to it.
    The faster one is reported; both are restatements ("port"): the reference itself cannot run."""
    import subprocess
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    results = []
    for kind, clips in (("torch", 16), ("numpy", 2)):
        try:
            out = subprocess.run([sys.executable, "-m", "oracle.cpu_time", kind, str(clips)], cwd=ROOT, env=env, capture_output=True,
                                 text=True, timeout=900)
            results.append(json.loads(out.stdout.strip().splitlines()[-1]))
        except Exception as e:          # a missing torch must not cost the bench line
            results.append(dict(value=0.0, unit="clips/s", cores=usable_cores(), kind="port", sample="%s leg failed: %r" % (kind, e)))
    best = max(results, key=lambda r: r["value"])
    other = [r for r in results if r is not best][0]
    best = dict(best)
    best.pop("seconds", None)
    best["also"] = "%s -> %.3f clips/s" % (other["sample"], other["value"])
    return best


def launch_ranks(n, argv):
    """`python bench.py --gpus N` without a torch.distributed.run environment: start
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N bench.py <same arguments>` as a child process on a free
    local port, pass its output through (rank 0 prints the ONE JSON line) and return its exit code."""
    import subprocess
    # --standalone: torch.distributed.run picks a free rendezvous port itself (a port found here by bind-and-close could be taken by
    # another job on the host before the ranks bind it: ADVICE round 4); --local-addr: the container hostname may not resolve
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1", "--nproc-per-node", str(n),
           os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    env.setdefault("OMP_NUM_THREADS", "1")
    return subprocess.run(cmd, env=env, cwd=ROOT).returncode


def pick_device(local_rank, visible):
    """The device ordinal of this rank: LOCAL_RANK when the launcher shows every rank all the node's GPUs (torch.distributed.run), 0 when it
    shows each rank exactly one (per-rank HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES).  Anything else cannot give one GPU per rank."""
    if visible > local_rank or visible < 0:          # (< 0: the runtime could not say -- the launcher's convention)
        return local_rank
    if visible == 1:
        return 0
    raise SystemExit("LOCAL_RANK %d but this process sees %d GPU(s): launch one rank per GPU" % (local_rank, visible))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8, help="clips per GPU (BASELINE.json config: batch 8 per MI355X)")
    ap.add_argument("--structure", default="unet", choices=["unet", "concat", "gn_p3d", "unet++nonsa", "gn_p3d_decoder", "gn_p3d_concat", "unet++ds"],
                    help="graph to time (default: the BASELINE.json headline, p3d_unet)")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=112, help="clip height = width (BASELINE configs[4] uses 32 frames of 224)")
    ap.add_argument("--pointwise", default="fp32", choices=["fp32", "fp16"],
                    help="fp16: 1x1x1 convs on the fp16 MFMA with fp32 accumulate (BASELINE configs[4]); fp16-level parity")
    ap.add_argument("--attention", default="auto", choices=["auto", "gemm", "flash"],
                    help="unet++ds: how the attention cores run (p3d_set_attention_mode)")
    ap.add_argument("--bn-fusion", default="default", choices=["default", "off", "fwd", "full"],
                    help="A/B runs: BatchNorm passes of their own / fused into the convs in the forward pass / in both passes")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--kernels", action="store_true", help="also print the per-kernel table to stderr")
    ap.add_argument("--dump-launches", default=None, help="write every launch record of the profiled step to this CSV")
    ap.add_argument("--per-layer", default=None, help="write the per-layer roofline table of the profiled step to this CSV")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the loss, prediction and variables of the last timed step to DIR/<name>.npy (float32, <= 64 MB)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # bare `python bench.py --gpus N`: this process has not touched the GPU yet; it only starts the N ranks as a CHILD
        # (never an exec) and relays rank 0's JSON line and the child's exit code
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:]))

    from sap3d_tensorflow_amd.dp import Plane
    plane = Plane()
    world, rank, local_rank = plane.world, plane.rank, plane.local_rank
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: launch with torch.distributed.run --nproc-per-node %d" %
                         (args.gpus, world, args.gpus))

    from sap3d_tensorflow_amd import P3DSession
    from sap3d_tensorflow_amd import synthetic

    B = args.batch
    T, S = args.frames, args.size
    # Rehearsal of the multi-process launch on a ONE-GPU box (torch.distributed.run, rendezvous, barriers, rank-0 output):
    # every rank uses device 0 and no RCCL communicator is built (RCCL refuses two ranks on one device), so gradients
    # stay local.  The printed value is meaningless and says so.
    rehearsal = os.environ.get("P3D_BENCH_REHEARSAL") == "1"
    device = 0 if rehearsal else pick_device(local_rank, P3DSession.device_count())
    sess = P3DSession(args.structure, batch=B, frames=T, height=S, width=S, device=device, world_size=world, rank=rank, seed=1)
    if args.pointwise == "fp16":
        sess.set_pointwise_fp16(True)
    if args.attention != "auto":
        sess.set_attention_mode(args.attention)
    if args.bn_fusion != "default":
        sess.set_bn_fusion({"off": 0, "fwd": 1, "full": 2}[args.bn_fusion])
    rccl_ranks = None
    if world > 1 and not rehearsal:
        sess.comm_init(plane.share_from_rank0(P3DSession.comm_unique_id))
        # what RCCL itself says: every rank must sit in ONE communicator of `world` ranks, with its own rank number, on its own GPU
        n, r, d = sess.comm_info()
        if (n, r, d) != (world, rank, device):
            raise SystemExit("rank %d: RCCL communicator has %d ranks (this one: %d, device %d), expected %d / %d / %d" %
                             (rank, n, r, d, world, rank, device))
        rccl_ranks = n
    x = synthetic.synthetic_clip(rank, (B, T, S, S, 3))
    y = synthetic.synthetic_target(3 + rank, (B, T, S, S))
    sess.upload(x, y)

    for i in range(args.warmup):
        sess.train_step_device(0.5, seed=i)
    sess.synchronize()
    plane.barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        sess.train_step_device(0.5, seed=1000 + i)
    t_enqueued = time.perf_counter() - t0          # host-side launch time (the GPU runs behind it)
    sess.synchronize()
    plane.barrier()
    dt = plane.max_over_ranks(time.perf_counter() - t0)
    loss = sess.last_loss()
    if args.dump_outputs:
        if rank == 0:              # before any untimed step changes the variables
            dump_outputs(sess, loss, args.dump_outputs)
        plane.barrier()            # the other ranks wait, so that the dump stays out of their one-step timing below
    # host cost of enqueueing ONE step into empty queues (no back-pressure from a full hardware queue, unlike t_enqueued)
    t1 = time.perf_counter()
    sess.train_step_device(0.5, seed=999_999)
    t_one = time.perf_counter() - t1
    sess.synchronize()
    plane.barrier()
    t_one_max = plane.max_over_ranks(t_one)        # the slowest rank's host: what N ranks on one host's cores cost each other

    if rank == 0:
        ms = 1e3 * dt / args.steps
        value = world * B * args.steps / dt
        recs = sess.profile_step(0.5, seed=7)
        rows = kernel_table(recs)
        if args.dump_launches:
            with open(args.dump_launches, "w") as f:
                f.write("op,kernel,phase,ms,flops,bytes\n")
                for r in recs:
                    f.write("%s,\"%s\",%d,%.5f,%.0f,%.0f\n" % (r["name"], r["kernel"], r["phase"], r["ms"], r["flops"], r["bytes"]))
        if args.per_layer:
            rows_l = per_layer_table(recs)
            with open(args.per_layer, "w") as f:
                f.write("layer,launches,ms,gflop,mbytes,tflops,gbs,bound,frac_of_roofline\n")
                for r in rows_l:
                    f.write("%s,%d,%.4f,%.3f,%.3f,%.2f,%.1f,%s,%.4f\n" % (r["layer"], r["launches"], r["ms"], r["gflop"], r["mbytes"], r["tflops"],
                                                                          r["gbs"], r["bound"], r["frac"]))
        out = {
            "metric": "clips/s (16x112x112 fwd+bwd)", "value": round(value, 2), "unit": "clips/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            **({"rehearsal": "all ranks on device 0, no all-reduce: NOT a measurement"} if rehearsal else {}),
            "dtype": "f32" if args.pointwise == "fp32" else "f32 (1x1x1 convs: fp16 MFMA operands, f32 accumulate)", "data": "synthetic",
            "config": {"workload": "%s train step: fwd + Smooth-L1 + bwd + Adam, %dx%dx%dx3 clips, batch %d per GPU (%s)" %
                                   ({"unet": "p3d_unet (P3D-199 encoder + unet decoder)", "concat": "p3d_concat",
                                     "gn_p3d": "p3d_gn.inference_p3d (GroupNorm + CBAM)",
                                     "unet++nonsa": "p3d_unetplusplus_nonsa (nested UNet++ head, no attention)",
                                     "gn_p3d_decoder": "p3d_gn.inference_p3d_decoder_block (GroupNorm + CBAM, decoder blocks)",
                                     "gn_p3d_concat": "p3d_gn.inference_p3d_concat (GroupNorm + CBAM)",
                                     "unet++ds": "p3d_unetplusplus_ds (nested UNet++ head with self attention)"}[args.structure], T, S, S, B,
                                    {"unet": "BASELINE.json configs[2]", "gn_p3d": "BASELINE.json configs[3] graph, 1 GPU"}.get(args.structure, "SURVEY.md row N2" if args.structure == "unet++ds" else "SURVEY.md row N1")),
                       "global_batch": world * B, "parallelism": "dp%d" % world, "dropout": 0.5},
            "model_tflops": round(value * FLOP_PER_CLIP_FWD_BWD * (T / 16.0) * (S / 112.0) ** 2 / 1e12, 2) if args.structure == "unet" else None,
            "final_loss": loss,
            "bn_fusion": args.bn_fusion, "attention": args.attention,
            "launches_per_step": len(recs),
            **({"rccl_ranks": rccl_ranks} if world > 1 else {}),
            "host_enqueue_ms_per_step": round(1e3 * t_enqueued / args.steps, 3),
            "host_enqueue_ms_one_step_empty_queue": round(1e3 * t_one, 3),
            "host_enqueue_ms_one_step_empty_queue_max_over_ranks": round(1e3 * t_one_max, 3),
            "roofline": roofline_of(rows),
            "kernels": [dict(kernel=r["kernel"], launches=r["launches"], ms=round(r["ms"], 3), avg_us=round(r["avg_us"], 2),
                             tflops=round(r["tflops"], 2), gbs=round(r["gbs"], 1)) for r in rows[:12]],
        }
        if world == 1 and not args.no_cpu_baseline and args.structure == "unet" and (T, S) == (16, 112):
            out["cpu_baseline"] = cpu_baseline()
        if args.kernels:
            for r in rows:
                print("%-28s n=%5d  %9.3f ms  avg %8.2f us  %7.2f TF/s  %8.1f GB/s" %
                      (r["kernel"], r["launches"], r["ms"], r["avg_us"], r["tflops"], r["gbs"]), file=sys.stderr)
        print(json.dumps(out), flush=True)
    plane.barrier()        # rank 0 profiles and prints while the others wait: tear the communicators down together
    sess.close()
    plane.close()


if __name__ == "__main__":
    main()
