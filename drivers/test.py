#!/usr/bin/env python3
"""Python-3 counterpart of the reference's evaluation program (/root/reference/test.py) on libp3dhip.

Restores a checkpoint, runs the test clips batch by batch through ONE plain batched forward with training False (test.py:160;
the backbone BatchNorm couples the clips of a batch, as in the reference -- not gen_pred's per-window predict_windows), and
scores the last frame of every clip at the fixation maps' resolution: CC, SIM, AUC_Judd, AUC_Borji, NSS (test.py:166-176),
all on the GPU (P3DSession.evaluate).  A trailing partial batch is dropped (BatchData(..., remainder=False), test.py:89).
It prints test.py's two line formats: the running means every 100 batches (test.py:161-163, NaN-including like np.mean of
the raw lists) and the NaN-dropped means at the end (test.py:177-183).

The reference walks JPEG folders and decodes them with cv2 (test.py:73-90, dataflow.py:219-241); that stays out of scope.
Here a test set is one .npz (--data) with
    x         [N,16,112,112,3] float32, already normalised -- or raw uint8 BGR frames [N,16,H0,W0,3] (as cv2.imread gives them),
              which go through the loader's pre-processing (sap3d_tensorflow_amd.dataflow.mapf_frames);
    density   uint8 [N,Hd,Wd] or [N,16,Hd,Wd] (cv2.IMREAD_GRAYSCALE images; resized to the fixation size on the GPU);
    fixation  uint8 [N,H,W] or [N,16,H,W] (H x W = 1080 x 960 in the reference).  Only the last frame is scored.
Without --data, a synthetic set (sap3d_tensorflow_amd.synthetic.synthetic_test_set) is used.

--sauc M adds a sixth column, shuffled AUC (utils/metrics.py:157-197) of the clean full-resolution prediction against the
union of the fixations of M other clips (Borji's M = 10).  It draws from its own np.random.RandomState(seed): the five
reference columns are identical with and without it.  With --sauc-device the column is computed inside the evaluation pass
(P3DSession.evaluate(shuffled=...); include/p3d_hip.h, "Shuffled AUC in the evaluation pass"): the set's fixation maps go into a
pool on the device once, one bit per pixel, and per batch the draws from RandomState(seed) are, in this order: for each clip of the
batch in clip order rng.choice(np.delete(arange(n), i), size=min(M, n - 1), replace=False); the union is taken on the device and
the clips' n_other come back; then for each clip in clip order, nothing when it has no fixation, else n_rep times
rng.permutation(n_other)[:n_fix].  (Without the flag the host path interleaves choice and permutations clip by clip: the two
orders coincide at --batch 1, where the sixth column is the same number, and differ in the draws -- not in the law -- above it.)
The scored map is the CLEAN map after the resize and every optional stage, so with --sauc-device --match-hist density is allowed:
each clip's map is the one matched to its own density, scored against the other clips' fixations.  --kldiv and --info-gain BASELINE.npy add KL divergence
(utils/metrics.py:338-362) and information gain over the baseline map (float32 [H, W] at the fixation maps' size) of the same
scored map, computed on the GPU in the same pass (P3DSession.set_eval_extra); their NaN-dropped means follow the other columns
on both lines, and the five reference columns are identical with and without them.  --time prints per batch: forward, host random draws, host->device
copy and the device metric stage."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_LINE = " Step: %d, Metrics: CC: %.3f  SIM: %.3f   NSS: %.3f  AUC_Judd: %.3f   AUC_Borji: %.3f"        # test.py:161-163
ALL_LINE = " All: %d, Metrics: CC: %.3f  SIM: %.3f   NSS: %.3f  AUC_Judd: %.3f   AUC_Borji: %.3f"          # test.py:182-183


def batches(n, batch):
    """[lo, hi) of every full batch: BatchData(..., remainder=False) drops a trailing partial batch (test.py:89)."""
    return [(lo, lo + batch) for lo in range(0, n - batch + 1, batch)]


def last_frame(maps):
    maps = np.asarray(maps)
    return maps[:, -1] if maps.ndim == 4 else maps


def load_set(path, device=0):
    d = np.load(path)
    x, density, fixation = d["x"], last_frame(d["density"]), last_frame(d["fixation"])
    if x.dtype == np.uint8:
        from sap3d_tensorflow_amd import dataflow
        n, t = x.shape[:2]
        x = dataflow.mapf_frames(x.reshape((n * t,) + x.shape[2:]), 112, device=device).reshape(n, t, 112, 112, 3)
    if density.dtype != np.uint8 or fixation.dtype != np.uint8:
        raise ValueError("density and fixation maps must be uint8 images")
    if not (len(x) == len(density) == len(fixation)):
        raise ValueError("x, density and fixation hold different numbers of clips")
    return np.asarray(x, np.float32), density, fixation


def nan_dropped_means(cols):
    """test.py:177-181: every metric's list without its NaNs, then the mean."""
    return [float(np.mean(np.asarray(c)[~np.isnan(c)])) for c in cols]


def metric_line(fmt, index, cols, extra=()):
    """cols in evaluate's order (CC, SIM, AUC_Judd, AUC_Borji, NSS [, sAUC]); the reference prints CC SIM NSS Judd Borji.
    extra: (label, value) of --kldiv / --info-gain, after everything else."""
    cc, sim, judd, borji, nss = cols[:5]
    line = fmt % (index, cc, sim, nss, judd, borji)
    if len(cols) > 5:
        line += "   sAUC: %.3f" % cols[5]
    for label, value in extra:
        line += "   %s: %.3f" % (label, value)
    return line


def nan_dropped_mean(c):
    """The mean of a list without its NaNs; NaN for a list that holds nothing else (the progress line's before the first batch)."""
    c = np.asarray(c, np.float64)
    c = c[~np.isnan(c)]
    return float(np.mean(c)) if c.size else float("nan")


def load_baseline(path, size):
    """--info-gain's map: float32 [H, W] of an .npy, of the fixation maps' size."""
    base = np.asarray(np.load(path), np.float32)
    if base.shape != tuple(size):
        raise ValueError("--info-gain: the baseline %s is %s, the fixation maps are %s" % (path, base.shape, tuple(size)))
    return base


def shuffled_auc(sess, fixation, lo, m, rng, device=0):
    """Column 6 for the clips of the batch at `lo`: shuffled AUC of the clean prediction (resized to the fixation size, and
    through the session's postprocess stage when that is on) against the union of the fixations of m other clips of the set,
    drawn from `rng`."""
    from sap3d_tensorflow_amd import dataflow, metrics
    pred = sess.activation("pred")[:, -1, :, :, 0]
    post = sess.postprocess
    match = sess.hist_match
    if match and match["mode"] == "density":
        raise ValueError("--sauc scores the clean map against other clips' fixations: it takes --match-hist FILE.npz, not density")
    stage = sess.prior_stage
    if stage:
        table = (match["cdf"], match["bin_centers"]) if match else None
        full = dataflow.postprocess_maps(pred, fixation.shape[1:], device=device, hist_match=table, nbins=match["nbins"] if match else 256,
                                         prior=sess.prior_map, prior_mode=stage["mode"], prior_weight=stage["weight"], **(post or {}))
    elif match:
        full = dataflow.postprocess_maps(pred, fixation.shape[1:], device=device, hist_match=(match["cdf"], match["bin_centers"]),
                                         nbins=match["nbins"], **(post or {}))
    elif post:
        full = dataflow.postprocess_maps(pred, fixation.shape[1:], device=device, **post)
    else:
        full = dataflow.resize_linear(pred, fixation.shape[1:], device=device)
    out = []
    for k in range(len(pred)):
        i = lo + k
        others = rng.choice(np.delete(np.arange(len(fixation)), i), size=min(m, len(fixation) - 1), replace=False)
        other = np.any(fixation[others] >= 128, axis=0).astype(np.float32)
        out.append(metrics.AUC_shuffled(full[k], (fixation[i] >= 128).astype(np.float32), other, device=device, rng=rng))
    return out


def sauc_others(n, lo, hi, m, rng):
    """--sauc-device: the other clips of every clip of the batch [lo, hi), int32 [hi - lo, min(m, n - 1)], drawn clip by clip as
    shuffled_auc draws them."""
    return np.asarray([rng.choice(np.delete(np.arange(n), i), size=min(m, n - 1), replace=False) for i in range(lo, hi)], np.int32)


def match_target(args):
    """What --match-hist asks for, as P3DSession.set_hist_match takes it: "off", "density", or the table of an .npz."""
    if not args.match_hist:
        return "off"
    if args.match_hist == "density":
        return "density"
    from sap3d_tensorflow_amd import dataflow
    return dataflow.load_match_table(args.match_hist)


def prior_plan(args):
    """What the --prior* flags and --info-gain prior ask for, or None when no prior is built: dict(source: "set" (the set's own
    fixation array) or the .npz of --prior-from, leave_out, sigma, radius, mode, weight, baseline: "prior" or None).  Exits on a
    combination that cannot be served, before anything runs."""
    ig = args.info_gain == "prior"
    stage = args.prior != "off"
    if not ig and not stage:
        for flag, given in (("--prior-from", bool(args.prior_from)), ("--prior-sigma", args.prior_sigma != 0.), ("--prior-radius", args.prior_radius != 0)):
            if given:
                raise SystemExit("%s builds a prior that nothing uses: add --info-gain prior or --prior mul|mix" % flag)
        if args.prior_weight != 0.:
            raise SystemExit("--prior-weight needs --prior mul|mix")
        if args.prior_leave_out:
            raise SystemExit("--prior-leave-out needs --info-gain prior")
        return None
    if args.prior_weight != 0. and not stage:
        raise SystemExit("--prior-weight needs --prior mul|mix")
    if not 0. <= args.prior_weight <= 1.:
        raise SystemExit("--prior-weight: the weight must be in [0, 1]")
    if not args.prior_sigma >= 0. or args.prior_radius < 0 or args.prior_radius > 255:
        raise SystemExit("--prior-sigma must be >= 0 and --prior-radius in 0..255")
    if args.prior_leave_out and not ig:
        raise SystemExit("--prior-leave-out needs --info-gain prior")
    if args.prior_leave_out and args.prior_from:
        raise SystemExit("--prior-leave-out takes a batch's clips out of the set's own prior: it does not go with --prior-from")
    return dict(source=args.prior_from or "set", leave_out=bool(args.prior_leave_out), sigma=float(args.prior_sigma), radius=int(args.prior_radius),
                mode=args.prior, weight=float(args.prior_weight), baseline="prior" if ig else None)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--model", type=str, default="", help="checkpoint: a directory with a TF `checkpoint` state file, a TF bundle "
                   "prefix, or an .npz keyed by TF variable names (test.py:145-150); none: freshly initialised weights")
    p.add_argument("--ema", action="store_true", help="[addition] score the moving averages of the checkpoint: every trainable is "
                   "restored from <var>/ExponentialMovingAverage (train.py --ema-decay; P3DSession.restore ema_as_weights)")
    p.add_argument("--structure", type=str, default="unet++",
                   help="unet, concat, unet++ (built as unet++ds, p3d_unetplusplus_ds, the buildable form of test.py:133-138), "
                        "unet++nonsa, gn_p3d, gn_p3d_concat, gn_p3d_decoder")
    p.add_argument("--data", type=str, default="", help="test set .npz (x, density, fixation); default: a synthetic set")
    p.add_argument("--clips", type=int, default=6, help="clips of the synthetic set")
    p.add_argument("--batch", type=int, default=2)
    p.add_argument("--gpu", type=str, default="0")
    p.add_argument("--seed", type=int, default=0, help="seeds numpy's global stream (the metrics' draws) and the synthetic set")
    p.add_argument("--sauc", type=int, default=0, metavar="M", help="add shuffled AUC against the fixations of M other clips")
    p.add_argument("--sauc-device", action="store_true", help="[addition] compute --sauc's column inside the evaluation pass, from a "
                   "fixation pool kept on the device (P3DSession.open_fixation_pool)")
    p.add_argument("--time", action="store_true", help="print the stage times of every batch")
    p.add_argument("--kldiv", action="store_true", help="add KL divergence of the density from the scored map (utils/metrics.py KLdiv; "
                   "P3DSession.set_eval_extra)")
    p.add_argument("--info-gain", type=str, default="", metavar="BASELINE.npy|prior", help="[addition] add information gain over the "
                   "baseline map of this .npy, float32 [H, W] at the fixation maps' size (the MIT benchmark's InfoGain); `prior`: "
                   "over a fixation prior built on the device from the set's own fixation maps (P3DSession.open_prior)")
    p.add_argument("--prior-from", type=str, default="", metavar="OTHER.npz", help="[addition] build the prior from the `fixation` array "
                   "of another set instead")
    p.add_argument("--prior-sigma", type=float, default=0., metavar="S", help="[addition] the Gaussian that smooths the summed fixations")
    p.add_argument("--prior-radius", type=int, default=0, metavar="R", help="[addition] its radius, as --blur-radius")
    p.add_argument("--prior-leave-out", action="store_true", help="[addition] with --info-gain prior: every batch is scored against "
                   "the prior of the other clips (its own are taken out of the counts, and put back)")
    p.add_argument("--prior", choices=("off", "mul", "mix"), default="off", help="[addition] combine every (smoothed) prediction with the "
                   "prior before it is matched, normalised and scored (P3DSession.set_prior_stage): v ((1 - A) g + A), or (1 - A) v + A g")
    p.add_argument("--prior-weight", type=float, default=0., metavar="A", help="[addition] the weight A in [0, 1]")
    p.add_argument("--blur-sigma", type=float, default=0., metavar="S", help="[addition] smooth every resized prediction with a "
                   "Gaussian of S pixels before it is scored (P3DSession.set_postprocess)")
    p.add_argument("--blur-radius", type=int, default=0, metavar="R", help="[addition] the Gaussian's radius in pixels, at most 255; "
                   "0: cv2's rule, (int(rint(8 S + 1)) | 1) // 2")
    p.add_argument("--normalize", choices=("none", "max", "range"), default="none",
                   help="[addition] scale every (smoothed) map by its maximum, or to its range, before it is scored")
    # the reduced graph of the tests (the reference's is base 64, blocks 3/8/36)
    p.add_argument("--base", type=int, default=64, help=argparse.SUPPRESS)
    p.add_argument("--match-hist", type=str, default="", metavar="density|FILE.npz", help="[addition] match the histogram of every "
                   "(smoothed) prediction before it is normalised and scored (utils/metric_utils.py match_hist; "
                   "P3DSession.set_hist_match): `density` -- to its own ground-truth density map; or an .npz with `cdf` and "
                   "`bin_centers` -- one target table for every map")
    p.add_argument("--match-bins", type=int, default=256, metavar="N", help="[addition] bins of --match-hist's histograms, 2 .. 1024")
    p.add_argument("--blocks", type=str, default="3,8,36", help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if not 2 <= args.match_bins <= 1024:
        p.error("--match-bins must be in 2..1024")
    if args.sauc_device and not args.sauc:
        p.error("--sauc-device needs --sauc M")
    if args.sauc_device and args.sauc > 64:
        p.error("--sauc-device takes M <= 64")
    return args


def main(argv=None):
    args = parse_args(argv)
    from sap3d_tensorflow_amd import P3DSession, synthetic
    device = int(args.gpu)
    if args.data:
        x, density, fixation = load_set(args.data, device)
    else:
        x, density, fixation = synthetic.synthetic_test_set(args.seed, args.clips)
    plan = prior_plan(args)                                                                       # refused before anything runs
    baseline = load_baseline(args.info_gain, fixation.shape[1:]) if args.info_gain and args.info_gain != "prior" else None
    prior_fix = fixation
    if plan and plan["source"] != "set":
        prior_fix = last_frame(np.load(plan["source"])["fixation"])
        if prior_fix.dtype != np.uint8 or prior_fix.shape[1:] != fixation.shape[1:]:
            raise ValueError("--prior-from: %s holds %s %s fixation maps, the set's are uint8 %s" % (plan["source"], prior_fix.dtype, prior_fix.shape[1:], fixation.shape[1:]))
    structure = "unet++ds" if args.structure == "unet++" else args.structure
    blocks = tuple(int(v) for v in args.blocks.split(","))
    sess = P3DSession(structure, batch=args.batch, frames=x.shape[1], height=x.shape[2], width=x.shape[3], base=args.base,
                      blocks=blocks, device=device, seed=0)
    if args.model:
        print("loading checkpoint %s" % sess.restore(args.model, ema_as_weights=args.ema))
    print("Now using model %s with structure %s" % (args.model or "(initialised)", structure))
    sess.set_postprocess(args.blur_sigma, args.blur_radius, args.normalize)
    sess.set_hist_match(match_target(args), args.match_bins)
    ig_prior = bool(plan and plan["baseline"])
    if plan:
        sess.open_prior(fixation.shape[1:], "fixations")
        sess.prior_add(prior_fix)
        sess.finish_prior(plan["sigma"], plan["radius"])
        if plan["mode"] != "off":
            sess.set_prior_stage(plan["mode"], plan["weight"])
    extra_on = args.kldiv or baseline is not None or ig_prior
    if ig_prior:
        sess.set_eval_extra(kldiv=args.kldiv, baseline="prior")
    elif extra_on:
        sess.set_eval_extra(kldiv=args.kldiv, info_gain=baseline is not None, baseline=baseline)
    extra_cols = [[] for _ in range(2)]                                   # KL, IG
    labels = [(k, name) for k, name, on in ((0, "KLdiv", args.kldiv), (1, "IG", baseline is not None or ig_prior)) if on]

    def extras():
        return [(name, nan_dropped_mean(extra_cols[k])) for k, name in labels]
    np.random.seed(args.seed)
    sauc_rng = np.random.RandomState(args.seed) if args.sauc else None
    if args.sauc_device:
        if len(fixation) < 2:
            raise SystemExit("--sauc-device needs at least two clips")
        sess.open_fixation_pool(fixation.shape[1:], len(fixation))
        sess.fixation_pool_put(0, fixation)
    cols = [[] for _ in range(6 if args.sauc else 5)]
    index = 0
    for lo, hi in batches(len(x), args.batch):
        index += 1
        if index % 100 == 0:
            print(metric_line(STEP_LINE, index, [np.mean(c) for c in cols], extras()))
        if plan and plan["leave_out"]:                                    # the baseline of the other clips
            sess.prior_add(fixation[lo:hi], -1)
            sess.finish_prior(plan["sigma"], plan["radius"])
            sess.set_eval_extra(kldiv=args.kldiv, baseline="prior")
        shuffled = None
        if args.sauc_device:                                              # the docstring's draw order
            shuffled = dict(others=sauc_others(len(fixation), lo, hi, args.sauc, sauc_rng), rng=sauc_rng)
            shuffled["n_other"] = sess.shuffled_begin(shuffled["others"])
        m = sess.evaluate(x[lo:hi], density[lo:hi], fixation[lo:hi], size=fixation.shape[1:], shuffled=shuffled)
        if plan and plan["leave_out"]:
            sess.prior_add(fixation[lo:hi], 1)
        for k in range(5):
            cols[k].extend(m[:, k].tolist())
        if extra_on:
            e = sess.last_eval_extra()
            for k in range(2):
                extra_cols[k].extend(e[:, k].tolist())
        if args.sauc_device:
            cols[5].extend(sess.last_eval_shuffled()[0].tolist())
        elif args.sauc:
            cols[5].extend(shuffled_auc(sess, fixation, lo, args.sauc, sauc_rng, device))
        if args.time:
            t = sess.last_eval_ms
            print("  batch %d: forward %.3f ms  host draws %.3f ms  host->device %.3f ms  device metrics %.3f ms"
                  % (index, t["forward"], t["draws"], t["h2d"], t["device"]))
    post = sess.postprocess
    print(metric_line(ALL_LINE, index, nan_dropped_means(cols), extras()) +
          ("   postprocess: sigma %g radius %d normalize %s" % (post["sigma"], post["radius"], post["norm"]) if post else "") +
          ("   match-hist: %s, %d bins" % (args.match_hist, args.match_bins) if args.match_hist else "") +
          ("   prior: %s %g" % (plan["mode"], plan["weight"]) if plan and plan["mode"] != "off" else ""))
    print("Testing Finished!")
    sess.close()
    return cols + [extra_cols[k] for k, _ in labels]


if __name__ == "__main__":
    main()
