#!/usr/bin/env python3
"""Python-3 counterpart of the reference trainer (/root/reference/train.py) on libp3dhip.

Same flags (train.py:21-45), same step semantics (train.py:217-218: dropout 0.5, training=True, Adam lr,
Smooth-L1 sum), same periodic eval forward (train.py:225-226) and checkpoint cadence (train.py:266-267).  Two flags are
additions the reference does not have: `--loss bce | l1` trains with sigmoid cross-entropy on the head's logits or the L1
sum instead of Smooth-L1, and `--loss kld | kld_cc` with the per-map KL divergence, plus `--cc-weight` times (1 - CC) for
kld_cc, and `--loss kld_cc_nss | kld_cc_nss_sim` adds `--nss-weight` times -NSS on fixation maps and `--sim-weight` times
(1 - SIM) (P3DSession.set_loss); `--regularization weightdecay | l2 | both` adds the weight-decay and L2
terms the reference builds and leaves commented out of its loss (train.py:161, gn/train_p3d_gn_dataset.py:188-189;
P3DSession.set_regularization); `--optimizer momentum | sgd` (with `--momentum`, `--nesterov`) fine-tunes with the
optimisers the reference's --pretrain help names, and `--optimizer-state` saves and restores the optimiser's slots with the
checkpoints (P3DSession.set_optimizer, save_checkpoint / restore optimizer_state); `--clip-norm X` clips every step's
gradients by their global norm, as tf.clip_by_global_norm does, and prints the norm and the scale with the step
(P3DSession.set_grad_clip); `--ema-decay D` (with `--ema-warmup`) keeps tf.train.ExponentialMovingAverage's shadows of the
trainables: the checkpoints carry them, --pretrain restores them when present, and the periodic eval forward and the
validation pass score the averaged weights (P3DSession.set_ema); `--accum-steps K` sums the gradients of K batches before
every optimiser update (P3DSession.set_grad_accum): `--saveiter / --validiter / --plotiter` and the printed step then count
updates, and the printed loss is the sum of the K batches' losses; `--aug-flip / --aug-reverse / --aug-min-scale /
--aug-contrast / --aug-brightness` augment every training clip on the device (P3DSession.set_augment): one set of decisions per
clip for frames, density maps and fixation maps, drawn from the step's seed.  The periodic eval forward and the validation pass
upload their clips again and score them as given, never the augmented ones.  The dataset loaders (dataflow.py,
tensorpack, cv2) are out of scope: clips come either from `--data clips.npz` (arrays x [N,16,112,112,3] already normalised like
dataflow.py:204-208, y [N,16,112,112]; raw uint8 frames go through sap3d_tensorflow_amd.dataflow.mapf_frames first; for the
losses with an NSS term also fix [N,16,112,112] uint8, fixated where >= 128, or at any other resolution, which
sap3d_tensorflow_amd.dataflow.fixations_to_grid brings to the grid) or are synthetic with the loader's value law (fixations:
sap3d_tensorflow_amd.synthetic.synthetic_fixations of the target).
Checkpoints are TensorFlow-1.x V2 bundles `model/<info>/p3d_<step>.ckpt.*` with a `checkpoint` state file, keyed by the
TF variable names of train.py:180-185 (trainables + BN moving statistics): the files the reference's Saver writes and
restores (sap3d_tensorflow_amd/tf_checkpoint.py); `--pretrain` takes such a directory, a bundle prefix, or an .npz.
`--video-data set.npz` [addition] trains from whole videos kept on the device instead of pre-cut clips (P3DSession.open_trainset):
arrays frames uint8 [sum F,H0,W0,3] RGB, density uint8 [sum F,Hd,Wd], optionally fix uint8 [sum F,Hf,Wf], and video_frames int [V].  The
clip list is VideoDataset.setup_video_dataset_p3d's (dataflow.py:39-62; sap3d_tensorflow_amd.dataflow.clip_tuples / split_clips):
`--videolength`, `--overlap`, `--trainingprops` mean what they mean there and `--skip-head` is its skip_head; every epoch is a fresh
permutation of the training tuples; training runs through P3DSession.trainset_step, the eval forward and the validation pass over
the held-out tuples through trainset_forward.  `--trainset-format u8 | f32` picks the frame store (default: u8 for frames
already at --imagesize, else f32).
Every `--validiter` steps the validation pass of train.py:243-264 runs: eval forward over the validation clips, CC / SIM /
AUC_Judd of the LAST frame of every clip (GPU kernels, sap3d_tensorflow_amd.metrics), NaNs dropped, means printed."""
import argparse
import datetime
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def get_arguments():
    p = argparse.ArgumentParser(description="P3D saliency trainer (MI355X-native)")
    p.add_argument("--normalization", type=str, default="BN", help="BN -> p3d.py graphs, GN -> gn/p3d_gn.py nets (train.py:37; case-insensitive)")
    p.add_argument("--structure", type=str, default="unet",
                   help="unet | concat | unet++ (train.py:149-154).  unet++ builds p3d_unetplusplus_ds with --SA True (the attention head "
                        "that can be built, p3d.py:340) and p3d_unetplusplus_nonsa with --SA False (p3d.py:401); both can also be named directly")
    p.add_argument("--SA", type=lambda v: str(v).lower() in ("1", "true", "yes"), default=True, help="self attention in the unet++ head (train.py:38)")
    p.add_argument("--net", type=str, default="P3D", help="with --normalization gn: P3D | P3D_CONCAT | P3D_DECODER (gn/train_p3d_gn_dataset.py:30,169-180)")
    p.add_argument("--batch", type=int, default=2)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--epoch", type=int, default=1)
    p.add_argument("--gpu", type=str, default="0")
    p.add_argument("--pretrain", type=str, default="", help="checkpoint to resume from (train.py:204-210): a directory with a `checkpoint` "
                   "state file (as the reference takes, ./model/<pretrain>/), a TF bundle prefix, or an .npz")
    p.add_argument("--saveiter", type=int, default=1000)
    p.add_argument("--validiter", type=int, default=1000)
    p.add_argument("--plotiter", type=int, default=1000)
    p.add_argument("--info", type=str, default="run")
    # accepted for command-line compatibility with train.py:29-34; they drive the reference's dataset pipeline, which is
    # out of scope here, except for the clip geometry
    p.add_argument("--trainingprops", type=float, default=0.99)
    p.add_argument("--dataset", type=str, default="svsdndhf1k")
    p.add_argument("--videolength", type=int, default=16, help="frames per clip (train.py:32)")
    p.add_argument("--overlap", type=int, default=15)
    p.add_argument("--imagesize", type=int, nargs=2, default=(112, 112), help="clip height width (train.py:34)")
    p.add_argument("--data", type=str, default="", help="npz with x, y; empty = synthetic clips")
    p.add_argument("--video-data", type=str, default="",
                   help="[addition] npz of whole videos kept on the device (P3DSession.open_trainset): frames uint8 [sum F,H0,W0,3] RGB, "
                        "density uint8 [sum F,Hd,Wd], optional fix uint8 [sum F,Hf,Wf], video_frames int [V]; clips are cut there by "
                        "--videolength / --overlap / --skip-head / --trainingprops (dataflow.py:39-62).  Not with --data")
    p.add_argument("--skip-head", type=int, default=11, help="[--video-data] first frame of a video's first clip (dataflow.py:39 skip_head)")
    p.add_argument("--trainset-format", choices=("u8", "f32"), default=None,
                   help="[--video-data] frame store: u8 (3 bytes per pixel; frames already at --imagesize) or f32 (normalised floats, "
                        "any source size); default u8 where it applies")
    p.add_argument("--steps", type=int, default=20, help="steps per epoch when synthetic")
    p.add_argument("--validclips", type=int, default=4, help="validation batches per validation pass when synthetic")
    # not a reference flag (its flags are train.py:21-45): the loss option of P3DSession.set_loss
    p.add_argument("--loss", choices=("smooth_l1", "bce", "l1", "kld", "kld_cc", "kld_cc_nss", "kld_cc_nss_sim"), default="smooth_l1",
                   help="[addition, no reference flag] training loss: smooth_l1 (the reference's, train.py:159), bce (sigmoid "
                        "cross-entropy on the head's logits, summed; no reference counterpart), l1 (L1 sum, train.py:160), kld "
                        "(KL divergence of every predicted / ground-truth map, utils/metrics.py:338-361, summed) or kld_cc "
                        "(kld + cc-weight * (1 - CC), utils/metrics.py:227-250), kld_cc_nss (kld_cc - nss-weight * NSS on the "
                        "fixation maps, utils/metrics.py:200-224) or kld_cc_nss_sim (that + sim-weight * (1 - SIM), :258-287)")
    p.add_argument("--cc-weight", type=float, default=1.0, help="[addition] weight of the (1 - CC) term of --loss kld_cc*")
    p.add_argument("--nss-weight", type=float, default=1.0, help="[addition] weight of the -NSS term of --loss kld_cc_nss*; above 0 "
                   "the clips need fixation maps (--data with `fix`; synthetic runs draw them from the target)")
    p.add_argument("--sim-weight", type=float, default=None, help="[addition] weight of the (1 - SIM) term of --loss kld_cc_nss* "
                   "(default 0 for kld_cc_nss, 1 for kld_cc_nss_sim)")
    # not a reference flag either: the regularisation option of P3DSession.set_regularization
    p.add_argument("--regularization", choices=("none", "weightdecay", "l2", "both"), default="none",
                   help="[addition, no reference flag] terms added to the loss: weightdecay (mean of wd * l2_loss over the "
                        "get_conv_weight kernels, the reference's commented-out train.py:161 and gn/train_p3d_gn_dataset.py:188), "
                        "l2 (mean of 0.0005 * l2_loss over the kernel_regularizer kernels, gn/train_p3d_gn_dataset.py:189; "
                        "--net P3D_DECODER only) or both")
    p.add_argument("--wd", type=float, default=0.0,
                   help="[addition] weight-decay scale; 0 = the reference's (0.001 BatchNorm nets, 0.0005 GroupNorm nets)")
    p.add_argument("--l2", type=float, default=0.0, help="[addition] l2 scale; 0 = the reference's 0.0005")
    # the optimiser the reference's --pretrain help names ("finetune using SGD", train.py:27; gn/train_p3d_gn_dataset.py:61
    # prints Momentum) but never builds: P3DSession.set_optimizer
    p.add_argument("--optimizer", choices=("adam", "momentum", "sgd"), default="adam",
                   help="[addition] adam (tf.train.AdamOptimizer, the reference's, train.py:168), momentum "
                        "(tf.train.MomentumOptimizer(lr, --momentum)) or sgd (tf.train.GradientDescentOptimizer(lr))")
    p.add_argument("--momentum", type=float, default=0.9, help="[addition] momentum of --optimizer momentum")
    p.add_argument("--nesterov", action="store_true", help="[addition] Nesterov momentum (--optimizer momentum only)")
    p.add_argument("--optimizer-state", action="store_true",
                   help="[addition] checkpoints hold the optimiser's slots under their TF names (<var>/Adam, <var>/Adam_1 and "
                        "beta1_power / beta2_power; <var>/Momentum), and --pretrain restores them: a run resumes its optimiser")
    # Momentum and SGD multiply the raw gradient of a SUM loss by lr; TF-1 trainers pair them with tf.clip_by_global_norm
    p.add_argument("--clip-norm", type=float, default=0.0,
                   help="[addition] clip the gradients by their global norm to this value before the optimiser applies them "
                        "(tf.clip_by_global_norm); inf reports the norm without clipping; 0 = off")
    # single checkpoints of a batch-2 SUM loss are noisy: the averaged weights are what TF-1 trainers evaluate
    p.add_argument("--ema-decay", type=float, default=None, metavar="D",
                   help="[addition] keep an exponential moving average of the trainables with this decay (0 <= D < 1, "
                        "tf.train.ExponentialMovingAverage); checkpoints carry the shadows, and the eval forward and the validation "
                        "pass run on them")
    p.add_argument("--ema-warmup", action="store_true",
                   help="[addition] TF's num_updates: step t averages with min(D, (1 + t) / (10 + t)) (--ema-decay only)")
    # BatchNorm normalises over the batch in the whole backbone: a larger --batch changes the statistics, accumulation does not
    p.add_argument("--accum-steps", type=int, default=1, metavar="K",
                   help="[addition] sum the gradients of K batches, each run with its own BatchNorm statistics, before every "
                        "optimiser update (the loss is a sum over the batch, so this is the gradient of K * batch clips; not "
                        "averaged: scale --lr for momentum / sgd).  --saveiter, --validiter, --plotiter and the printed step "
                        "count updates; the printed loss is the sum over the K batches; batches left over at the end of an "
                        "epoch are dropped.  1 = off")
    # the reference's clips overlap in 15 of 16 frames (--overlap) and its loader only resizes (dataflow.py:187-191)
    p.add_argument("--aug-flip", type=float, default=0.0, metavar="P", help="[addition] flip a training clip horizontally with probability P")
    p.add_argument("--aug-reverse", type=float, default=0.0, metavar="P", help="[addition] reverse a training clip in time with probability P")
    p.add_argument("--aug-min-scale", type=float, default=1.0, metavar="S",
                   help="[addition] scale jitter: crop a random window of S .. 1 of the frame (0 < S <= 1) and resize it back "
                        "(cv2.INTER_LINEAR; fixation maps by the grid law); 1 = off")
    p.add_argument("--aug-contrast", type=float, default=0.0, metavar="C", help="[addition] frames * a with a uniform in 1 +- C (0 <= C < 1)")
    p.add_argument("--aug-brightness", type=float, default=0.0, metavar="B", help="[addition] frames + b with b uniform in +- B (B >= 0)")
    return p.parse_args()


def augment_settings(args):
    """P3DSession.set_augment's arguments from the --aug-* flags, or None when all five are at their neutral values."""
    cfg = dict(flip=args.aug_flip, reverse=args.aug_reverse, min_scale=args.aug_min_scale, contrast=args.aug_contrast,
               brightness=args.aug_brightness)
    return None if cfg == dict(flip=0.0, reverse=0.0, min_scale=1.0, contrast=0.0, brightness=0.0) else cfg


def with_fixations(args):
    """Whether the loss reads fixation maps: a loss with an NSS term whose weight is above 0."""
    return args.loss in ("kld_cc_nss", "kld_cc_nss_sim") and args.nss_weight > 0


def grid_fixations(fix, y_shape):
    """The `fix` array of --data on the clips' grid: uint8 [N,T,H,W] as it is, any other [N,T,H0,W0] through fixations_to_grid."""
    from sap3d_tensorflow_amd.dataflow import fixations_to_grid
    fix = np.asarray(fix)
    if fix.dtype != np.uint8 or fix.ndim != 4 or fix.shape[:2] != tuple(y_shape[:2]):
        raise SystemExit("--data: fix is %s %s, expected uint8 [N,T,H,W] beside y %s" % (fix.dtype, fix.shape, tuple(y_shape)))
    if fix.shape == tuple(y_shape):
        return fix
    n, t = fix.shape[:2]
    return fixations_to_grid(fix.reshape((n * t,) + fix.shape[2:]), y_shape[2], y_shape[3]).reshape(tuple(y_shape))


def batches(args, rng):
    """(x, y, fixations) per batch; fixations None unless the loss reads them."""
    from sap3d_tensorflow_amd import synthetic as law
    if args.data:
        d = np.load(args.data)
        x, y = d["x"].astype(np.float32), d["y"].astype(np.float32)
        fix = None
        if with_fixations(args):
            if "fix" not in d:
                raise SystemExit("--loss %s with --nss-weight %g needs fixation maps: --data has no `fix`" % (args.loss, args.nss_weight))
            fix = grid_fixations(d["fix"], y.shape)
        for e in range(args.epoch):
            order = rng.permutation(len(x))
            for i in range(0, len(x) - args.batch + 1, args.batch):
                idx = order[i:i + args.batch]
                yield x[idx], y[idx], (fix[idx] if fix is not None else None)
    else:
        for s in range(args.epoch * args.steps):
            shape = (args.batch, args.videolength, args.imagesize[0], args.imagesize[1])
            y = law.synthetic_target(10_000 + s, shape)
            yield law.synthetic_clip(s, shape + (3,)), y, (law.synthetic_fixations(20_000 + s, y) if with_fixations(args) else None)


def batches_per_epoch(args):
    """How many batches batches() yields per epoch."""
    if args.data:
        return len(range(0, len(np.load(args.data)["y"]) - args.batch + 1, args.batch))
    return args.steps


def validation_batches(args):
    """gt_df of train.py:110-121: the held-out clips (the last 1 - trainingprops share of --data), or synthetic ones."""
    from sap3d_tensorflow_amd import synthetic as law
    if args.data:
        d = np.load(args.data)
        x, y = d["x"].astype(np.float32), d["y"].astype(np.float32)
        first = min(int(len(x) * args.trainingprops), len(x) - args.batch)
        for i in range(max(first, 0), len(x) - args.batch + 1, args.batch):
            yield x[i:i + args.batch], y[i:i + args.batch]
    else:
        for s in range(args.validclips):
            shape = (args.batch, args.videolength, args.imagesize[0], args.imagesize[1])
            yield law.synthetic_clip(500_000 + s, shape + (3,)), law.synthetic_target(600_000 + s, shape)


PUT_CHUNK = 256      # frames per put of --video-data


def video_clips(args, video_frames, rng):
    """The training and validation tuples of --video-data: dataflow.py:39-62 with --videolength, --overlap, --skip-head and
    --trainingprops, shuffled from `rng`."""
    from sap3d_tensorflow_amd import dataflow
    tuples = dataflow.clip_tuples([int(f) for f in video_frames], args.videolength, args.overlap, args.skip_head)
    return dataflow.split_clips(tuples, args.trainingprops, rng)


def video_batches(train, args, rng):
    """A list of --batch (video, start) tuples per batch: every epoch a fresh permutation of the training tuples from `rng`, the
    remainder dropped."""
    for e in range(args.epoch):
        order = rng.permutation(len(train))
        for i in range(0, len(train) - args.batch + 1, args.batch):
            yield [train[j] for j in order[i:i + args.batch]]


class VideoData:
    """--video-data: the set on the session's device and the clip lists.  `rng` is the driver's: the split draws from it first,
    then every epoch's permutation."""

    def __init__(self, sess, args, rng):
        from sap3d_tensorflow_amd import dataflow
        d = np.load(args.video_data)
        for k in ("frames", "density", "video_frames"):
            if k not in d:
                raise SystemExit("--video-data: no `%s` array" % k)
        frames, density, counts = d["frames"], d["density"], [int(f) for f in d["video_frames"]]
        H, W = args.imagesize
        total = sum(counts)
        if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or len(frames) != total:
            raise SystemExit("--video-data: frames are %s %s, expected uint8 [%d,H0,W0,3]" % (frames.dtype, frames.shape, total))
        if density.dtype != np.uint8 or density.ndim != 3 or len(density) != total:
            raise SystemExit("--video-data: density is %s %s, expected uint8 [%d,Hd,Wd]" % (density.dtype, density.shape, total))
        grid = frames.shape[1:3] == (H, W)
        fmt = args.trainset_format or ("u8" if grid else "f32")
        if fmt == "u8" and not grid:
            raise SystemExit("--trainset-format u8 takes frames already at --imagesize %d %d, not %d x %d" % ((H, W) + frames.shape[1:3]))
        fix = None
        if with_fixations(args):
            if "fix" not in d:
                raise SystemExit("--loss %s with --nss-weight %g needs fixation maps: --video-data has no `fix`" % (args.loss, args.nss_weight))
            fix = d["fix"]
            if fix.dtype != np.uint8 or fix.ndim != 3 or len(fix) != total:
                raise SystemExit("--video-data: fix is %s %s, expected uint8 [%d,Hf,Wf]" % (fix.dtype, fix.shape, total))
        self.sess, self.args, self.density, self.size = sess, args, density, (H, W)
        self.base = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        sess.open_trainset(counts, frame_format=fmt, fixations=fix is not None)
        for v, n in enumerate(counts):
            for i in range(0, n, PUT_CHUNK):
                a, b = int(self.base[v]) + i, int(self.base[v]) + min(i + PUT_CHUNK, n)
                sess.trainset_put_frames_u8(v, i, frames[a:b, ..., ::-1])          # the set takes cv2's BGR order, the npz is RGB
                sess.trainset_put_density_u8(v, i, density[a:b])
                if fix is not None:
                    f = fix[a:b]
                    sess.trainset_put_fixations(v, i, f if f.shape[1:] == (H, W) else dataflow.fixations_to_grid(f, H, W))
        self.train, self.valid = video_clips(args, counts, rng)
        self.per_epoch = len(range(0, len(self.train) - args.batch + 1, args.batch))
        info = sess.trainset_info()
        print("Training set on the device:", info["videos"], "videos,", info["total_frames"], "frames,", info["frame_format"], "frames,",
              info["bytes"], "bytes;", len(self.train), "training clips,", len(self.valid), "validation clips")

    def batches(self, rng):
        """(clips, None, None) per batch, in batches()'s shape."""
        for clips in video_batches(self.train, self.args, rng):
            yield clips, None, None

    def last_density(self, clips):
        """The ground truth of the last frame of every clip, float32 [n,H,W] (dataflow.py:210-214)."""
        from sap3d_tensorflow_amd import dataflow
        at = [int(self.base[v]) + s + self.args.videolength - 1 for v, s in clips]
        return dataflow.mapf_density(self.density[at], self.size, device=int(self.args.gpu))

    def validation_batches(self):
        """(prediction, ground truth) of the last frames per batch of held-out tuples, the remainder dropped."""
        for i in range(0, len(self.valid) - self.args.batch + 1, self.args.batch):
            clips = self.valid[i:i + self.args.batch]
            yield self.sess.trainset_forward(clips)[:, -1, ..., 0], self.last_density(clips)


def validate(sess, args, step, video=None):
    """train.py:243-264: CC, SIM, AUC_Judd between the last predicted frame and the last ground-truth frame of every
    validation clip; NaNs (no fixation, flat map) are dropped before averaging.  video: the --video-data set, whose held-out
    tuples are scored instead."""
    from sap3d_tensorflow_amd import metrics
    print("Doing validation...")
    preds, gts = [], []
    for p_, g_ in (video.validation_batches() if video is not None else ()):
        preds.append(p_); gts.append(g_)
    for xs, ys in (validation_batches(args) if video is None else ()):
        image0 = sess.forward(xs, dropout=0.0, training=False)[..., 0]              # train.py:250-251
        preds.append(image0[:, -1]); gts.append(ys[:, -1])                          # prediction[-1], ground_truth[-1]
    if not preds:
        return None
    p, g = np.concatenate(preds), np.concatenate(gts)
    cc, sim, auc = metrics.CC_batch(p, g), metrics.SIM_batch(p, g), metrics.AUC_Judd_batch(p, g)       # jitter on, as train.py:260
    res = tuple(float(np.mean(v[~np.isnan(v)])) if np.any(~np.isnan(v)) else float("nan") for v in (cc, sim, auc))
    print(datetime.datetime.now().isoformat()[:-7], " Step:", step, " Metrics:", *res)
    return res


def scoring(sess, ema):
    """The weights an evaluation runs on: the moving averages under --ema-decay, else the session as it is."""
    import contextlib
    return sess.averaged() if ema else contextlib.nullcontext(sess)


def main():
    args = get_arguments()
    from sap3d_tensorflow_amd import P3dError, P3DSession
    if args.video_data and args.data:
        raise SystemExit("--video-data and --data exclude each other")
    gn_nets = {"P3D": "gn_p3d", "P3D_CONCAT": "gn_p3d_concat", "P3D_DECODER": "gn_p3d_decoder"}     # gn/train_p3d_gn_dataset.py:169-180
    gn = args.normalization.lower() == "gn"
    if gn and args.net not in gn_nets:
        raise SystemExit("--net %s is not built (its attention() calls do not match utils/network.py:157 and cannot build "
                         "in the reference either); have %s" % (args.net, sorted(gn_nets)))
    structure = args.structure
    if structure == "unet++":                                                        # train.py:153-154
        structure = "unet++ds" if args.SA else "unet++nonsa"
    if gn:
        structure = gn_nets[args.net]
    sess = P3DSession(structure, batch=args.batch, frames=args.videolength, height=args.imagesize[0], width=args.imagesize[1],
                      device=int(args.gpu), seed=0)                                  # graph + global_variables_initializer
    sess.set_adam(args.lr)
    if args.nesterov and args.optimizer != "momentum":
        sess.close()
        raise SystemExit("--nesterov needs --optimizer momentum")
    if args.optimizer != "adam":
        try:
            sess.set_optimizer(args.optimizer, lr=args.lr, momentum=args.momentum, use_nesterov=args.nesterov)
        except (P3dError, ValueError) as e:
            sess.close()
            raise SystemExit("--optimizer %s: %s" % (args.optimizer, e))
    saliency = args.loss in ("kld_cc_nss", "kld_cc_nss_sim")
    try:
        if args.loss == "kld_cc":
            sess.set_loss(args.loss, cc_weight=args.cc_weight)
        elif saliency:
            sess.set_loss(args.loss, cc_weight=args.cc_weight, nss_weight=args.nss_weight, sim_weight=args.sim_weight)
        else:
            sess.set_loss(args.loss)
    except (P3dError, ValueError) as e:
        sess.close()
        raise SystemExit("--loss %s: %s" % (args.loss, e))
    terms = {"none": (), "weightdecay": ("weightdecay",), "l2": ("l2",), "both": ("weightdecay", "l2")}[args.regularization]
    try:
        sess.set_regularization(terms, wd=args.wd, l2=args.l2)
    except P3dError as e:
        sess.close()
        raise SystemExit("--regularization %s: %s" % (args.regularization, e))
    if args.clip_norm != 0.0:
        try:
            sess.set_grad_clip(args.clip_norm)
        except (P3dError, ValueError) as e:
            sess.close()
            raise SystemExit("--clip-norm %s: %s" % (args.clip_norm, e))
    ema = args.ema_decay is not None
    if args.ema_warmup and not ema:
        sess.close()
        raise SystemExit("--ema-warmup needs --ema-decay")
    if ema:
        try:
            sess.set_ema(args.ema_decay, warmup=args.ema_warmup)
        except P3dError as e:
            sess.close()
            raise SystemExit("--ema-decay %s: %s" % (args.ema_decay, e))
    accum = args.accum_steps
    if accum != 1:
        try:
            sess.set_grad_accum(accum)
        except P3dError as e:
            sess.close()
            raise SystemExit("--accum-steps %s: %s" % (accum, e))
    aug = augment_settings(args)
    if aug is not None:
        try:
            sess.set_augment(**aug)
        except P3dError as e:
            sess.close()
            raise SystemExit("--aug-*: %s" % e)
    model_dir = os.path.join("model", args.info)
    os.makedirs(model_dir, exist_ok=True)
    if args.pretrain:
        print(args.pretrain, "Using this model to retrain...")
        try:
            sess.restore(args.pretrain, optimizer_state=args.optimizer_state, ema=ema)      # train.py:204-210
        except KeyError as e:
            if not ema or "moving averages" not in str(e):
                raise
            sess.restore(args.pretrain, optimizer_state=args.optimizer_state)          # a checkpoint without shadows:
            sess.set_ema(None)                                                          # they start from its weights
            sess.set_ema(args.ema_decay, warmup=args.ema_warmup)
    print("Start training")
    step = 0                  # optimiser updates
    micro = 0                 # batches seen: `step` itself unless --accum-steps
    rng = np.random.default_rng(0)
    video = None
    if args.video_data:
        try:
            video = VideoData(sess, args, rng)
        except (P3dError, ValueError) as e:
            sess.close()
            raise SystemExit("--video-data: %s" % e)
    per_epoch = (video.per_epoch if video else batches_per_epoch(args)) if accum > 1 else 0
    loss = 0.0
    for xs, ys, fs in (video.batches(rng) if video else batches(args, rng)):
        micro += 1
        if video:
            loss += sess.trainset_step(xs, dropout=0.5, seed=micro)                 # xs: the batch's (video, start) tuples
        else:
            loss += sess.train_step(xs, ys, dropout=0.5, seed=micro, fixations=fs)  # train.py:217-218
        if accum > 1 and sess.grad_accum[1] != 0:
            if micro % per_epoch == 0:      # an incomplete cycle does not cross the epoch (the loaders' remainder=False)
                sess.set_grad_accum(accum)
                loss = 0.0
            continue                        # no update yet: nothing to print, score or save
        step += 1
        if args.clip_norm != 0.0:
            gn_, sc_ = sess.last_grad_norm()
        if step < 10 or step % args.plotiter == 0:
            clip = ("gnorm", "%.9g" % gn_, "scale", "%.9g" % sc_) if args.clip_norm != 0.0 else ()
            if saliency:      # the means over the maps of the last batch where each term is defined
                t = sess.last_loss_terms()
                clip += ("KLD", "%.9g" % t["kld"], "CC", "%.9g" % t["cc"], "NSS", "%.9g" % t["nss"], "SIM", "%.9g" % t["sim"])
            with scoring(sess, ema):
                if video:
                    image, truth = sess.trainset_forward(xs), video.last_density(xs[:1])[0]      # cut again: the clip as stored
                else:
                    image, truth = sess.forward(xs, dropout=0.0, training=False), ys[0][-1]     # train.py:225-226; uploads xs again: the clip as given
            print("Datetime", datetime.datetime.now().isoformat()[:-7], "Training step:", step,
                  float(np.sum(image[0, -1]) * 255.0), float(np.sum(truth) * 255.0), "Training Loss", loss, *clip)
        if step % args.validiter == 0:
            with scoring(sess, ema):
                validate(sess, args, step, video)                                   # train.py:243-264
        if step % args.saveiter == 0:
            sess.save_checkpoint(model_dir, step, keep=10, optimizer_state=args.optimizer_state, ema=ema)     # train.py:180-185,266-267
        loss = 0.0
    if accum > 1:
        print("Optimiser updates:", step, "from", micro, "batches")
    print("Training Finished!")
    sess.close()


if __name__ == "__main__":
    main()
