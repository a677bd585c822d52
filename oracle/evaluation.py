"""ORACLE (test infrastructure only -- never imported by the product): the evaluation pass of the reference's test.py
(/root/reference/test.py:160-183) in numpy, on top of oracle/metrics.py and oracle/dataflow.py:
  * AUC_shuffled, /root/reference/utils/metrics.py:157-197, restated with Python 2 semantics;
  * test_py_clip_metrics, the per-clip body of test.py:166-176 (resizes, in-place jitter, numpy draw order);
  * synthetic_test_set, the law of the synthetic evaluation set of drivers/test.py.

PARITY UNPINNED, as for oracle/metrics.py: the reference is Python 2 / TF 1.x code with cv2 and skimage imports and ships no
metric fixtures, so only a side-by-side reading pins this file.
"""
import numpy as np

from .metrics import AUC_Borji, AUC_Judd, CC, NSS, SIM, _same_shape, _trapz, normalize
from .p3d import synthetic_clip


def AUC_shuffled(saliency_map, fixation_map, other_map, n_rep=100, step_size=0.1, rng=None, other_idx=None):
    """utils/metrics.py:157-197 with Python 2 semantics (`map` is eager): other_map > 0.5 raveled; for each of the n_rep
    splits in order one random.permutation(len(fixated))[:n_fix] (:190; numpy's global stream unless `rng`); transposed to
    [min(n_fix, n_other), n_rep] (:191).  Shorter rows keep fp's division by n_fix (:151-152); n_other = 0 gives no random
    samples and the curve closes at (1, 1).  A shape mismatch raises (:186-187); no fixation: NaN before any draw (:122-124).
    `other_idx` supplies the sampled pixel indices instead.  Returns (mean AUC, per-split AUCs)."""
    other = np.asarray(other_map) > 0.5
    if other.shape != np.shape(fixation_map):
        raise ValueError("other_map.shape != fixation_map.shape")
    S2 = np.asarray(saliency_map, dtype=np.float64)
    F2 = np.asarray(fixation_map) > 0.5
    _same_shape(S2, F2)
    if not np.any(F2):
        return np.nan, None
    S = normalize(S2, method="range").ravel()
    F = F2.ravel()
    S_fix = S[F]
    n_fix = len(S_fix)
    if other_idx is None:
        src = rng if rng is not None else np.random
        fixated = np.nonzero(other.ravel())[0]
        rows = [src.permutation(len(fixated))[:n_fix] for _ in range(n_rep)]
        other_idx = fixated[np.asarray(rows, dtype=np.int64).reshape(n_rep, -1).T]
    S_rand = S[np.asarray(other_idx, dtype=np.int64).reshape(-1, n_rep)]
    auc = np.zeros(n_rep) * np.nan
    for rep in range(n_rep):
        thresholds = np.r_[0:np.max(np.r_[S_fix, S_rand[:, rep]]):step_size][::-1]
        tp = np.zeros(len(thresholds) + 2)
        fp = np.zeros(len(thresholds) + 2)
        tp[0] = 0; tp[-1] = 1
        fp[0] = 0; fp[-1] = 1
        for k, thresh in enumerate(thresholds):
            tp[k + 1] = np.sum(S_fix >= thresh) / float(n_fix)
            fp[k + 1] = np.sum(S_rand[:, rep] >= thresh) / float(n_fix)
        auc[rep] = _trapz(tp, fp)
    return np.mean(auc), auc


def test_py_clip_metrics(prediction, density_u8, fixation_u8, jitter=True, n_rep=100, step_size=0.1, rng=None):
    """The body of test.py's per-clip loop (test.py:166-176) for ONE clip -> [CC, SIM, AUC_Judd, AUC_Borji, NSS] (float64).
    prediction: the clip's last 112x112 frame (float32); density_u8 [Hd, Wd] and fixation_u8 [H, W] the decoded grey images.
      * prediction -> cv2.resize(prediction, (W, H)) (:170), float32;  density -> cv2.resize(uint8) / 255. (dataflow.py:236-238,
        float64);  fixation -> / 255. (dataflow.py:239-241);
      * CC and SIM see the clean map; AUC_Judd adds random.rand(H, W) * 1e-7 IN PLACE (utils/metrics.py:54,65: np.array(...,
        copy=False) then +=, a float64 sum rounded once to float32), so AUC_Borji and NSS see the jittered map;
      * draws from `rng` (default numpy's global stream): jitter, then randint(0, H*W, [n_fix, n_rep]) (:139); a clip without
        fixation draws nothing (both return NaN first, :56-59 and :122-124);
      * `jitter` may be the noise array itself (float64 [H, W], random.rand * 1e-7 already applied): then it is not drawn."""
    from . import dataflow
    H, W = np.shape(fixation_u8)
    src = rng if rng is not None else np.random
    pred = dataflow.resize_linear(np.asarray(prediction, dtype=np.float32), H, W)
    density = dataflow.resize_linear_u8(np.asarray(density_u8, dtype=np.uint8), H, W) / 255.
    fixation = np.asarray(fixation_u8) / 255.
    out = [CC(pred, density), SIM(pred, density)]
    n_fix = int(np.count_nonzero(fixation > 0.5))
    if n_fix == 0:
        return np.array(out + [np.nan, np.nan, NSS(pred, fixation)])
    if jitter is not None and not np.isscalar(jitter):
        noise = np.asarray(jitter, dtype=np.float64).reshape(H, W)
    else:
        noise = src.rand(H, W) * 1e-7 if jitter else None
    if noise is not None:
        pred = (pred.astype(np.float64) + noise).astype(np.float32)        # numpy's float32 += float64
    out.append(AUC_Judd(pred, fixation))
    out.append(AUC_Borji(pred, fixation, src.randint(0, H * W, [n_fix, n_rep]), step_size)[0])
    out.append(NSS(pred, fixation))
    return np.array(out)


def synthetic_test_set(seed, n, size=(1080, 960), density_size=(270, 480), frames=16, crop=112):
    """The synthetic evaluation set of drivers/test.py (sap3d_tensorflow_amd.synthetic.synthetic_test_set): x by the
    synthetic_clip law; density uint8 [n, Hd, Wd] uniform bytes; fixation uint8 [n, H, W]: clip i gets 255 at k ~ U{50..999}
    uniform pixel draws (with replacement), except every third clip (i % 3 == 2), which stays empty."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = synthetic_clip(seed, (n, frames, crop, crop, 3))
    density = rng.integers(0, 256, size=(n,) + tuple(density_size), dtype=np.uint8)
    fixation = np.zeros((n,) + tuple(size), np.uint8)
    for i in range(n):
        k = int(rng.integers(50, 1000))
        pix = rng.integers(0, size[0] * size[1], size=k)
        if i % 3 != 2:
            fixation[i].reshape(-1)[pix] = 255
    return x, density, fixation
