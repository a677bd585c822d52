"""The SPLIT SWEEP on the device (include/p3d_hip.h; csrc/score_auc_u8.hip): p3d_score_sweep_u8 / p3d_debug_score_sweep_u8 against
tests/score_auc_ref.py's replay -- per_rep bit for bit (every input of the float64 walk is an integer and the order is specified),
lev and top exactly --, the shuffled path through the fixation pool against tests/sauc_ref.py, p3d_video_score_auc on a resident
video against the op-level entry points on video_maps_u8's bytes, the refusals, and drivers/gen_pred.py's new flags."""
import importlib.util
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import sauc_ref as S            # noqa: E402
import score_auc_ref as A       # noqa: E402

OFFSETS = (0, 1, 5, 15)
ROWS = (1, 2, 63, 64, 65, 300)
REPS = (1, 3, 100, 130)
STEPS = (0.1, 0.3, 1.0, 1.0 / 1024)


def _same(got, want):
    """Equal bit for bit, NaN where NaN."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


def _held(sal, fix, idx, n_rows, n_rep, step=0.1, offset=0):
    """The debug hook on a batch against the replay: per_rep, lev, top."""
    from sap3d_tensorflow_amd import metrics
    got, t = metrics.score_sweep(sal, fix, idx, n_rows, step, with_tables=True, offset=offset, n_rep=n_rep)
    want = A.sweep_maps(sal, fix, idx, n_rows, n_rep, step)
    assert np.array_equal(t["lev"], want["lev"])
    assert np.array_equal(t["top"], want["top"])
    assert _same(got, want["per_rep"])
    return got


def _draw(rng, N, rows, n_rep):
    return rng.randint(0, N, [rows, n_rep]).astype(np.int32)


@pytest.mark.parametrize("shape", A.SHAPES)
def test_every_shape_content_and_offset_equals_the_replay(shape):
    H, W = shape
    rng = np.random.RandomState(H + W)
    for content in A.CONTENTS:
        sal, fix = A.case(H, W, content)
        nf = int(A.n_fix(fix[None])[0])
        idx = _draw(rng, H * W, nf, 3)
        for offset in OFFSETS:
            got = _held(sal[None], fix[None], idx, [nf], 3, 0.1, offset)
            assert np.isfinite(got).all()


def test_rows_and_splits_on_both_sides_of_a_wave_and_of_a_block():
    sal, fix = A.case(64, 65, "blobs", 300)
    rng = np.random.RandomState(5)
    for rows in ROWS:
        for n_rep in REPS:
            _held(sal[None], fix[None], _draw(rng, sal.size, rows, n_rep), [rows], n_rep)


@pytest.mark.parametrize("step", STEPS)
def test_every_step_on_every_content(step):
    rng = np.random.RandomState(11)
    for H, W in ((16, 16), (64, 65)):
        for content in A.CONTENTS:
            sal, fix = A.case(H, W, content)
            nf = int(A.n_fix(fix[None])[0])
            _held(sal[None], fix[None], _draw(rng, H * W, nf, 5), [nf], 5, step, 5)


def test_top_comes_from_a_sample_that_is_the_maps_only_maximum():
    H, W = 16, 16
    rng = np.random.RandomState(3)
    sal = rng.randint(0, 200, (H, W)).astype(np.uint8)
    fix = np.zeros((H, W), np.uint8)
    fix.ravel()[rng.choice(H * W, 20, replace=False)] = 255
    peak = int(np.flatnonzero(fix.ravel() < 128)[7])
    sal.ravel()[peak] = 255                               # the only 255, and not fixated
    idx = _draw(rng, H * W, 20, 4)
    idx[idx == peak] = 0
    idx[13, 2] = peak                                     # split 2 alone samples it
    from sap3d_tensorflow_amd import metrics
    _held(sal[None], fix[None], idx, [20], 4)
    _, t = metrics.score_sweep(sal, fix, idx, [20], with_tables=True, n_rep=4)
    maxfix = int(sal[fix >= 128].max())
    assert maxfix < 255 and t["top"][0].tolist() == [max(maxfix, int(sal.ravel()[idx[:, k]].max())) for k in range(4)] and t["top"][0, 2] == 255


def _mixed(n, H, W, n_rep, seed):
    """n maps of mixed content with row counts from 0 to nf; map 1 has no fixation and map 2 is flat where the batch has them."""
    rng = np.random.RandomState(seed)
    sal, fix, idx, rows = [], [], [], []
    for b in range(n):
        s, f = A.case(H, W, A.CONTENTS[b % 3], None, b)
        s, f = s.copy(), f.copy()
        if b == 1:
            f[:] = 0
        if b == 2:
            s[:] = 77
        nf = int(np.count_nonzero(f >= 128))
        k = (nf, nf // 2, 0, 1)[b % 4] if nf else 0
        sal.append(s); fix.append(f); rows.append(k)
        idx.append(_draw(rng, H * W, k, n_rep).ravel())
    return np.stack(sal), np.stack(fix), np.concatenate(idx), np.array(rows, np.int32)


@pytest.mark.parametrize("n", [1, 2, 17])
def test_batches_with_a_map_without_fixation_and_a_flat_map(n):
    from sap3d_tensorflow_amd import metrics
    sal, fix, idx, rows = _mixed(n, 7, 19, 3, n)
    got = _held(sal, fix, idx, rows, 3, 0.1, 1)
    if n > 2:
        assert np.isnan(got[1]).all() and np.isnan(got[2]).all() and np.isfinite(got[0]).all() and np.isfinite(got[3:]).all()
        assert np.array_equal(got[6], np.full(3, 1.0))            # n_rows = 0: every point at fp = 0, the curve closes at (1, 1)
    again = metrics.score_sweep(sal, fix, idx, rows, n_rep=3)          # the plain entry point, and a second call
    assert _same(again, got) and _same(metrics.score_sweep(sal, fix, idx, rows, n_rep=3), got)


def test_one_full_resolution_pair():
    H, W = 1080, 960
    rng = np.random.RandomState(8)
    sal = np.clip(rng.gamma(0.6, 30.0, (H, W)), 0, 255).astype(np.uint8)
    fix = np.zeros((H, W), np.uint8)
    fix.ravel()[rng.choice(H * W, 300, replace=False)] = 255
    _held(sal[None], fix[None], _draw(rng, H * W, 300, 100), [300], 100)


def test_op_level_refusals_leave_the_outputs_untouched():
    from sap3d_tensorflow_amd import P3dError, lib
    import ctypes as C
    sal, fix = A.case(7, 19)
    sal, fix = np.ascontiguousarray(sal), np.ascontiguousarray(fix)
    nf = int(np.count_nonzero(fix >= 128))
    idx = _draw(np.random.RandomState(0), sal.size, nf, 2)
    rows = np.array([nf], np.int32)
    u8, ip, dp = C.POINTER(C.c_ubyte), C.POINTER(C.c_int), C.POINTER(C.c_double)
    out = np.full((1, 2), -7.0)

    def call(sal_=sal, fix_=fix, n=1, H=7, W=19, idx_=idx, rows_=rows, n_rep=2, step=0.1, out_=out):
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)
        return lib().p3d_score_sweep_u8(0, p(sal_, u8), p(fix_, u8), n, H, W, p(idx_, ip), p(rows_, ip), n_rep, step, p(out_, dp))
    bad_idx = idx.copy(); bad_idx[3, 1] = sal.size
    neg_idx = idx.copy(); neg_idx[0, 0] = -1
    for kw in (dict(sal_=None), dict(fix_=None), dict(idx_=None), dict(rows_=None), dict(out_=None), dict(n=0), dict(n=65536), dict(H=0),
               dict(H=4096, W=2049), dict(step=0.0), dict(step=-0.1), dict(step=float("nan")), dict(step=1.0 / 1025), dict(n_rep=0),
               dict(idx_=bad_idx), dict(idx_=neg_idx), dict(rows_=np.array([nf + 1], np.int32), idx_=np.zeros((nf + 1, 2), np.int32)),
               dict(rows_=np.array([-1], np.int32))):
        assert call(**kw) == -1, kw
        assert (out == -7.0).all(), kw
    assert call() == 0 and np.isfinite(out).all()
    from sap3d_tensorflow_amd import metrics
    with pytest.raises(P3dError, match="fixated pixels"):
        metrics.score_sweep(sal, fix, np.zeros((nf + 1, 2), np.int32), [nf + 1])


# ---- the resident video -------------------------------------------------------------------------------------------------------------
CFG = dict(base=16, blocks=(2, 2, 3))
F20, T, SIZE = 20, 16, (48, 40)


def _session():
    from sap3d_tensorflow_amd import P3DSession
    return P3DSession("unet", seed=2, batch=3, frames=T, height=32, width=32, **CFG)


def _video(sess, seed=4):
    frames = np.random.default_rng(seed).normal(0.0, 0.5, (F20, 32, 32, 3)).astype(np.float32)
    sess.open_video(F20, "newest")
    sess.video_put(0, frames)
    for i in range(0, 5, 3):
        sess.video_predict(list(range(5))[i:i + 3])


def _truth(seed=3):
    rng = np.random.RandomState(seed)
    den = np.stack([A._blob(rng, *SIZE) for _ in range(F20)])
    fix = np.stack([A._fix(rng, SIZE[0], SIZE[1], 40) for _ in range(F20)])
    fix[5] = 0                                            # a frame without fixation
    return den, fix


def _pool(seed=9):
    rng = np.random.RandomState(seed)
    pool = np.stack([A._fix(rng, SIZE[0], SIZE[1], k) for k in (60, 45, 7, 0, 80, 33)])        # slot 2: fewer than nf; slot 3: none
    ids = rng.randint(0, 6, (F20, 3)).astype(np.int32)
    ids[:, 1] = ids[:, 0]                                 # repeats
    ids[0] = 0                                            # n_other = 60 > nf
    ids[2] = 2                                            # n_other = 7 < nf
    ids[3] = 3                                            # n_other = 0
    return pool, ids


def test_video_score_auc_equals_the_op_level_entry_points_on_the_bytes_of_video_maps_u8():
    from sap3d_tensorflow_amd import metrics
    sess = _session()
    _video(sess)
    den, fix = _truth()
    pool, ids = _pool()
    n_rep, step = 7, 0.1
    maps = sess.video_maps_u8(0, F20, size=SIZE)
    plain = sess.video_score(0, F20, den, fix, size=SIZE, columns=("cc", "sim", "judd", "kl", "nss"))
    sess.open_fixation_pool(SIZE, len(pool))
    sess.fixation_pool_put(0, pool)
    # an evaluation armed through its own union, to be scored after the new calls
    x = np.random.default_rng(1).normal(0.0, 0.5, (3, T, 32, 32, 3)).astype(np.float32)
    others = ids[:3]
    shuffled = lambda n_other: dict(others=others, n_other=n_other, rng=np.random.RandomState(7), n_rep=4)
    ev0 = sess.evaluate(x, den[:3], fix[:3], size=SIZE, n_rep=5, rng=np.random.RandomState(3), shuffled=shuffled(None))
    sh0 = sess.last_eval_shuffled()[1].copy()
    held = sess.shuffled_begin(others)

    rng = np.random.RandomState(21)
    n_other = sess.video_shuffled_begin(ids)
    uni = S.other_maps(pool, ids)
    assert np.array_equal(n_other, uni.reshape(F20, -1).sum(axis=1)) and n_other[2] == 7 and n_other[3] == 0
    bidx, nf = metrics.borji_draws_u8(fix, n_rep, rng)
    ranks, n_rows = metrics.shuffled_draws(nf, n_other, n_rep, rng)
    assert np.array_equal(n_rows, np.minimum(nf, n_other)) and nf[5] == 0
    got = sess.video_score_auc(0, F20, den, fix, size=SIZE, columns=("cc", "sim", "judd", "kl", "nss"), borji_idx=bidx, shuffled_ranks=ranks,
                               n_rows=n_rows, n_rep=n_rep, step_size=step)
    assert set(sess.last_score_ms) == {"upload", "device", "score", "auc"} and sess.last_score_ms["auc"] > 0.0
    assert _same(got["scores"], plain)
    assert _same(got["borji"], metrics.score_sweep(maps, fix, bidx, nf, step, n_rep=n_rep))
    assert _same(got["borji"], A.sweep_maps(maps, fix, bidx, nf, n_rep, step)["per_rep"])
    sidx = np.concatenate([r.ravel() for r in S.replay_idx(pool, ids, ranks, n_rows, n_rep)]).astype(np.int32)
    assert _same(got["shuffled"], metrics.score_sweep(maps, fix, sidx, n_rows, step, n_rep=n_rep))
    assert _same(got["shuffled"], A.sweep_maps(maps, fix, sidx, n_rows, n_rep, step)["per_rep"])
    assert np.isnan(got["borji"][5]).all() and np.isnan(got["shuffled"][5]).all() and np.isfinite(np.delete(got["shuffled"], 5, 0)).all()
    # only the sweeps, without a density map; a part of the video; and a second call
    part_b, part_nf = metrics.borji_draws_u8(fix[17:], n_rep, np.random.RandomState(2))
    only = sess.video_score_auc(17, 3, None, fix[17:], size=SIZE, columns=(), borji_idx=part_b, n_rep=n_rep, step_size=0.3)
    assert np.isnan(only["scores"]).all() and np.isnan(only["shuffled"]).all()
    assert _same(only["borji"], metrics.score_sweep(maps[17:], fix[17:], part_b, part_nf, 0.3, n_rep=n_rep))
    again = sess.video_score_auc(0, F20, den, fix, size=SIZE, columns=("cc", "sim", "judd", "kl", "nss"), borji_idx=bidx, shuffled_ranks=ranks,
                                 n_rows=n_rows, n_rep=n_rep, step_size=step)
    assert all(_same(again[k], got[k]) for k in got)
    # what was there is what it was: the read-out, video_score, and the evaluation armed on its own union
    assert np.array_equal(sess.video_maps_u8(0, F20, size=SIZE), maps)
    assert _same(sess.video_score(0, F20, den, fix, size=SIZE, columns=("cc", "sim", "judd", "kl", "nss")), plain)
    ev1 = sess.evaluate(x, den[:3], fix[:3], size=SIZE, n_rep=5, rng=np.random.RandomState(3), shuffled=shuffled(held))
    assert _same(ev1, ev0) and _same(sess.last_eval_shuffled()[1], sh0)
    sess.close_video()
    sess.close()


def test_video_refusals_leave_the_outputs_untouched():
    from sap3d_tensorflow_amd import P3dError, metrics
    sess = _session()
    _video(sess)
    den, fix = _truth()
    pool, ids = _pool()
    n_rep = 3
    rng = np.random.RandomState(1)
    bidx, nf = metrics.borji_draws_u8(fix, n_rep, rng)
    maps = sess.video_maps_u8(0, F20, size=SIZE)
    kw = dict(size=SIZE, columns="matlab", n_rep=n_rep)
    with pytest.raises(P3dError, match="no fixation pool"):
        sess.video_shuffled_begin(ids)
    with pytest.raises(P3dError, match="no fixation pool"):
        sess.video_score_auc(0, F20, den, fix, shuffled_ranks=[0], n_rows=np.zeros(F20, np.int32), **kw)
    sess.open_fixation_pool(SIZE, len(pool))
    sess.fixation_pool_put(0, pool[:5])
    with pytest.raises(P3dError, match="never filled"):
        sess.video_shuffled_begin(np.full((F20, 2), 5, np.int32))
    with pytest.raises(P3dError, match="no union is held"):
        sess.video_score_auc(0, F20, den, fix, shuffled_ranks=[0], n_rows=np.zeros(F20, np.int32), **kw)
    sess.fixation_pool_put(5, pool[5:])
    n_other = sess.video_shuffled_begin(ids)
    ranks, n_rows = metrics.shuffled_draws(nf, n_other, n_rep, rng)
    for match, args in (("nothing is asked", dict(columns=())),
                        ("fixation maps", dict(fixation=None, columns=("cc",), borji_idx=bidx)),
                        ("out of range", dict(borji_idx=np.where(np.arange(bidx.size) == 11, SIZE[0] * SIZE[1], bidx))),
                        ("at most 1024", dict(borji_idx=bidx, step_size=1e-4)),
                        ("n_rep", dict(borji_idx=bidx, n_rep=0)),
                        ("min\\(n_fix, n_other\\)", dict(shuffled_ranks=ranks, n_rows=np.where(np.arange(F20) == 4, n_rows - 1, n_rows))),
                        ("rank", dict(shuffled_ranks=np.where(np.arange(ranks.size) == 0, int(n_other[0]), ranks), n_rows=n_rows)),
                        ("frames", dict(first=1, n=F20 - 1, density=den[1:], fixation=fix[1:], shuffled_ranks=ranks, n_rows=n_rows[1:])),
                        ("flags", dict(columns=32, borji_idx=bidx))):
        call = dict(first=0, n=F20, density=den, fixation=fix, **kw)
        call.update(args)
        with pytest.raises(P3dError, match=match):
            sess.video_score_auc(call.pop("first"), call.pop("n"), call.pop("density"), call.pop("fixation"), **call)
    sess.open_fixation_pool((SIZE[0], SIZE[1] + 1), 2)     # a pool of another size drops the held union
    with pytest.raises(P3dError, match="no union is held"):
        sess.video_score_auc(0, F20, den, fix, shuffled_ranks=ranks, n_rows=n_rows, **kw)
    sess.fixation_pool_put(0, np.zeros((2, SIZE[0], SIZE[1] + 1), np.uint8))
    sess.video_shuffled_begin(np.zeros((F20, 1), np.int32))
    with pytest.raises(P3dError, match="the fixation pool holds"):
        sess.video_score_auc(0, F20, den, fix, shuffled_ranks=[0], n_rows=np.zeros(F20, np.int32), **kw)
    # the library's own outputs stay as they were on a refusal
    import ctypes as C
    from sap3d_tensorflow_amd import lib
    out, per = np.full((F20, 5), -7.0), np.full((F20, n_rep), -7.0)
    bad = np.ascontiguousarray(np.where(np.arange(bidx.size) == 11, -1, bidx), np.int32)
    p = lambda a, t: a.ctypes.data_as(t)
    u8, ip, dp = C.POINTER(C.c_ubyte), C.POINTER(C.c_int), C.POINTER(C.c_double)
    rc = lib().p3d_video_score_auc(sess._h, 0, F20, 255.0, SIZE[0], SIZE[1], p(den, u8), p(fix, u8), 7, 1, p(out, dp), p(bad, ip), None, None, n_rep, 0.1,
                                   p(per, dp), None, None)
    assert rc == -1 and (out == -7.0).all() and (per == -7.0).all()
    assert np.array_equal(sess.video_maps_u8(0, F20, size=SIZE), maps)
    sess.close_video()
    sess.close()


def test_driver_writes_borji_and_shuffled_means_and_leaves_the_plain_run_alone(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("gen_pred", os.path.join(ROOT, "drivers", "gen_pred.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    videos, truth = tmp_path / "videos", tmp_path / "truth"
    videos.mkdir()
    truth.mkdir()
    rng = np.random.RandomState(0)
    F = 20
    np.save(videos / "a.npy", rng.randint(0, 256, (F, 60, 80, 3)).astype(np.uint8))
    den = np.stack([A._blob(rng, *SIZE) for _ in range(F)])
    fix = np.stack([A._fix(rng, SIZE[0], SIZE[1], 30) for _ in range(F)])
    fix[3] = 0
    np.save(truth / "a_density.npy", den)
    np.save(truth / "a_fixation.npy", fix)
    common = ["--structure", "unet", "--videos", str(videos), "--batch", "3", "--base", "16", "--blocks", "1,1,1", "--resident", "--truth", str(truth),
              "--size", str(SIZE[0]), str(SIZE[1]), "--write", "npy"]
    gp.main(common + ["--out", str(tmp_path / "auc"), "--score-borji", "--score-sauc", "3", "--score-rep", "6", "--score-step", "0.1", "--score-seed", "5"])
    text = capsys.readouterr().out
    gp.main(common + ["--out", str(tmp_path / "plain1")])
    gp.main(common + ["--out", str(tmp_path / "plain2")])
    one, two = (tmp_path / d / "a_scores.npy" for d in ("plain1", "plain2"))
    assert one.read_bytes() == two.read_bytes() and np.load(one).shape == (F, 5)
    assert not (tmp_path / "plain1" / "a_auc.npy").exists()
    assert np.array_equal(np.load(tmp_path / "auc" / "a_scores.npy"), np.load(one), equal_nan=True)
    # the replay from the same seed, on the bytes the driver scored
    from sap3d_tensorflow_amd import P3DSession, metrics
    sess = P3DSession("unet", batch=3, device=0, seed=0, base=16, blocks=(1, 1, 1))
    assert gp.predict_video_resident(sess, np.load(videos / "a.npy"), 3) == F
    maps = sess.video_maps_u8(0, F, size=SIZE)
    sess.close_video()
    sess.close()
    auc = np.load(tmp_path / "auc" / "a_auc.npy")
    assert auc.shape == (F, 2) and auc.dtype == np.float64
    want = np.full((F, 2), np.nan)
    draw = np.random.RandomState(5)
    for c0 in range(0, F, gp.SCORE_CHUNK):
        c1 = min(F, c0 + gp.SCORE_CHUNK)
        ids = gp.sauc_ids(draw, F, c0, c1, 3, own=True)
        n_other = S.other_maps(fix, ids).reshape(c1 - c0, -1).sum(axis=1)
        bidx, nf = metrics.borji_draws_u8(fix[c0:c1], 6, draw)
        ranks, n_rows = metrics.shuffled_draws(nf, n_other, 6, draw)
        assert all(b not in ids[b - c0] for b in range(c0, c1))
        want[c0:c1, 0] = [np.mean(r) for r in A.sweep_maps(maps[c0:c1], fix[c0:c1], bidx, nf, 6, 0.1)["per_rep"]]
        sidx = np.concatenate([r.ravel() for r in S.replay_idx(fix, ids, ranks, n_rows, 6)])
        want[c0:c1, 1] = [np.mean(r) for r in A.sweep_maps(maps[c0:c1], fix[c0:c1], sidx, n_rows, 6, 0.1)["per_rep"]]
    assert _same(auc, want) and np.isnan(auc[3]).all() and np.isfinite(np.delete(auc, 3, 0)).all()
    means = gp.auc_means(auc)                             # (np.nanmean down the columns of [F, 2], the driver's order of summation)
    assert np.allclose(means, [np.nanmean(auc[:, 0]), np.nanmean(auc[:, 1])], rtol=1e-14, atol=0.0)
    assert "a auc over %d frames: borji=%r, sauc=%r\n" % (F, float(means[0]), float(means[1])) in text
