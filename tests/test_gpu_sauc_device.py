"""Shuffled AUC from a fixation pool on the device (csrc/fixpool.hip, include/p3d_hip.h): pack, union + scan and select are held to
the numpy replay (tests/sauc_ref.py) with tolerance 0 through the guarded op-level hooks; the whole armed sequence on supplied
maps, P3DSession.evaluate(shuffled=...) and drivers/test.py --sauc-device are held to metrics.AUC_shuffled on the clean
full-resolution map, and the five columns (and KL / IG) to their unarmed bits."""
import contextlib
import importlib.util
import io
import os

import numpy as np
import pytest

from oracle import evaluation as oev

import sauc_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(base=16, blocks=(2, 2, 3))
BYTES = np.array([0, 127, 128, 255], np.uint8)          # both sides of the threshold


def _sparse_pool(seed, cap, shape, counts):
    """uint8 [cap, H, W]: map i has counts[i] fixated pixels (128 / 255) and some bytes of 127 that must not count."""
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    pool = np.zeros((cap, n), np.uint8)
    for i in range(cap):
        pool[i, rng.choice(n, min(n, 40), replace=False)] = 127
        pool[i, rng.choice(n, counts[i], replace=False)] = rng.choice(BYTES[2:], counts[i])
    return pool.reshape((cap,) + tuple(shape))


# ---- pack -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,n", [((3, 5), 3), ((7, 19), 5), ((16, 16), 3), ((1080, 960), 2)],
                         ids=["3x5-partial-word", "7x19-misaligned-maps", "16x16", "1080x960"])
def test_pack_equals_the_replay_at_every_offset(shape, n):
    """3x5: one partial word; 7x19 = 133 pixels: two words and a partial one, and 133 % 4 != 0 so that maps 1.. of the call start
    misaligned (the element path) whatever the offset; 16x16 and 1080x960 at offset 0: the 16-byte path for every map."""
    from sap3d_tensorflow_amd import dataflow as gdf
    rng = np.random.default_rng(shape[0])
    maps = rng.choice(BYTES, size=(n,) + shape)
    want = ref.pack(maps)
    tail = (shape[0] * shape[1]) % 64
    for offset in range(4):
        got = gdf.pack_fixations(maps, offset=offset)
        assert got.dtype == np.uint64 and np.array_equal(got, want), offset
        if tail:
            assert np.all(got[:, -1] >> np.uint64(tail) == 0)
    ones = np.full((1,) + shape, 255, np.uint8)
    got = gdf.pack_fixations(ones)
    assert np.array_equal(got, ref.pack(ones)) and np.all(got[0, :-1] == np.uint64(2 ** 64 - 1))


# ---- union and scan -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 10, 64])
def test_union_and_scan_equal_the_replay(M):
    """130 x 130 = 16 900 pixels = 265 words: the scan's block seam lies between words 255 and 256 (P3D_FIX_SCAN_BLOCK = 256).  Slot
    11 is empty (an all-empty union when a row names only it), slot 12 is all ones next to slot 11's zeros in rows that mix
    word ranges."""
    from sap3d_tensorflow_amd import dataflow as gdf
    shape, cap = (130, 130), 13
    assert ref.n_words(130 * 130) == 265 > ref.SCAN_BLOCK
    pool = _sparse_pool(M, cap, shape, [300 + 17 * i for i in range(cap)])
    pool[11] = 0
    pool[12] = 0
    pool[12].reshape(-1)[64 * 3:64 * 5] = 255                  # words 3 and 4 full, their neighbours empty in this map
    pool[12].reshape(-1)[64 * 255:64 * 257] = 200              # full words on either side of the seam
    rng = np.random.default_rng(M + 100)
    others = rng.integers(0, 11, size=(4, M)).astype(np.int32)     # repeats for M > 11 at the latest; M = 10 repeats by chance
    others[1, :] = 11                                          # all-empty
    others[2, :] = 12                                          # full words next to empty ones
    if M > 1:
        others[3, 1] = others[3, 0]                            # a repeated id
    words = gdf.pack_fixations(pool)
    uni, prefix, n_other = gdf.union_fixations(words, shape, others)
    w_uni, w_prefix, w_n = ref.union(pool, others)
    assert np.array_equal(uni, w_uni) and np.array_equal(prefix, w_prefix) and np.array_equal(n_other, w_n)
    assert n_other[1] == 0 and n_other[2] == 4 * 64 and prefix[2, 256] == 3 * 64


@pytest.mark.gpu
def test_union_at_full_resolution():
    from sap3d_tensorflow_amd import dataflow as gdf
    shape = (1080, 960)
    assert ref.n_words(1080 * 960) == 16200
    pool = _sparse_pool(3, 4, shape, [900, 50, 0, 400])
    others = np.array([[0, 1, 3], [2, 2, 2]], np.int32)
    got = gdf.union_fixations(gdf.pack_fixations(pool), shape, others)
    want = ref.union(pool, others)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


# ---- select -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_select_equals_nonzero_at_the_edges_and_for_a_full_permutation():
    from sap3d_tensorflow_amd import dataflow as gdf
    shape, cap = (130, 130), 3
    pool = _sparse_pool(9, cap, shape, [700, 500, 0])
    flat = pool.reshape(cap, -1)
    flat[0, 64 * 255 + 63] = 255                               # the last bit of word 255 (the last word before the seam) ...
    flat[0, 64 * 256: 64 * 258] = 0
    flat[0, 64 * 258] = 255                                    # ... and the first bit of the next non-empty word, past the seam
    flat[1, 64 * 10: 64 * 12] = 255                            # full words
    others = np.array([[0, 1], [0, 0], [1, 2]], np.int32)
    other = ref.other_maps(pool, others).reshape(3, -1)
    words = gdf.pack_fixations(pool)
    _, prefix, n_other = gdf.union_fixations(words, shape, others)
    n_rep = 3
    ranks, n_rows = [], []
    rng = np.random.RandomState(4)
    for b in range(3):
        n = int(n_other[b])
        seam = int(prefix[b, 256])                             # the rank of the first set bit past the block seam
        edge = [0, n - 1, max(seam - 1, 0), min(seam, n - 1), min(seam + 1, n - 1)]
        k = int(np.nonzero(other[b])[0].searchsorted(64 * 255 + 63))
        edge += [min(k, n - 1), min(k + 1, n - 1)]                         # (row 0: word 255's last bit, then the next non-empty word's first)
        r = np.concatenate([np.asarray(edge), rng.permutation(n)]) if b == 0 else np.asarray(edge + list(rng.permutation(n)[:20]))
        r = np.resize(r, ((len(r) + n_rep - 1) // n_rep) * n_rep)       # whole rows
        ranks.append(r.astype(np.int32))
        n_rows.append(len(r) // n_rep)
    got = gdf.select_fixations(words, shape, others, np.concatenate(ranks), n_rows, n_rep)
    at = 0
    for b in range(3):
        want = ref.select(other[b], ranks[b])
        assert np.array_equal(got[at:at + len(want)], want), b
        at += len(want)
    assert other[1, 64 * 255 + 63] and other[1, 64 * 258] and not other[1, 64 * 256:64 * 258].any()      # row 1 is slot 0 alone
    from sap3d_tensorflow_amd import P3dError
    with pytest.raises(P3dError, match="rank"):
        gdf.select_fixations(words, shape, others[:1], np.array([int(n_other[0])] * n_rep, np.int32), [1], n_rep)
    with pytest.raises(P3dError, match="outside"):
        gdf.union_fixations(words, shape, np.array([[0, cap]], np.int32))


# ---- the armed sequence on supplied maps --------------------------------------------------------------------------------------
def _eval_case(seed, size, cap=5, B=2):
    rng = np.random.default_rng(seed)
    H, W = size
    maps = rng.random((B, 112, 112)).astype(np.float32)
    dens = rng.integers(0, 256, size=(B, max(H // 4, 1), max(W // 2, 1)), dtype=np.uint8)
    fix = _sparse_pool(seed + 1, B, size, [60, 25][:B])
    pool = _sparse_pool(seed + 2, cap, size, [80, 9, 0, 30, 12][:cap])
    return maps, dens, fix, pool


def _want_shuffled(full, fix, pool, others, n_other, n_rep, step, seed):
    """metrics.AUC_shuffled on the clean map with the replayed indices, per clip; also the oracle's per-split areas."""
    from sap3d_tensorflow_amd import metrics as gm
    n_fix = np.count_nonzero(fix.reshape(len(fix), -1) >= 128, axis=1)
    ranks, n_rows = gm.shuffled_draws(n_fix, n_other, n_rep, np.random.RandomState(seed))
    idx = ref.replay_idx(pool, others, ranks, n_rows, n_rep)
    other = ref.other_maps(pool, others)
    means, per = [], []
    for b in range(len(fix)):
        f = (fix[b] >= 128).astype(np.float32)
        means.append(gm.AUC_shuffled(full[b], f, other[b].astype(np.float32), n_rep=n_rep, step_size=step, other_idx=idx[b]))
        per.append(oev.AUC_shuffled(full[b], f, other[b].astype(np.float32), n_rep, step, other_idx=idx[b])[1])
    return means, per


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(135, 120), (1080, 960)], ids=["135x120", "1080x960"])
@pytest.mark.parametrize("stages", ["plain", "post+prior", "density+extra"])
def test_armed_sequence_on_supplied_maps(size, stages):
    """The per-split areas are the bits of metrics.AUC_shuffled on the clean scored map (dataflow's entry points make that map);
    each stays within the project's abs = 1e-12 of oracle.evaluation.AUC_shuffled (tests/test_gpu_eval.py); out[B][5] and KL / IG
    are the unarmed bits.  Clip 0 has n_other > n_fix, clip 1 n_other < n_fix (shorter rows)."""
    from sap3d_tensorflow_amd import dataflow as gdf
    from sap3d_tensorflow_amd import metrics as gm
    maps, dens, fix, pool = _eval_case(11, size)
    H, W = size
    others = np.array([[0, 3, 4], [1, 2, 2]], np.int32)
    kw, full = {}, None
    rng = np.random.default_rng(5)
    if stages == "plain":
        full = gdf.resize_linear(maps, size)
    elif stages == "post+prior":
        prior = rng.random(size).astype(np.float32)
        kw = dict(postprocess=dict(sigma=1.5, radius=0, norm="range"), prior=prior, prior_mode="mul", prior_weight=0.25)
        full = gdf.postprocess_maps(maps, size, sigma=1.5, radius=0, norm="range", prior=prior, prior_mode="mul", prior_weight=0.25)
    else:
        kw = dict(hist_match="density", nbins=64, extra=("kldiv", "info_gain"), baseline=rng.random(size).astype(np.float32) + 0.1)
    n_rep, step = 4, 0.1
    n_other = ref.union(pool, others)[2]
    assert n_other[0] > np.count_nonzero(fix[0] >= 128) and 0 < n_other[1] < np.count_nonzero(fix[1] >= 128)
    out, xout, per = gm.evaluate_maps(maps, dens, fix, n_rep=3, rng=np.random.RandomState(1), **kw,
                                      shuffled=dict(pool=pool, others=others, rng=np.random.RandomState(2), n_rep=n_rep, step_size=step))
    plain = gm.evaluate_maps(maps, dens, fix, n_rep=3, rng=np.random.RandomState(1), **kw)
    p_out, p_x = plain if isinstance(plain, tuple) else (plain, None)
    assert np.array_equal(out, p_out, equal_nan=True)
    if p_x is not None:
        assert np.array_equal(xout, p_x, equal_nan=True)
    assert per.shape == (2, n_rep) and np.all((per >= 0) & (per <= 1))
    if full is not None:
        means, oracle_per = _want_shuffled(full, fix, pool, others, n_other, n_rep, step, 2)
        for b in range(2):
            print("clip", b, "device", float(np.mean(per[b])), "metrics.AUC_shuffled", means[b], "oracle max |d|", np.max(np.abs(per[b] - oracle_per[b])))
            assert float(np.mean(per[b])) == means[b]
            assert per[b] == pytest.approx(oracle_per[b], abs=1e-12)


@pytest.mark.gpu
def test_armed_sequence_without_fixation_and_without_others():
    """n_fix = 0: NaN for every split, no draw; n_other = 0: no sample, the curve closes at (1, 1), the oracle's number."""
    from sap3d_tensorflow_amd import dataflow as gdf
    from sap3d_tensorflow_amd import metrics as gm
    size = (135, 120)
    maps, dens, fix, pool = _eval_case(21, size)
    fix[0] = 0
    others = np.array([[0, 1], [2, 2]], np.int32)              # slot 2 is empty
    out, xout, per = gm.evaluate_maps(maps, dens, fix, n_rep=3, rng=np.random.RandomState(1),
                                      shuffled=dict(pool=pool, others=others, rng=np.random.RandomState(2), n_rep=3))
    assert np.all(np.isnan(per[0])) and np.all(np.isnan(out[0, 2:]))
    full = gdf.resize_linear(maps, size)
    means, oracle_per = _want_shuffled(full, fix, pool, others, [ref.union(pool, others)[2][0], 0], 3, 0.1, 2)
    assert float(np.mean(per[1])) == means[1] and per[1] == pytest.approx(oracle_per[1], abs=1e-12)
    assert np.array_equal(out, gm.evaluate_maps(maps, dens, fix, n_rep=3, rng=np.random.RandomState(1)), equal_nan=True)


# ---- session ------------------------------------------------------------------------------------------------------------------
def _session(batch):
    from sap3d_tensorflow_amd import P3DSession
    return P3DSession("unet", batch=batch, seed=0, **CFG)


@pytest.fixture(scope="module")
def sess_case():
    from sap3d_tensorflow_amd import synthetic
    size = (135, 120)
    x, dens, fix = synthetic.synthetic_test_set(4, 2, size=size, density_size=(30, 40))
    fix = _sparse_pool(31, 2, size, [70, 20])
    pool = _sparse_pool(32, 6, size, [90, 10, 0, 35, 5, 60])
    s = _session(2)
    yield s, x, dens, fix, pool, size
    s.close()


@pytest.mark.gpu
def test_session_evaluate_shuffled_equals_the_composition(sess_case):
    from sap3d_tensorflow_amd import dataflow as gdf
    s, x, dens, fix, pool, size = sess_case
    plain = s.evaluate(x, dens, fix, size=size, n_rep=5, rng=np.random.RandomState(3))
    s.open_fixation_pool(size, 8)
    s.fixation_pool_put(0, pool[:4])
    s.fixation_pool_put(4, pool[4:])
    info = s.fixation_pool_info()
    assert info == dict(size=size, capacity=8, words=ref.n_words(size[0] * size[1]), filled=6)
    assert np.array_equal(s.fixation_pool_get(0, 6), ref.pack(pool)) and np.array_equal(s.fixation_pool_get(0, 6), gdf.pack_fixations(pool))
    others = np.array([[0, 3, 5], [1, 4, 4]], np.int32)
    got = s.evaluate(x, dens, fix, size=size, n_rep=5, rng=np.random.RandomState(3), shuffled=dict(others=others, rng=np.random.RandomState(7), n_rep=6))
    assert np.array_equal(got, plain, equal_nan=True)
    means, per = s.last_eval_shuffled()
    full = gdf.resize_linear(s.activation("pred")[:, -1, :, :, 0], size)
    n_other = ref.union(pool, others)[2]
    want, oracle_per = _want_shuffled(full, fix, pool, others, n_other, 6, 0.1, 7)
    assert per.shape == (2, 6) and list(means) == want
    for b in range(2):
        assert per[b] == pytest.approx(oracle_per[b], abs=1e-12)
    # not armed any more: a plain evaluate adds nothing and clears nothing
    again = s.evaluate(x, dens, fix, size=size, n_rep=5, rng=np.random.RandomState(3))
    assert np.array_equal(again, plain, equal_nan=True) and np.array_equal(s.last_eval_shuffled()[1], per)
    # with the postprocess stage on, the clean map is the stage's output
    s.set_postprocess(1.0, 0, "max")
    p2 = s.evaluate(x, dens, fix, size=size, n_rep=5, rng=np.random.RandomState(3))
    g2 = s.evaluate(x, dens, fix, size=size, n_rep=5, rng=np.random.RandomState(3), shuffled=dict(others=others, rng=np.random.RandomState(7), n_rep=6))
    assert np.array_equal(g2, p2, equal_nan=True)
    full2 = gdf.postprocess_maps(s.activation("pred")[:, -1, :, :, 0], size, sigma=1.0, radius=0, norm="max")
    assert list(s.last_eval_shuffled()[0]) == _want_shuffled(full2, fix, pool, others, n_other, 6, 0.1, 7)[0]
    s.set_postprocess(0., 0, "none")
    s.close_fixation_pool()


@pytest.mark.gpu
def test_session_refusals_leave_the_handle_usable(sess_case):
    from sap3d_tensorflow_amd import P3dError
    s, x, dens, fix, pool, size = sess_case
    plain = s.evaluate(x, dens, fix, size=size, n_rep=5, rng=np.random.RandomState(3))

    def same_as_before():
        assert np.array_equal(s.evaluate(x, dens, fix, size=size, n_rep=5, rng=np.random.RandomState(3)), plain, equal_nan=True)
    with pytest.raises(P3dError, match="no fixation pool"):
        s.shuffled_begin(np.zeros((2, 1), np.int32))
    s.open_fixation_pool(size, 8)
    s.fixation_pool_put(0, pool)
    with pytest.raises(P3dError, match="never filled"):           # an unfilled slot
        s.shuffled_begin(np.array([[0, 6], [1, 1]], np.int32))
    with pytest.raises(P3dError, match="outside"):                # an id out of range
        s.shuffled_begin(np.array([[0, 8], [1, 1]], np.int32))
    with pytest.raises(P3dError, match="not inside"):
        s.fixation_pool_put(7, pool[:2])
    with pytest.raises(P3dError, match="never filled"):
        s.fixation_pool_get(5, 2)
    same_as_before()
    others = np.array([[0, 3], [1, 4]], np.int32)
    n_other = s.shuffled_begin(others)
    assert np.array_equal(n_other, ref.union(pool, others)[2])
    n_fix = np.count_nonzero(fix.reshape(2, -1) >= 128, axis=1)
    rows = np.minimum(n_fix, n_other).astype(np.int32)
    ok = np.zeros(int(rows.sum()) * 2, np.int32)
    bad = ok.copy()
    bad[-1] = n_other[1]                                           # a rank >= n_other
    with pytest.raises(P3dError, match="rank"):
        s.evaluate(x, dens, fix, size=size, n_rep=5, shuffled=dict(others=others, n_other=n_other, n_rep=2, ranks=bad, n_rows=rows))
    same_as_before()
    wrong = rows.copy()
    wrong[0] -= 1                                                  # a wrong n_rows
    with pytest.raises(P3dError, match="min\\(n_fix, n_other\\)"):
        s.evaluate(x, dens, fix, size=size, n_rep=5, shuffled=dict(others=others, n_other=n_other, n_rep=2, ranks=ok[:-2], n_rows=wrong))
    same_as_before()                                               # (the refused evaluation disarmed the option)
    s.close_fixation_pool()
    with pytest.raises(P3dError, match="no evaluation has run armed"):
        s.last_eval_shuffled()
    s.open_fixation_pool((64, 64), 2)                              # a pool of another size than the evaluation
    s.fixation_pool_put(0, np.zeros((2, 64, 64), np.uint8))
    with pytest.raises(P3dError, match="fixation pool is 64 x 64"):
        s.evaluate(x, dens, fix, size=size, n_rep=5, shuffled=dict(others=np.zeros((2, 1), np.int32), rng=np.random.RandomState(0)))
    same_as_before()
    s.close_fixation_pool()
    same_as_before()


# ---- driver -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_driver_device_path_equals_the_host_path_at_batch_one():
    spec = importlib.util.spec_from_file_location("test_driver_sauc_gpu", os.path.join(ROOT, "drivers", "test.py"))
    d = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(d)
    base = ["--structure", "unet", "--base", "16", "--blocks", "2,2,3", "--clips", "4", "--seed", "3"]

    def run(extra):
        with contextlib.redirect_stdout(io.StringIO()):
            return d.main(base + extra)
    host = run(["--batch", "1", "--sauc", "2"])
    dev = run(["--batch", "1", "--sauc", "2", "--sauc-device"])
    assert len(dev) == 6 and np.array_equal(np.array(dev), np.array(host), equal_nan=True)
    assert any(np.isnan(dev[5])) and any(np.isfinite(dev[5]))       # the synthetic set's third clip has no fixation
    five = run(["--batch", "2"])
    dev2 = run(["--batch", "2", "--sauc", "2", "--sauc-device"])
    assert np.array_equal(np.array(dev2[:5]), np.array(five), equal_nan=True)
    assert all(0.0 <= v <= 1.0 or np.isnan(v) for v in dev2[5])
