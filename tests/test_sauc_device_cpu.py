"""Shuffled AUC from a fixation pool, without a GPU: the numpy replay of the header's STORE / UNION / SELECT (tests/sauc_ref.py) and
metrics.shuffled_draws are held to oracle.evaluation.AUC_shuffled bit for bit, and the new entry points are declared, exported and
bound."""
import numpy as np
import pytest

from oracle import evaluation as oev

import sauc_ref as ref


def _case(seed, n_fix, other_counts, shape=(23, 19), cap=5):
    rng = np.random.default_rng(seed)
    H, W = shape
    s = rng.random(shape).astype(np.float32)
    f = np.zeros(H * W, np.float32)
    f[rng.choice(H * W, n_fix, replace=False)] = 1.0
    pool = np.zeros((cap, H * W), np.uint8)
    for i, k in enumerate(other_counts):
        pool[i, rng.choice(H * W, k, replace=False)] = rng.choice([128, 200, 255], k)
        pool[i, rng.choice(H * W, 7)] |= 127          # just under the threshold where nothing is set
    return s, f.reshape(shape), pool.reshape((cap,) + shape)


@pytest.mark.parametrize("n_fix,other_counts", [(30, (40, 25, 0, 0, 0)), (60, (10, 8, 0, 0, 0)), (12, (0, 0, 0, 0, 0)), (0, (9, 9, 0, 0, 0))],
                         ids=["n_other>n_fix", "n_other<n_fix", "n_other=0", "n_fix=0"])
def test_replay_and_draws_equal_the_oracle_bit_for_bit(n_fix, other_counts):
    from sap3d_tensorflow_amd import metrics as gm
    s, f, pool = _case(n_fix + 1, n_fix, other_counts)
    others = np.array([[0, 1, 1]])                              # a repeated id
    o = ref.other_maps(pool, others)[0]
    n_other = int(np.count_nonzero(o))
    assert n_other == ref.union(pool, others)[2][0]
    r1, r2 = np.random.RandomState(5), np.random.RandomState(5)
    want, want_rep = oev.AUC_shuffled(s, f, o.astype(np.float32), 9, 0.1, rng=r1)
    ranks, n_rows = gm.shuffled_draws([n_fix], [n_other], 9, rng=r2)
    assert n_rows[0] == (min(n_fix, n_other) if n_fix else 0) and ranks.size == n_rows[0] * 9
    assert r1.randint(1 << 30) == r2.randint(1 << 30)           # both streams were consumed alike (n_fix = 0, n_other = 0: see below)
    idx = ref.replay_idx(pool, others, ranks, n_rows, 9)[0]
    got, got_rep = oev.AUC_shuffled(s, f, o.astype(np.float32), 9, 0.1, other_idx=idx)
    if n_fix == 0:                                               # "no fixation to predict": NaN, and no draw
        assert np.isnan(want) and np.isnan(got) and want_rep is None and got_rep is None and ranks.size == 0
        return
    assert np.array_equal(got_rep, want_rep) and got == want
    if n_other == 0 and n_fix:
        assert ranks.size == 0 and np.all(np.isfinite(want_rep))     # no sample: the curve closes at (1, 1)


def test_shuffled_draws_walks_the_clips_in_order():
    from sap3d_tensorflow_amd import metrics as gm
    n_fix, n_other = [4, 0, 9, 3], [10, 7, 5, 0]
    r1, r2 = np.random.RandomState(2), np.random.RandomState(2)
    ranks, n_rows = gm.shuffled_draws(n_fix, n_other, 3, rng=r1)
    want = []
    for f, o in zip(n_fix, n_other):
        if f:
            want.append(np.asarray([r2.permutation(o)[:f] for _ in range(3)], np.int64).reshape(3, -1).T.ravel())
    assert list(n_rows) == [4, 0, 5, 0]
    assert np.array_equal(ranks, np.concatenate(want)) and ranks.dtype == np.int32


def test_pack_law_and_round_trip():
    rng = np.random.default_rng(0)
    for shape in ((3, 5), (7, 19), (16, 16)):
        m = rng.choice(np.array([0, 127, 128, 255], np.uint8), size=(3,) + shape)
        w = ref.pack(m)
        n = shape[0] * shape[1]
        assert w.shape == (3, (n + 63) // 64) and w.dtype == np.uint64
        for i in range(3):
            flat = m[i].ravel()
            for p in range(n):
                assert bool((int(w[i, p // 64]) >> (p % 64)) & 1) == (flat[p] >= 128)
            if n % 64:
                assert int(w[i, -1]) >> (n % 64) == 0
        assert np.array_equal(ref.unpack(w, n), m.reshape(3, -1) >= 128)
    pool = rng.choice(np.array([0, 0, 0, 255], np.uint8), size=(4, 9, 31))
    uni, prefix, n_other = ref.union(pool, [[0, 3], [2, 2]])
    assert np.array_equal(uni[0], ref.pack(pool[0])[0] | ref.pack(pool[3])[0]) and np.array_equal(uni[1], ref.pack(pool[2])[0])
    assert prefix[0, 0] == 0 and n_other[1] == np.count_nonzero(pool[2])
    other = ref.other_maps(pool, [[0, 3]])[0]
    assert np.array_equal(ref.select(other, np.arange(n_other[0])), np.nonzero(other.ravel())[0])


def test_new_entry_points_are_declared_exported_and_bound():
    import test_abi_cpu
    from sap3d_tensorflow_amd import _lib
    names = {"p3d_fixpool_open", "p3d_fixpool_put", "p3d_fixpool_info", "p3d_fixpool_get", "p3d_fixpool_close", "p3d_fixpool_last_ms",
             "p3d_eval_shuffled_begin", "p3d_eval_shuffled_draws", "p3d_last_eval_shuffled", "p3d_debug_fix_pack", "p3d_debug_fix_union",
             "p3d_debug_fix_select", "p3d_debug_eval_maps_shuffled"}
    assert names <= set(test_abi_cpu.declared_symbols())
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert ref.SCAN_BLOCK == 256


def test_driver_documents_and_parses_the_device_path():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("test_driver_sauc", os.path.join(root, "drivers", "test.py"))
    d = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(d)
    a = d.parse_args(["--sauc", "3", "--sauc-device", "--match-hist", "density"])
    assert a.sauc == 3 and a.sauc_device
    assert not d.parse_args(["--sauc", "3"]).sauc_device
    with pytest.raises(SystemExit):
        d.parse_args(["--sauc-device"])
    r1, r2 = np.random.RandomState(1), np.random.RandomState(1)
    got = d.sauc_others(6, 2, 4, 2, r1)
    want = [r2.choice(np.delete(np.arange(6), i), size=2, replace=False) for i in (2, 3)]
    assert got.shape == (2, 2) and np.array_equal(got, np.asarray(want)) and not np.any(got == np.array([[2], [3]]))
    assert "permutation(n_other)[:n_fix]" in d.__doc__ and "--sauc-device" in d.__doc__
