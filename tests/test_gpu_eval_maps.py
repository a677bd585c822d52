"""The full-resolution evaluation (csrc/metrics_full.hip) on supplied maps: metrics.evaluate_maps runs the launches of
P3DSession.evaluate (one shared sequence, p3d_debug_eval_maps) on the cases of tests/eval_maps_ref.py -- more than one sort
element per thread, both sides of the LDS histogram's limit, 257 and 258 blocks per map, ties, mixed batches, the byte rules,
degenerate rows -- against the float64 oracle composed as oracle.evaluation.test_py_clip_metrics composes test.py:166-176, at
the tolerances of tests/test_gpu_eval.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import evaluation as oev

import eval_maps_ref as R
from test_gpu_eval import TOL, _check          # the project's existing bounds: CC / NSS rel 1e-9, SIM rel 1e-10, AUC abs 1e-12


def _run(c, seed=R.ORACLE_SEED, maps=slice(None), density=None):
    """evaluate_maps on (a slice of) a case -> ([n, 5], the generator's state afterwards)."""
    from sap3d_tensorflow_amd import metrics as gm
    rng = np.random.RandomState(seed)
    jit = c.jitter[maps] if c.jitter is not None else False
    got = gm.evaluate_maps(c.maps[maps], (c.density if density is None else density)[maps], c.fixation[maps], jitter=jit,
                           n_rep=c.n_rep, step_size=c.step, rng=rng)
    return got, rng.get_state()


def _same_state(a, b):
    return np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.BUILDERS))
def test_evaluate_maps_matches_the_oracle_composition(name):
    c = R.case(name)
    want, ref_state = R.oracle_rows(name)
    got, state = _run(c)
    print(name, "n_fix", c.n_fix)
    for b in range(len(got)):
        print("  got ", got[b].tolist())
        print("  want", want[b].tolist())
    assert got.shape == want.shape and _same_state(state, ref_state)
    again, _ = _run(c)
    assert np.array_equal(got, again, equal_nan=True)                  # bit-reproducible by design
    for b, n_fix in enumerate(c.n_fix):
        if (name, b) == R.NAN_PIXEL:
            # np.mean / np.min propagate the NaN into CC and SIM (and NSS); the place of a NaN among sorted thresholds is
            # unspecified in numpy too, so the AUC columns are not compared
            assert np.isnan(want[b, [0, 1, 4]]).all() and np.isnan(got[b, [0, 1, 4]]).all()
        elif n_fix == c.fixation[b].size:
            # every pixel fixated: AUC_Judd is x / 0 (NaN on both sides), NSS the mean of all z-scores (0 but for rounding)
            assert np.isnan(want[b, 2]) and abs(want[b, 4]) < R.NSS_ALL_FIXATED_ABS
            _check(np.r_[got[b, :4], want[b, 4]], want[b])
            assert abs(got[b, 4]) < R.NSS_ALL_FIXATED_ABS
        else:
            _check(got[b], want[b])
        if n_fix == 0:
            assert np.isnan(got[b, 2:]).all() and np.isfinite(got[b, :2]).all()


@pytest.mark.gpu
def test_a_map_scores_the_same_alone_as_in_a_batch():
    """Slot and counter offsets are sums over the maps before (next_pow2(n_fix), + map index): the eight maps of one call, n_fix
    0 .. 5000, equal bit for bit the same maps scored one per call with the same random indices."""
    from sap3d_tensorflow_amd import metrics as gm
    c = R.case("batch")
    H, W = R.scored_size(c)
    rng = np.random.RandomState(R.ORACLE_SEED)
    batch = gm.evaluate_maps(c.maps, c.density, c.fixation, jitter=False, n_rep=c.n_rep, step_size=c.step, rng=rng)
    rng = np.random.RandomState(R.ORACLE_SEED)                          # one stream: map b's draw follows map b-1's
    for b in range(len(c.maps)):
        one = gm.evaluate_maps(c.maps[b:b + 1], c.density[b:b + 1], c.fixation[b:b + 1], jitter=False, n_rep=c.n_rep,
                               step_size=c.step, rng=rng)
        assert np.array_equal(one[0], batch[b], equal_nan=True), (b, one[0], batch[b])
    # and in another order, so that every map sits at other offsets
    order = np.array([7, 3, 0, 6, 1, 5, 2, 4])
    idx = {}
    rng = np.random.RandomState(R.ORACLE_SEED)
    for b in range(len(c.maps)):                                        # map b's indices as the batch drew them
        idx[b] = rng.randint(0, H * W, [c.n_fix[b], c.n_rep]) if c.n_fix[b] else None

    class Replay:                                                       # hands each map its own draw back, whatever the order
        def __init__(self):
            self.k = 0

        def randint(self, lo, hi, shape):
            while idx[order[self.k]] is None:
                self.k += 1
            out = idx[order[self.k]]
            self.k += 1
            assert (lo, hi) == (0, H * W) and list(shape) == list(out.shape)
            return out
    moved = gm.evaluate_maps(c.maps[order], c.density[order], c.fixation[order], jitter=False, n_rep=c.n_rep, step_size=c.step,
                             rng=Replay())
    assert np.array_equal(moved, batch[order], equal_nan=True)


@pytest.mark.gpu
def test_evaluate_maps_agrees_with_the_one_block_entry_points():
    """The maps of the batch case with n_fix <= LCAP through both kernel families.  The density maps get bytes 0 / 255 (v / 255.
    is then exact in float32, what the one-block kernels take) and jitter is off (the one-block AUC_Judd adds float32 noise in
    float32): tests/test_gpu_eval.py::test_full_resolution_reductions_agree_with_the_one_block_entry_points."""
    from sap3d_tensorflow_amd import dataflow as gdf
    from sap3d_tensorflow_amd import metrics as gm
    c = R.case("batch")
    keep = [b for b, k in enumerate(c.n_fix) if k <= R.kernel_constants()["LCAP"]]
    assert [c.n_fix[b] for b in keep] == [0, 1, 2, 1000, 2048, 4096]
    dens = np.where(c.density >= 128, 255, 0).astype(np.uint8)
    got, _ = _run(c, maps=keep, density=dens)
    H, W = R.scored_size(c)
    rng = np.random.RandomState(R.ORACLE_SEED)
    for row, b in zip(got, keep):
        dmap = gdf.mapf_density(dens[b][None], (H, W))[0]
        fmap = (c.fixation[b] >= 128).astype(np.float32)
        one = [gm.CC(c.maps[b], dmap), gm.SIM(c.maps[b], dmap), gm.AUC_Judd(c.maps[b], fmap, jitter=False)]
        n_fix = c.n_fix[b]
        one.append(gm.AUC_Borji(c.maps[b], fmap, n_rep=c.n_rep, step_size=c.step,
                                rand_idx=rng.randint(0, H * W, [n_fix, c.n_rep])) if n_fix else np.nan)
        one.append(gm.NSS(c.maps[b], fmap))
        print(b, row.tolist(), one)
        _check(row, one)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["blocks257", "blocks258"])
def test_auc_shuffled_over_more_than_256_blocks(name):
    """Passes A and B without density maps at 257 blocks per map (a second trip of the folds) and at 258 (a second trip of pass
    B's slot offsets too), then the sweep over the compacted fixated values."""
    from sap3d_tensorflow_amd import metrics as gm
    c = R.case(name)
    s = c.maps[0]
    f = (c.fixation[0] >= 128).astype(np.float32)
    o = np.zeros(s.shape, np.float32)
    o.flat[np.random.default_rng(9).choice(s.size, 1500, replace=False)] = 1
    r1, r2 = np.random.RandomState(5), np.random.RandomState(5)
    got = gm.AUC_shuffled(s, f, o, n_rep=5, step_size=0.1, rng=r1)
    want = oev.AUC_shuffled(s, f, o, 5, 0.1, rng=r2)[0]
    print(got, want)
    assert got == pytest.approx(want, abs=TOL["auc"])
    assert np.array_equal(r1.get_state()[1], r2.get_state()[1])


@pytest.mark.gpu
def test_the_hook_refuses_what_the_evaluation_refuses():
    from sap3d_tensorflow_amd import lib
    c = R.case("odd")
    H, W = R.scored_size(c)
    n_fix = np.array(c.n_fix, np.int32)
    idx = np.zeros(int(n_fix.sum() + 1) * 4, np.int32)
    out = np.empty((1, 5))
    u8, fp, dp, ip = C.POINTER(C.c_ubyte), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)

    def call():
        return lib().p3d_debug_eval_maps(0, c.maps.ctypes.data_as(fp), 1, c.maps.shape[1], c.maps.shape[2], 1,
                                         c.density.ctypes.data_as(u8), c.density.shape[1], c.density.shape[2],
                                         c.fixation.ctypes.data_as(u8), H, W, None, idx.ctypes.data_as(ip),
                                         n_fix.ctypes.data_as(ip), 4, 0.1, out.ctypes.data_as(dp))
    assert call() == 0
    n_fix[0] += 1                                                     # disagrees with the device's count
    assert call() != 0 and b"n_fix" in lib().p3d_last_error()
    n_fix[0] -= 1
    idx[0] = H * W                                                    # an index past the map
    assert call() != 0 and b"out of range" in lib().p3d_last_error()
    idx[0] = 0
    assert call() == 0
