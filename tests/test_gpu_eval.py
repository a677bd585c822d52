"""The evaluation pass of test.py on the GPU (csrc/metrics_full.hip through the C ABI): the float32 resize bit-exact to the
oracle, shuffled AUC, P3DSession.evaluate against the oracle composition of test.py:166-176, the whole-GPU reductions
against the one-block entry points, and drivers/test.py end to end."""
import ctypes as C
import io
import os
import contextlib

import numpy as np
import pytest

from oracle import dataflow as odf
from oracle import metrics as om
from oracle import evaluation as oev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(base=16, blocks=(2, 2, 3))
TOL = dict(cc=1e-9, sim=1e-10, nss=1e-9, auc=1e-12)


def _session(batch, structure="unet"):
    from sap3d_tensorflow_amd import P3DSession
    return P3DSession(structure, batch=batch, seed=0, **CFG)


def _check(got, want):
    """[CC, SIM, AUC_Judd, AUC_Borji, NSS] at the existing metric tolerances."""
    assert got[0] == pytest.approx(want[0], rel=TOL["cc"]), (got, want)
    assert got[1] == pytest.approx(want[1], rel=TOL["sim"]), (got, want)
    for k in (2, 3):
        if np.isnan(want[k]):
            assert np.isnan(got[k])
        else:
            assert got[k] == pytest.approx(want[k], abs=TOL["auc"]), (k, got, want)
    if np.isnan(want[4]):
        assert np.isnan(got[4])
    else:
        assert got[4] == pytest.approx(want[4], rel=TOL["nss"]), (got, want)


@pytest.mark.gpu
def test_resize_linear_is_bit_exact_to_the_oracle():
    from sap3d_tensorflow_amd import dataflow as gdf
    rng = np.random.default_rng(1)
    for (h, w, H, W) in ((112, 112, 1080, 960), (37, 53, 101, 77), (300, 200, 37, 23), (1, 17, 1, 40), (1, 40, 3, 17),
                         (17, 1, 40, 1), (112, 112, 112, 112)):
        m = rng.random((3, h, w)).astype(np.float32)
        got = gdf.resize_linear(m, (H, W))
        want = np.stack([odf.resize_linear(k, H, W) for k in m])
        assert got.shape == (3, H, W) and np.array_equal(got, want), (h, w, H, W)
    assert gdf.resize_linear(m[0], 5).shape == (5, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("n_other", [1500, 60, 0])
def test_auc_shuffled_matches_the_oracle(n_other):
    from sap3d_tensorflow_amd import metrics as gm
    rng = np.random.default_rng(n_other)
    s = rng.random((200, 150)).astype(np.float32)
    f = np.zeros((200, 150), np.float32)
    f.flat[rng.choice(s.size, 300, replace=False)] = 1
    o = np.zeros((200, 150), np.float32)
    o.flat[rng.choice(s.size, n_other, replace=False)] = 1
    for step in (0.1, 0.03):
        r1, r2 = np.random.RandomState(5), np.random.RandomState(5)
        got = gm.AUC_shuffled(s, f, o, n_rep=20, step_size=step, rng=r1)
        want = oev.AUC_shuffled(s, f, o, 20, step, rng=r2)[0]
        assert got == pytest.approx(want, abs=1e-12)
        assert np.array_equal(r1.get_state()[1], r2.get_state()[1])
    np.random.seed(8)
    a = gm.AUC_shuffled(s, f, o, n_rep=10)
    np.random.seed(8)
    assert a == pytest.approx(oev.AUC_shuffled(s, f, o, 10)[0], abs=1e-12)
    assert np.isnan(gm.AUC_shuffled(s, np.zeros_like(f), o))
    with pytest.raises(ValueError):
        gm.AUC_shuffled(s, f, o[:, :-1])
    with pytest.raises(NotImplementedError):
        gm.AUC_Borji(s, f, rand_sampler=lambda *a: None)          # AUC_Borji keeps refusing the sampler hook


def _eval_set(n, size=(1080, 960), seed=2, density_size=(270, 480)):
    from sap3d_tensorflow_amd import synthetic
    return synthetic.synthetic_test_set(seed, n, size=size, density_size=density_size)


@pytest.mark.gpu
def test_evaluate_matches_the_oracle_composition_at_full_resolution():
    x, dens, fix = _eval_set(3)                       # clip 2 has no fixation
    s = _session(3)
    pred = s.forward(x)[:, -1, :, :, 0]
    np.random.seed(11)
    got = s.evaluate(x, dens, fix)
    after = np.random.get_state()
    np.random.seed(11)
    want = [oev.test_py_clip_metrics(pred[b], dens[b], fix[b]) for b in range(3)]
    ref_state = np.random.get_state()
    assert np.array_equal(after[1], ref_state[1]) and after[2:] == ref_state[2:]
    for b in range(3):
        _check(got[b], want[b])
    assert np.isnan(got[2, 2:]).all() and np.isfinite(got[2, :2]).all()
    np.random.seed(11)
    again = s.evaluate(x, dens[:, None], fix[:, None])            # [B, T, H, W] maps: the last frame; bit-identical rerun
    assert np.array_equal(got, again, equal_nan=True)
    assert set(s.last_eval_ms) == {"forward", "draws", "h2d", "device"}
    np.random.seed(12)
    nj = s.evaluate(x, dens, fix, jitter=False, n_rep=7, step_size=0.05)
    np.random.seed(12)
    for b in range(3):
        _check(nj[b], oev.test_py_clip_metrics(pred[b], dens[b], fix[b], jitter=False, n_rep=7, step_size=0.05))
    s.close()


@pytest.mark.gpu
def test_evaluate_refuses_what_it_does_not_reproduce():
    from sap3d_tensorflow_amd import P3dError, lib
    x, dens, fix = _eval_set(2, size=(90, 80))
    s = _session(2)
    with pytest.raises(ValueError):
        s.evaluate(x, dens, fix, size=(1080, 960))                  # the reference's skimage branch
    s.evaluate(x, dens, fix, size=(90, 80))
    n_fix = np.count_nonzero(fix.reshape(2, -1) >= 128, axis=1).astype(np.int32)
    n_fix[0] += 1                                                     # disagrees with the device's count
    idx = np.zeros(int(n_fix.sum()) * 4, np.int32)
    out = np.empty((2, 5))
    u8 = C.POINTER(C.c_ubyte)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = lib().p3d_eval_last_frames(s._h, np.ascontiguousarray(dens).ctypes.data_as(u8), dens.shape[1], dens.shape[2],
                                    np.ascontiguousarray(fix).ctypes.data_as(u8), 90, 80, None, idx.ctypes.data_as(ip),
                                    n_fix.ctypes.data_as(ip), 4, 0.1, out.ctypes.data_as(dp), None)
    assert rc != 0 and b"n_fix" in lib().p3d_last_error()
    idx[0] = 90 * 80                                                   # an index past the map
    n_fix[0] -= 1
    rc = lib().p3d_eval_last_frames(s._h, np.ascontiguousarray(dens).ctypes.data_as(u8), dens.shape[1], dens.shape[2],
                                    np.ascontiguousarray(fix).ctypes.data_as(u8), 90, 80, None, idx.ctypes.data_as(ip),
                                    n_fix.ctypes.data_as(ip), 4, 0.1, out.ctypes.data_as(dp), None)
    assert rc != 0 and b"out of range" in lib().p3d_last_error()
    s.close()
    with pytest.raises(P3dError):
        f = np.zeros((20, 20), np.float32); f[3, 4] = 1
        lib_out = np.empty(3)
        rc = lib().p3d_metric_auc_shuffled(0, f.ctypes.data_as(C.POINTER(C.c_float)), f.ctypes.data_as(C.POINTER(C.c_float)),
                                           np.zeros(3, np.int32).ctypes.data_as(ip), 400, 2, 1, 3, 0.1, lib_out.ctypes.data_as(dp))
        from sap3d_tensorflow_amd._lib import check
        check(rc)                                                      # n_fix = 2, the map has 1


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(112, 112), (1080, 960)])
def test_full_resolution_reductions_agree_with_the_one_block_entry_points(size):
    """Same maps through both paths.  The density maps come at the target size with bytes 0 / 255 (the uint8 resize is then a
    copy and v / 255. is exact in float32, what the one-block kernels take); jitter is off (the one-block AUC_Judd adds
    float32 noise in float32)."""
    from sap3d_tensorflow_amd import dataflow as gdf
    from sap3d_tensorflow_amd import metrics as gm
    H, W = size
    x, dens, fix = _eval_set(3, size=size, seed=6, density_size=size)
    dens = np.where(dens >= 128, 255, 0).astype(np.uint8)
    s = _session(3)
    np.random.seed(4)
    got = s.evaluate(x, dens, fix, size=size, jitter=False, n_rep=20)
    pred = s.activation("pred")[:, -1, :, :, 0]
    full = gdf.resize_linear(pred, size)
    dmap = np.stack([gdf.mapf_density(d[None], size)[0] for d in dens])
    fmap = (fix >= 128).astype(np.float32)
    np.random.seed(4)
    for b in range(3):
        one = [gm.CC(full[b], dmap[b]), gm.SIM(full[b], dmap[b]), gm.AUC_Judd(full[b], fmap[b], jitter=False)]
        n_fix = int(fmap[b].sum())
        one.append(gm.AUC_Borji(full[b], fmap[b], n_rep=20, rand_idx=np.random.randint(0, H * W, [n_fix, 20])) if n_fix else np.nan)
        one.append(gm.NSS(full[b], fmap[b]))
        _check(got[b], one)
    s.close()


@pytest.mark.gpu
def test_driver_end_to_end_on_a_synthetic_set(tmp_path):
    import importlib.util
    from sap3d_tensorflow_amd import synthetic
    spec = importlib.util.spec_from_file_location("test_driver", os.path.join(ROOT, "drivers", "test.py"))
    d = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(d)
    s = _session(2)
    s.init_params(7)
    s.save_checkpoint(str(tmp_path), 5)
    args = ["--model", str(tmp_path), "--structure", "unet", "--base", "16", "--blocks", "2,2,3", "--batch", "2", "--clips", "5",
            "--seed", "3"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        cols = d.main(args)
    lines = buf.getvalue().splitlines()
    all_line = [l for l in lines if l.startswith(" All:")]
    # what the driver should have computed: evaluate on batches [0,2), [2,4) (clip 4 dropped), numpy seeded as --seed
    x, dens, fix = synthetic.synthetic_test_set(3, 5)
    np.random.seed(3)
    rows = np.concatenate([s.evaluate(x[lo:lo + 2], dens[lo:lo + 2], fix[lo:lo + 2]) for lo in (0, 2)])
    assert np.array_equal(np.array(cols).T, rows, equal_nan=True)
    assert all_line == [d.metric_line(d.ALL_LINE, 2, d.nan_dropped_means(rows.T.tolist()))]
    with contextlib.redirect_stdout(io.StringIO()):
        cols6 = d.main(args + ["--sauc", "2", "--time"])
    assert len(cols6) == 6 and np.array_equal(np.array(cols6[:5]), np.array(cols), equal_nan=True)
    assert all(0.0 <= v <= 1.0 or np.isnan(v) for v in cols6[5])
    s.close()
