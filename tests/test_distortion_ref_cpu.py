"""tests/distortion_ref.py, the numpy replay of include/p3d_hip.h's "Distortion of frames under their 8-bit maps", against the
properties the contract states, dataflow.distortion_report against a direct float64 computation, and the binding of the four new
entry points; no GPU.  The device tests (test_gpu_distortion.py) hold the kernels to this replay."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import distortion_ref as dr       # noqa: E402

LAW = dr.identity_law()


def inputs(n=2, H=21, W=26, seed=5):
    ref = dr.random_frames(n, H, W, seed)
    return dr.random_maps(n, H, W, seed + 1), ref, dr.near(ref, seed + 2)


def test_equal_frames():
    sal, ref, _ = inputs()
    table, blocks, qs = dr.distortion(sal, ref, ref, LAW, block=8, gate=100, with_q=True)
    for k in (dr.SSE, dr.WSSE, dr.MAXABS):
        assert (table[:, k:k + 4] == 0).all()
    assert (table[:, dr.CHANGED] == 0).all() and (table[:, dr.CHANGED_SALIENT] == 0).all() and (blocks == 0).all()
    assert all(q.size and (q == 65536).all() for q in qs)
    assert (table[:, dr.SQ] == 65536 * table[:, dr.NW]).all() and (table[:, dr.SWQ] == 65536 * table[:, dr.SWW]).all()
    assert (table[:, dr.SALIENT] == (sal >= 100).sum(axis=(1, 2))).all() and (table[:, dr.SW] == sal.astype(np.int64).sum(axis=(1, 2))).all()


def test_black_against_white():
    n, H, W = 2, 19, 23
    sal = dr.random_maps(n, H, W, 3)
    ref, test = np.zeros((n, H, W, 3), np.uint8), np.full((n, H, W, 3), 255, np.uint8)
    table, blocks = dr.distortion(sal, ref, test, np.full(256, 255, np.int32), block=16)
    assert (table[:, dr.SSE:dr.SSE + 4] == 65025 * H * W).all()            # every plane, Y included: Y(255, 255, 255) = 255
    assert (table[:, dr.WSSE:dr.WSSE + 4] == 255 * 65025 * H * W).all() and (table[:, dr.MAXABS:dr.MAXABS + 4] == 255).all()
    assert (table[:, dr.CHANGED] == H * W).all() and (table[:, dr.SALIENT] == 0).all()
    assert blocks.sum() == n * 3 * 65025 * H * W and blocks[0, 0, 0] == 3 * 65025 * 256 and blocks[0, 1, 1] == 3 * 65025 * 3 * 7


def textbook_ssim(a, b):
    """SSIM of one window in float64: unbiased variance and covariance, the unrounded constants."""
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    ma, mb = a.mean(), b.mean()
    va, vb = a.var(ddof=1), b.var(ddof=1)
    cov = ((a - ma) * (b - mb)).sum() / (a.size - 1)
    return (2 * ma * mb + c1) * (2 * cov + c2) / ((ma * ma + mb * mb + c1) * (va + vb + c2))


@pytest.mark.parametrize("kind", ["near", "unrelated", "inverted", "flat"])
def test_q_against_the_textbook(kind):
    H, W = 16, 20
    ref = dr.random_frames(1, H, W, 11)
    test = {"near": dr.near(ref, 12), "unrelated": dr.random_frames(1, H, W, 13), "inverted": 255 - ref,
            "flat": np.full_like(ref, 77)}[kind]
    ya, yb = dr.luma(ref[0]), dr.luma(test[0])
    _, _, qs = dr.distortion(np.zeros((1, H, W), np.uint8), ref, test, LAW, with_q=True)
    rows, cols = dr.windows(H, W)
    assert (len(rows), len(cols)) == (3, 4) and qs[0].shape == (3, 4)
    worst = 0.
    for j, y in enumerate(rows):
        for i, x in enumerate(cols):
            want = textbook_ssim(ya[y:y + 8, x:x + 8], yb[y:y + 8, x:x + 8])
            worst = max(worst, abs(qs[0][j, i] / 65536. - want))
    print(kind, "largest |q / 65536 - textbook SSIM|:", worst)
    # rounding q costs 0.5 / 65536; rounding c1 to 1 / 4096 and c2 to 1 / 4032 of a grey level squared moves the quotient by less
    # than that again
    assert worst <= 2. / 65536
    if kind == "inverted":
        assert qs[0].min() < 0                                 # num may be negative


def test_no_window_at_7_by_9():
    sal, ref, test = inputs(1, 7, 9)
    table, _ = dr.distortion(sal, ref, test, LAW)
    assert (table[0, [dr.NW, dr.SQ, dr.SWQ, dr.SWW]] == 0).all() and table[0, dr.SSE] > 0
    assert dr.distortion(*inputs(1, 8, 8), LAW)[0][0, dr.NW] == 1 and dr.distortion(*inputs(1, 12, 12), LAW)[0][0, dr.NW] == 4
    assert dr.distortion(*inputs(1, 9, 7), LAW)[0][0, dr.NW] == 0


def test_gate_and_counts():
    sal, ref, test = inputs(1, 10, 12)
    test[0, -1, -1] = ref[0, -1, -1]
    test[0, 0, 0, 1] = ref[0, 0, 0, 1] ^ 1
    for gate in (0, 1, 120, 255):
        table, _ = dr.distortion(sal, ref, test, LAW, gate=gate)
        salient = (sal[0] >= gate) if gate else np.zeros(sal[0].shape, bool)
        changed = (ref[0] != test[0]).any(axis=2)
        assert changed[0, 0] and not changed[-1, -1]
        assert table[0, dr.SALIENT] == salient.sum() and table[0, dr.CHANGED] == changed.sum()
        assert table[0, dr.CHANGED_SALIENT] == (salient & changed).sum()


def test_limits_and_config():
    sal, ref, test = inputs(1, 9, 9)
    dr.distortion(sal, ref, test, LAW, block=8, gate=255)
    for change in (dict(block=24), dict(block=4), dict(gate=256), dict(gate=-1)):
        with pytest.raises(ValueError):
            dr.distortion(sal, ref, test, LAW, **change)
    for bad in (256, -1):
        law = LAW.copy()
        law[7] = bad
        with pytest.raises(ValueError):
            dr.distortion(sal, ref, test, law)
    with pytest.raises(ValueError):
        dr.distortion(sal, ref, None, LAW)
    with pytest.raises(ValueError):
        dr.check(sal, ref, test, 0, 0, LAW, n=0)
    with pytest.raises(ValueError):
        dr.check(sal, ref, test, 0, 0, LAW, H=2048, W=4097)


# ---- dataflow's host side: the law and the report ----------------------------------------------------------------------------------
def test_the_law():
    from sap3d_tensorflow_amd import dataflow
    assert np.array_equal(dataflow.distortion_law(), np.arange(256)) and dataflow.distortion_law().dtype == np.int32
    law = dataflow.distortion_law(gate=100, floor=3)
    assert (law[:100] == 3).all() and np.array_equal(law[100:], np.arange(100, 256))
    law = dataflow.distortion_law(gamma=2.0)
    assert law[0] == 0 and law[255] == 255 and law[128] == int(np.floor(255 * (128 / 255.) ** 2 + 0.5)) and (np.diff(law) >= 0).all()
    for bad in (dict(gate=256), dict(gamma=0.), dict(gamma=float("nan")), dict(floor=256)):
        with pytest.raises(ValueError):
            dataflow.distortion_law(**bad)


def test_the_report_against_a_direct_computation():
    from sap3d_tensorflow_amd import dataflow
    n, H, W = 3, 16, 20
    sal, ref, test = inputs(n, H, W, seed=21)
    test[2] = ref[2]                                           # an SSE of 0
    sal[1] = 0                                                 # a weight sum of 0
    table, _ = dr.distortion(sal, ref, test, LAW, gate=50)
    rep = dataflow.distortion_report(table, H * W)
    assert all(v.dtype == np.float64 for v in rep.values())
    planes = [np.concatenate([f.astype(np.float64), dr.luma(f).astype(np.float64)[..., None]], axis=-1) for f in (ref, test)]
    w = sal.astype(np.float64)
    for f in range(n):
        err = (planes[0][f] - planes[1][f]) ** 2               # integers below 2^16 in float64: exact, and so are their sums
        mse = err.reshape(-1, 4).mean(axis=0)
        if f == 2:
            assert np.isposinf(rep["psnr"][f]).all() and np.isposinf(rep["wpsnr"][f]).all() and rep["ssim"][f] == 1.0 and rep["wssim"][f] == 1.0
            continue
        want = 10. * np.log10(255. ** 2 / mse)
        assert np.allclose(rep["psnr"][f], want, rtol=1e-12, atol=0.), (f, rep["psnr"][f], want)
        if f == 1:
            assert np.isnan(rep["wpsnr"][f]).all() and np.isnan(rep["wssim"][f]) and np.isnan(rep["changed_salient_share"][f])
            continue
        wmse = (err * w[f][..., None]).reshape(-1, 4).sum(axis=0) / w[f].sum()
        assert np.allclose(rep["wpsnr"][f], 10. * np.log10(255. ** 2 / wmse), rtol=1e-12, atol=0.)
        assert rep["ssim"][f] == table[f, dr.SQ] / (65536. * table[f, dr.NW]) and 0 < rep["ssim"][f] < 1
        assert rep["changed_salient_share"][f] == table[f, dr.CHANGED_SALIENT] / table[f, dr.SALIENT]
    none = dataflow.distortion_report(dr.distortion(*inputs(1, 7, 9), LAW)[0], 63)
    assert np.isnan(none["ssim"]).all() and np.isnan(none["wssim"]).all() and np.isnan(none["changed_salient_share"]).all()


# ---- the binding: include/p3d_hip.h through _header.py ------------------------------------------------------------------------------
def test_the_header_binds_the_four_entry_points():
    from sap3d_tensorflow_amd import _header
    h = _header.read()
    u8, i32, i64, ip, dp = (C.POINTER(t) for t in (C.c_ubyte, C.c_int32, C.c_int64, C.c_int, C.c_double))
    head = [C.c_int, u8, u8, u8, C.c_int, C.c_int, C.c_int, ip, i32]
    assert h.functions["p3d_distortion_u8"] == (C.c_int, head + [i64, i64])
    assert h.functions["p3d_debug_distortion_u8"] == (C.c_int, head + [C.c_int, i64, i64])
    assert h.functions["p3d_video_distortion"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, u8, u8, ip, i32,
                                                             i64, i64, u8, dp])
    assert h.functions["p3d_debug_distortion_plan"] == (C.c_int, [C.c_int] * 4 + [ip] * 5 + [i64])
    k = h.constants
    assert k["P3D_DISTORTION_FIELDS"] == 2 and (k["P3D_DISTORTION_BLOCK"], k["P3D_DISTORTION_GATE"]) == (0, 1)
    assert k["P3D_DISTORTION_RECORD"] == dr.RECORD
    names = ("SSE", "WSSE", "SW", "MAXABS", "CHANGED", "SALIENT", "CHANGED_SALIENT", "NW", "SQ", "SWQ", "SWW")
    assert [k["P3D_DISTORTION_" + s] for s in names] == [getattr(dr, s) for s in names]
