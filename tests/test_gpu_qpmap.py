"""The kernels of csrc/qpmap.hip through p3d_debug_qpmap_u8 (every device buffer, the scratch included, between guards) against
tests/qpmap_ref.py, tolerance 0 everywhere: the offsets, the levels and the statistics.  Shapes are the smallest at which each path
can go wrong: one partial block, two blocks to a 16-byte word, rows that straddle words, blocks wider than a lane's word, a grid of
more than 64 blocks, one map more than a chunk holds, and the saliency bytes at every phase of a 16-byte word."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import qpmap_ref as qr        # noqa: E402

SHAPES = [(1, 1, 8), (5, 7, 8), (9, 33, 8), (33, 70, 16), (33, 70, 64), (64, 130, 32), (130, 64, 128), (64, 130, 8)]
LAW = qr.linear_law(-20, 6)


@functools.lru_cache(maxsize=None)
def blobs(n, H, W, seed=3):
    b = qr.blobs(n, H, W, seed)
    b.setflags(write=False)
    return b


def check(sal, law=LAW, block=16, peak_weight=128, dilate=0, fall=0, rise=0, balance=1, target=0, lo=-127, hi=127, shots=None, offset=0,
          what=""):
    from sap3d_tensorflow_amd import dataflow
    want = qr.qpmap(sal, law, block, peak_weight, dilate, fall, rise, balance, target, lo, hi, shots)
    kw = dict(block=block, peak_weight=peak_weight, dilate=dilate, fall=fall, rise=rise, balance=balance, target=target, lo=lo, hi=hi,
              shots=shots, offset=offset)
    tag = (what, sal.shape, sorted(kw.items()))
    for full in (True, False):                             # with levels and statistics, and without: the same offsets
        qp, lev, st = dataflow.qpmap(sal, law, levels=full, stats=full, **kw)
        assert qp.dtype == np.int32 and qp.shape == want[0].shape, tag
        bad = np.argwhere(qp != want[0])
        assert bad.size == 0, tag + ("qp", full, len(bad), bad[:4].tolist(), [(int(qp[tuple(b)]), int(want[0][tuple(b)])) for b in bad[:4]])
        if full:
            assert lev.dtype == np.uint8 and st.dtype == np.int32
            bad = np.argwhere(lev != want[1])
            assert bad.size == 0, tag + ("levels", len(bad), bad[:4].tolist(), [(int(lev[tuple(b)]), int(want[1][tuple(b)])) for b in bad[:4]])
            assert np.array_equal(st, want[2]), tag + ("stats", st[:4].tolist(), want[2][:4].tolist())
        else:
            assert lev is None and st is None
    return want


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", [1, 3])
def test_shapes(shape, n):
    H, W, B = shape
    want = check(blobs(n, H, W), block=B, dilate=1, fall=1, rise=3, what="blobs")
    assert want[0].shape == (n, -(-H // B), -(-W // B))
    if shape == (64, 130, 8):
        assert want[0].shape[1] * want[0].shape[2] > 64


@pytest.mark.parametrize("shape", [(33, 70, 16), (9, 33, 8), (130, 64, 128)])
def test_one_map_more_than_a_chunk(shape):
    from sap3d_tensorflow_amd import dataflow
    H, W, B = shape
    chunk = dataflow.qpmap_plan(H, W, B, 65535)["maps_per_chunk"]
    assert 1 <= chunk <= 256
    n = chunk + 1
    assert dataflow.qpmap_plan(H, W, B, n)["maps_per_chunk"] == chunk
    sal = np.concatenate([blobs(8, H, W, seed=k) for k in range(-(-n // 8))])[:n]
    check(sal, block=B, dilate=1, fall=2, rise=1, shots=sorted({0, chunk - 1, chunk, n - 1}), what="chunk + 1")


@pytest.mark.parametrize("B", [8, 64])
def test_two_tiles_to_a_row(B):
    from sap3d_tensorflow_amd import dataflow
    H, W = 9, 4113                                            # one 16-byte word more than a tile is wide
    assert dataflow.qpmap_plan(H, W - 17, B)["blocks_per_map"] * 2 == dataflow.qpmap_plan(H, W, B)["blocks_per_map"]
    check(blobs(2, H, W), block=B, dilate=1, what="two tiles")


@pytest.mark.parametrize("B", [8, 16])
@pytest.mark.parametrize("offset", range(16))
def test_every_offset(B, offset):
    check(blobs(2, 33, 70), block=B, dilate=1, offset=offset, what="offset")


@pytest.mark.parametrize("peak_weight", [0, 128, 256])
@pytest.mark.parametrize("dilate", [0, 1, 8])
def test_peak_weight_and_dilate(peak_weight, dilate):
    check(blobs(2, 33, 70), block=8, peak_weight=peak_weight, dilate=dilate, what="level")      # a 5 x 9 grid: 8 exceeds it
    check(blobs(2, 33, 70), block=64, peak_weight=peak_weight, dilate=dilate, what="level")


@pytest.mark.parametrize("fall,rise", [(0, 0), (1, 3), (254, 1)])
def test_limiter_with_and_without_shots(fall, rise):
    sal, starts = qr.frames(9, 33, 70, seed=4, shots=[3, 4, 8])      # adjacent starts, and the last frame
    assert starts.tolist() == [0, 3, 4, 8]
    law = qr.linear_law(-100, 100)                            # steps large enough for 254 to bind nothing and 1 to bind everything
    free = check(sal, law=law, block=16, fall=fall, rise=rise, balance=0, what="no shots")
    cut = check(sal, law=law, block=16, fall=fall, rise=rise, balance=0, shots=starts, what="shots")
    if (fall, rise) == (1, 3):
        assert not np.array_equal(free[0], cut[0])            # the table matters


@pytest.mark.parametrize("balance", [0, 1])
def test_balance_and_saturation_on_a_negative_sum(balance):
    law = qr.linear_law(-90, -3)                              # every offset negative: S1 < 0
    want = check(blobs(3, 33, 70), law=law, block=8, balance=balance, target=-4, lo=-30, hi=-2, what="negative")
    assert (want[2][:, 2] < 0).all() and (want[2][:, 0] == -30).any()           # S1 < 0, and the clamp binds
    want = check(blobs(3, 64, 130), law=law, block=32, balance=balance, target=0, lo=-5, hi=5, what="negative")
    assert (want[2][:, 2] < 0).all()


@pytest.mark.parametrize("value", [0, 255])
@pytest.mark.parametrize("shape", [(33, 70, 8), (33, 70, 16), (130, 64, 128)])
def test_flat_maps(value, shape):
    H, W, B = shape
    for balance in (0, 1):
        want = check(np.full((2, H, W), value, np.uint8), block=B, balance=balance, target=2, what="flat")
        assert (want[1] == value).all() and (want[0] == (2 if balance else LAW[value])).all()


# ---- refusals: an error, p3d_last_error set, nothing written ------------------------------------------------------------------------
def raw_call(sal, cfg, law, qp, n=None, shots=None, hook="p3d_debug_qpmap_u8"):
    from sap3d_tensorflow_amd import _lib
    u8, i32 = C.POINTER(C.c_ubyte), C.POINTER(C.c_int32)
    lib = _lib.lib()
    n = sal.shape[0] if n is None else n
    st = None if shots is None else np.ascontiguousarray(shots, np.int32)
    args = [0, sal.ctypes.data_as(u8), n, sal.shape[1], sal.shape[2], cfg, law.ctypes.data_as(i32),
            None if st is None else st.ctypes.data_as(i32), 0 if st is None else len(st)]
    if hook == "p3d_debug_qpmap_u8":
        args.append(3)
    args += [None if qp is None else qp.ctypes.data_as(i32), None, None]
    rc = getattr(lib, hook)(*args)
    return rc, lib.p3d_last_error().decode()


@pytest.mark.parametrize("hook", ["p3d_debug_qpmap_u8", "p3d_qpmap_u8"])
def test_refusals(hook):
    from sap3d_tensorflow_amd import dataflow
    sal = np.ascontiguousarray(blobs(2, 33, 70))
    good = dict(block=16, peak_weight=128, dilate=0, fall=0, rise=0, balance=1, target=0, lo=-10, hi=10)
    sentinel = -(2 ** 31) + 5

    def refused(words, law=LAW, n=None, null_qp=False, shots=None, **change):
        qp = np.full((2, 3, 5), sentinel, np.int32)
        rc, msg = raw_call(sal, dataflow.qpmap_cfg(**dict(good, **change)), law, None if null_qp else qp, n=n, shots=shots, hook=hook)
        assert rc != 0 and msg and all(w in msg for w in words), (change, rc, msg)
        assert (qp == sentinel).all()

    rc, _ = raw_call(sal, dataflow.qpmap_cfg(**good), LAW, np.empty((2, 3, 5), np.int32), hook=hook)
    assert rc == 0
    for block in (0, 4, 12, 24, 256):
        refused(["block"], block=block)
    refused(["lo", "hi"], lo=3, hi=2, target=2)
    refused(["target"], target=11)
    refused(["target"], target=-11)
    refused(["-127"], lo=-128)
    refused(["127"], hi=128)
    bad = LAW.copy()
    bad[200] = 128
    refused(["law[200]", "128"], law=bad)
    bad[200] = -128
    refused(["law[200]"], law=bad)
    refused(["maps"], n=0)
    refused(["null"], null_qp=True)
    refused(["peak_weight"], peak_weight=257)
    refused(["dilate"], dilate=9)
    refused(["fall"], fall=255)
    refused(["rise"], rise=-1)
    refused(["balance"], balance=2)
    refused(["shot"], shots=[0, 2])                          # a start outside the call


def test_plan_limits_and_shape():
    from sap3d_tensorflow_amd import dataflow
    from sap3d_tensorflow_amd._lib import P3dError
    p = dataflow.qpmap_plan(1080, 960, 16, 64)
    assert p["strip_rows"] == 16 and p["tile_cols"] == 960 and p["blocks_per_map"] == 68 and 1 <= p["maps_per_chunk"] <= 64
    assert p["scratch_bytes"] >= p["maps_per_chunk"] * 68 * 60
    assert dataflow.qpmap_plan(2048, 4096, 64, 1)["blocks_per_map"] == 32 and dataflow.qpmap_plan(1024, 8192, 64, 1)["blocks_per_map"] == 32
    assert dataflow.qpmap_plan(2048, 4096, 128, 1)["maps_per_chunk"] == 1            # H * W = 2^23 is legal
    for args in [(2048, 4097, 16, 1), (0, 4, 16, 1), (4, 4, 12, 1), (4, 4, 16, 0), (4, 4, 16, 65536)]:
        with pytest.raises(P3dError):
            dataflow.qpmap_plan(*args)
