"""The kernels of csrc/distortion.hip through p3d_distortion_u8 and p3d_debug_distortion_u8 (every device buffer between guards),
against tests/distortion_ref.py: every integer of the table and of the block map equal, SSIM's included.  Shapes are the smallest
that reach each edge: one window, no window, windows that straddle the SSIM launch's tiles, rows of W and 3 W bytes that are no
multiple of 16, edge blocks, more than one frame, more than one tile of the sums' launch.  Black against white under a law of 255 is
the accumulator-width case: a 32-bit partial sum overflows after 259 such pixels."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import distortion_ref as dr       # noqa: E402

# a law with no structure, so that a wrong lookup shows; both ends of the range are in it
LAW = np.random.RandomState(1).randint(0, 256, 256).astype(np.int32)
LAW[0], LAW[255], LAW[17] = 0, 255, 255
LAW.setflags(write=False)
FULL = np.full(256, 255, np.int32)
GATE = 128

# (n, H, W), blocks
SHAPES = [
    ((1, 8, 8), (0, 8)),              # one window
    ((1, 7, 9), (0, 8)),              # no window
    ((1, 12, 12), (0, 16)),           # 2 x 2 windows
    ((1, 9, 17), (0, 8)),             # W and 3 W are no multiples of 16
    ((1, 33, 65), (0, 32)),           # one pixel past a 32 x 64 tile each way: windows straddle tiles
    ((1, 40, 70), (8, 16)),           # edge blocks
    ((3, 64, 128), (0, 64)),
    ((2, 270, 480), (0, 128)),
]
IDS = ["%dx%dx%d" % s[0] for s in SHAPES]


@functools.lru_cache(maxsize=None)
def frames_of(shape, content):
    """(sal, ref, test) of one case, read-only."""
    n, H, W = shape
    seed = H * W + n
    sal = dr.random_maps(n, H, W, seed)
    if content == "random":
        ref = dr.random_frames(n, H, W, seed + 1)
        test = dr.near(ref, seed + 2)
        test[:, : H // 2] = dr.random_frames(n, H, W, seed + 3)[:, : H // 2]       # unrelated in the upper half: large differences too
    elif content == "black_white":
        ref, test = np.zeros((n, H, W, 3), np.uint8), np.full((n, H, W, 3), 255, np.uint8)
    elif content == "equal":
        ref = dr.random_frames(n, H, W, seed + 1)
        test = ref.copy()
    elif content == "last_byte":
        ref = dr.random_frames(n, H, W, seed + 1)
        test = ref.copy()
        test[-1, -1, -1, 2] ^= 0x80
    else:
        raise KeyError(content)
    for a in (sal, ref, test):
        a.setflags(write=False)
    return sal, ref, test


@functools.lru_cache(maxsize=None)
def want_of(shape, content, block, gate, full=False, level=None):
    sal, ref, test = frames_of(shape, content)
    if level is not None:
        sal = np.full_like(sal, level)
    table, blocks = dr.distortion(sal, ref, test, FULL if full else LAW, block=block, gate=gate)
    table.setflags(write=False)
    return sal, ref, test, table, blocks


def run(shape, content, block, gate=GATE, offset=None, full=False, level=None, block_map=None):
    from sap3d_tensorflow_amd import dataflow
    sal, ref, test, table, blocks = want_of(shape, content, block, gate, full, level)
    tag = (shape, content, block, gate, offset, full, level)
    got, bs = dataflow.distortion(sal, ref, test, (block, gate), FULL if full else LAW, block_map=block_map, offset=offset)
    assert got.dtype == np.int64 and got.shape == table.shape, tag
    bad = np.argwhere(got != table)
    assert bad.size == 0, tag + ("table", bad[:8].tolist(), [(int(got[tuple(b)]), int(table[tuple(b)])) for b in bad[:8]])
    if block and block_map is not False:
        assert bs.dtype == np.int64 and bs.shape == blocks.shape, tag
        bad = np.argwhere(bs != blocks)
        assert bad.size == 0, tag + ("block_sse", len(bad), bad[:6].tolist())
        assert bs.sum() == got[:, dr.SSE:dr.SSE + 3].sum()
    else:
        assert bs is None
    return got


@pytest.mark.parametrize("shape,blocks", SHAPES, ids=IDS)
def test_shapes(shape, blocks):
    for block in blocks:
        got = run(shape, "random", block)
        run(shape, "random", block, offset=5)
    n, H, W = shape
    rows, cols = dr.windows(H, W)
    assert (got[:, dr.NW] == len(rows) * len(cols)).all()
    if len(rows):                                              # on the replay: the case is no degenerate one
        assert (got[:, dr.SQ] != 0).all() and (got[:, dr.SQ] < 65536 * got[:, dr.NW]).all()
    assert (got[:, dr.CHANGED] > 0).all() and (got[:, dr.SALIENT] > 0).all() and (got[:, dr.MAXABS:dr.MAXABS + 4] > 0).all()


def test_the_block_map_is_optional():
    run((1, 40, 70), "random", 16, block_map=False)


@pytest.mark.parametrize("shape", [(3, 64, 128), (2, 270, 480)], ids=["3x64x128", "2x270x480"])
def test_black_against_white_under_a_full_law(shape):
    """The accumulator-width case: every pixel adds 255 * 255^2 to WSSE."""
    n, H, W = shape
    for offset in (None, 0):
        got = run(shape, "black_white", 8, full=True, offset=offset)
    assert (got[:, dr.WSSE:dr.WSSE + 4] == 255 * 65025 * H * W).all() and 255 * 65025 * H * W > 2 ** 32
    assert (got[:, dr.SSE:dr.SSE + 4] == 65025 * H * W).all()


@pytest.mark.parametrize("shape", [(1, 33, 65), (3, 64, 128)], ids=["1x33x65", "3x64x128"])
def test_equal_frames(shape):
    got = run(shape, "equal", 16)
    assert (got[:, dr.SQ] == 65536 * got[:, dr.NW]).all() and (got[:, :dr.SW] == 0).all() and (got[:, dr.NW] > 0).all()


@pytest.mark.parametrize("shape", [(1, 9, 17), (1, 33, 65), (3, 64, 128)], ids=["1x9x17", "1x33x65", "3x64x128"])
def test_one_byte_at_the_last_pixel(shape):
    got = run(shape, "last_byte", 8, offset=7)
    assert (got[:-1, dr.CHANGED] == 0).all() and got[-1, dr.CHANGED] == 1 and got[-1, dr.MAXABS + 2] == 128
    assert got[-1, dr.SSE + 2] == 128 * 128 and got[-1, dr.SSE] == 0 and got[-1, dr.SSE + 3] > 0


@pytest.mark.parametrize("level", [0, GATE - 1, GATE])
def test_constant_maps(level):
    shape = (1, 40, 70)
    got = run(shape, "random", 0, level=level)
    assert got[0, dr.SALIENT] == (40 * 70 if level >= GATE else 0) and got[0, dr.SW] == int(LAW[level]) * 40 * 70
    assert got[0, dr.CHANGED_SALIENT] == (got[0, dr.CHANGED] if level >= GATE else 0)
    run(shape, "random", 0, gate=0, level=level)               # gate = 0: nothing is salient


@pytest.mark.parametrize("offset", range(16))
def test_hook_offsets(offset):
    run((2, 13, 37), "random", 8, offset=offset)


def test_the_plan_counts_the_windows():
    from sap3d_tensorflow_amd import dataflow
    for (n, H, W), blocks in SHAPES + [((1, 13, 37), (8,)), ((1, 1080, 1920), (16,))]:
        p = dataflow.distortion_plan(H, W, blocks[-1], n)
        rows, cols = dr.windows(H, W)
        assert (p["window_rows"], p["window_cols"]) == (len(rows), len(cols)), (H, W, p)
        assert p["blocks_per_frame"] == -(-H // p["tile_rows"]) * -(-W // p["tile_cols"]) and p["scratch_bytes"] >= 0
    for H, W in ((8, 8), (12, 12), (33, 65)):                  # against the replay's own count
        sal, ref, test = frames_of((1, H, W), "random")
        p = dataflow.distortion_plan(H, W)
        assert p["window_rows"] * p["window_cols"] == dr.distortion(sal, ref, test, LAW)[0][0, dr.NW]


# ---- refusals: -1, p3d_last_error set, nothing written -------------------------------------------------------------------------------
def raw_call(hook, sal, ref, test, cfg, law, table, block_sse, n=None, H=None, W=None):
    from sap3d_tensorflow_amd import _lib
    u8, i32, i64 = C.POINTER(C.c_ubyte), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    lib = _lib.lib()

    def p(a, t):
        return None if a is None else a.ctypes.data_as(t)
    args = [0, p(sal, u8), p(ref, u8), p(test, u8), sal.shape[0] if n is None else n, sal.shape[1] if H is None else H,
            sal.shape[2] if W is None else W, cfg, p(law, i32)]
    if hook == "p3d_debug_distortion_u8":
        args.append(3)
    args += [p(table, i64), p(block_sse, i64)]
    rc = getattr(lib, hook)(*args)
    return rc, lib.p3d_last_error().decode()


@pytest.mark.parametrize("hook", ["p3d_debug_distortion_u8", "p3d_distortion_u8"])
def test_refusals(hook):
    from sap3d_tensorflow_amd import dataflow
    sal, ref, test = (np.ascontiguousarray(a) for a in frames_of((1, 40, 70), "random"))
    FILL = 0x5a5a5a5a5a5a5a5a

    def call(block=8, gate=GATE, law=LAW, no_test=False, with_map=True, **shape):
        table, bs = np.full((1, dr.RECORD), FILL, np.int64), np.full((1, 5, 9), FILL, np.int64)
        rc, msg = raw_call(hook, sal, ref, None if no_test else test, dataflow.distortion_cfg(block, gate), np.ascontiguousarray(law), table,
                           bs if with_map else None, **shape)
        return rc, msg, table, bs

    def refused(words, **change):
        rc, msg, table, bs = call(**change)
        assert rc == -1 and msg and all(w in msg for w in words), (change, rc, msg)
        assert (table == FILL).all() and (bs == FILL).all()

    rc, _, table, bs = call()
    assert rc == 0 and np.array_equal(table, want_of((1, 40, 70), "random", 8, GATE)[3]) and (bs != FILL).all()
    refused(["null"], no_test=True)
    refused(["block map", "0"], block=0)
    refused(["block", "24"], block=24)
    bad = LAW.copy()
    bad[200] = 256
    refused(["wlaw[200]", "256"], law=bad)
    refused(["gate"], gate=256)
    refused(["maps"], n=0)
    refused(["H * W"], H=2048, W=4097)                         # above 2^23: refused before anything is read
    assert call(block=0, with_map=False)[0] == 0
