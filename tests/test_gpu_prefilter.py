"""The kernel of csrc/prefilter.hip behind qpmap.hip's grid launches, through p3d_prefilter_u8 and p3d_debug_prefilter_u8 (every device
buffer, the scratch included, between guards), against tests/prefilter_ref.py, tolerance 0 everywhere: the filtered frames and the
strength grid.  Frames are random bytes, so every off-by-one of a window shows; the maps are qpmap_ref's drifting blobs; the law falls
from 64 to 0.  Shapes are the smallest at which each mechanism can go wrong: rows of 3 W bytes that are no multiple of 16, shots with a
limiter, a radius beyond the frame, the largest radius, one pixel, one block, a tile's seams read from the plan, tiles that skip."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import prefilter_ref as pr        # noqa: E402
import qpmap_ref as qr            # noqa: E402

LAW = pr.falling_law(gate=160, full=20)
assert LAW.min() == 0 and LAW.max() == 64 and (np.diff(LAW) <= 0).all()

# (n, H, W, B, R, P), what else
SHAPES = [
    ((5, 37, 53, 8, 3, 2), dict(shots=(2,), rise=6, dilate=1)),      # 3 W = 159 is no multiple of 16
    ((6, 45, 70, 16, 2, 3), dict(shots=(1, 4))),
    ((3, 9, 7, 8, 16, 3), dict()),                                    # a radius beyond the frame
    ((2, 130, 267, 32, 16, 1), dict()),                               # the largest single-pass radius
    ((1, 1, 1, 8, 1, 1), dict()),                                     # the smallest frame
    ((2, 20, 24, 128, 4, 2), dict()),                                 # one block: a constant weight
]


@functools.lru_cache(maxsize=None)
def case(shape, shots=(), rise=0, fall=0, dilate=0, split=False):
    """The inputs and the replay of one case, computed once: (sal, frames, starts or None, cfg keywords, (out, grid, Wn))."""
    n, H, W, B, R, P = shape
    if split:
        sal, starts = np.zeros((n, H, W), np.uint8), None
        sal[:, :, :W // 2] = 255
    else:
        sal, starts = qr.frames(n, H, W, seed=7, shots=list(shots))
        starts = starts if shots else None
    frames = pr.random_frames(n, H, W, seed=H * W + R)
    kw = dict(block=B, peak_weight=128, dilate=dilate, fall=fall, rise=rise, radius=R, passes=P)
    want = pr.prefilter(sal, frames, LAW, shots=starts, **kw)
    for a in (sal, frames) + want:
        a.setflags(write=False)
    return sal, frames, starts, kw, want


def run(shape, offset=None, **more):
    from sap3d_tensorflow_amd import dataflow
    sal, frames, starts, kw, want = case(shape, **more)
    tag = (shape, sorted(more.items()), offset)
    for with_grid in (True, False):
        out, g = dataflow.prefilter(sal, frames, LAW, shots=starts, grid=with_grid, offset=offset, **kw)
        if with_grid:
            assert g.dtype == np.int32 and g.shape == want[1].shape, tag
            bad = np.argwhere(g != want[1])
            assert bad.size == 0, tag + ("grid", len(bad), bad[:4].tolist())
        else:
            assert g is None
        assert out.dtype == np.uint8 and out.shape == want[0].shape, tag
        bad = np.argwhere(out != want[0])
        assert bad.size == 0, tag + ("out", with_grid, len(bad), bad[:6].tolist(), [(int(out[tuple(b)]), int(want[0][tuple(b)])) for b in bad[:6]])
    return sal, frames, want


@pytest.mark.parametrize("shape,more", SHAPES, ids=[str(s[0]) for s in SHAPES])
def test_shapes(shape, more):
    sal, frames, (out, g, wn) = run(shape, **more)
    n, H, W, B, R, P = shape
    Q = 64 * (2 * B) ** 2
    if shape in (SHAPES[0][0], SHAPES[1][0], SHAPES[3][0]):           # on the replay: the case is no degenerate one
        print("share of pixels with 0 < Wn < Q:", ((wn > 0) & (wn < Q)).mean(), "of bytes changed:", (out != frames).mean())
        assert ((wn > 0) & (wn < Q)).mean() >= 0.5
        assert (out != frames).mean() >= 0.5
    if shape == SHAPES[0][0]:
        assert g.min() == 0 and g.max() == 64
    if shape == SHAPES[5][0]:
        assert g.shape[1:] == (1, 1) and all(len(np.unique(w)) == 1 for w in wn)


@pytest.mark.parametrize("offset", [0, 8, 5])
def test_hook_offsets(offset):
    shape, more = SHAPES[0]
    run(shape, offset=offset, **more)


def largest_halo(B=8):
    """(R, P) with the largest halo the plan fuses, or, where it fuses nothing, with the largest halo of a launch."""
    from sap3d_tensorflow_amd import dataflow
    plans = [((R, P), dataflow.prefilter_plan(64, 64, B, R, P)) for P in (1, 2, 3) for R in range(1, 17)]
    fused = [(p["halo"], rp) for rp, p in plans if p["fused"] and rp[1] > 1]
    if fused:
        return max(fused)[1]
    return max((p["halo"], rp) for rp, p in plans)[1]


def test_seams_of_a_tile():
    """One row more than a tile and three columns more than two tiles, under the largest halo."""
    from sap3d_tensorflow_amd import dataflow
    R, P = largest_halo()
    p = dataflow.prefilter_plan(64, 64, 8, R, P)
    H, W = p["tile_rows"] + 1, 2 * p["tile_cols"] + 3
    assert dataflow.prefilter_plan(H, W, 8, R, P)["blocks_per_frame"] == 6 and dataflow.prefilter_plan(H - 1, W - 3, 8, R, P)["blocks_per_frame"] == 2
    run((2, H, W, 8, R, P), shots=(1,), fall=3)


def test_both_sides_of_the_fused_switch():
    """Where the plan switches between the passes inside one launch and launches through memory: a case either side of the switch.
    Where it does not switch, the one form at the smallest and the largest multi-pass halo."""
    from sap3d_tensorflow_amd import dataflow
    forms = {(R, P): dataflow.prefilter_plan(64, 64, 8, R, P)["fused"] for P in (2, 3) for R in range(1, 17)}
    picks = []
    for P in (2, 3):
        for R in range(1, 16):
            if forms[(R, P)] != forms[(R + 1, P)]:
                picks += [(R, P), (R + 1, P)]
    if not picks:
        assert len(set(forms.values())) == 1
        picks = [(1, 3), (16, 2)]
    for R, P in picks[:4]:
        run((2, 40, 75, 8, R, P))


def test_tiles_that_skip():
    """Maps 255 in the left half and 0 in the right: whole tiles have Wn = 0 (copied) and whole tiles have Wn = Q (no blend)."""
    from sap3d_tensorflow_amd import dataflow
    shape = (2, 64, 160, 8, 4, 2)
    sal, frames, (out, g, wn) = run(shape, split=True)
    p = dataflow.prefilter_plan(64, 160, 8, 4, 2)
    th, tw = p["tile_rows"], p["tile_cols"]
    Q = 64 * 16 * 16
    tiles = [wn[0, y:y + th, x:x + tw] for y in range(0, 64, th) for x in range(0, 160, tw)]
    assert any((t == 0).all() for t in tiles) and any((t == Q).all() for t in tiles)
    zero = wn == 0
    assert zero.any() and np.array_equal(out[zero], frames[zero])
    assert (out[wn == Q] != frames[wn == Q]).mean() > 0.5


def test_one_frame_more_than_a_chunk():
    """The intermediate passes are held a chunk of frames at a time, and the chunk is sized in bytes, so only large frames overflow
    it.  The replay of whole frames this large is slow: the grid and the weights are replayed whole, the low-pass on a window of rows
    with a margin of R P rows, inside which it is exact -- in the first chunk and in the second."""
    from sap3d_tensorflow_amd import dataflow
    H, W, B, R, P = 2048, 3000, 128, 2, 2
    chunk = dataflow.prefilter_plan(H, W, B, R, P, 65535)["frames_per_chunk"]
    assert chunk == 3 and dataflow.prefilter_plan(H, W, B, R, 1, 65535)["scratch_bytes"] == 0
    n = chunk + 1
    base = pr.random_frames(1, H, W, 3)[0]
    frames = np.stack([base ^ np.uint8(37 * m) for m in range(n)])
    ramp = (np.arange(W, dtype=np.int64)[None, :] * 255 // (W - 1) + np.arange(H, dtype=np.int64)[:, None] // 64)
    sal = np.stack([np.clip(ramp + 20 * m, 0, 255).astype(np.uint8) for m in range(n)])
    out, g = dataflow.prefilter(sal, frames, LAW, block=B, radius=R, passes=P, rise=5, grid=True)
    want_g = pr.grid(sal, LAW, block=B, rise=5)
    assert np.array_equal(g, want_g) and g.min() == 0 and g.max() == 64
    y0, y1, m = 1000, 1040, R * P
    for f in (0, chunk - 1, chunk):
        wn = pr.weight(want_g[f], H, W, B)[y0:y1]
        low = pr.low_pass(frames[f, y0 - m:y1 + m], R, P)[m:-m]
        want, _ = pr.blend(frames[f, y0:y1], low, wn, B)
        assert 0 < wn.min() or wn.max() > 0
        assert np.array_equal(out[f, y0:y1], want.astype(np.uint8)), f
    assert not np.array_equal(out[chunk], out[0])


# ---- the plan's division ------------------------------------------------------------------------------------------------------------
def test_the_plan_divides_exactly():
    from sap3d_tensorflow_amd import dataflow
    for R in range(1, 17):
        p = dataflow.prefilter_plan(64, 64, 8, R, 1)
        A = (2 * R + 1) ** 2
        x = np.arange(0, 2 * 255 * A + A + 1, dtype=np.uint64)
        assert p["mul"] < 2 ** 32 and 0 < p["shift"] <= 32
        assert np.array_equal((x * np.uint64(p["mul"])) >> np.uint64(p["shift"]), x // np.uint64(2 * A)), R


# ---- refusals: -1, p3d_last_error set, nothing written -------------------------------------------------------------------------------
def raw_call(sal, frames, cfg, law, out, H=None, W=None, hook="p3d_debug_prefilter_u8"):
    from sap3d_tensorflow_amd import _lib
    u8, i32 = C.POINTER(C.c_ubyte), C.POINTER(C.c_int32)
    lib = _lib.lib()
    args = [0, sal.ctypes.data_as(u8), None if frames is None else frames.ctypes.data_as(u8), sal.shape[0], sal.shape[1] if H is None else H,
            sal.shape[2] if W is None else W, cfg, law.ctypes.data_as(i32), None, 0]
    if hook == "p3d_debug_prefilter_u8":
        args.append(3)
    args += [None if out is None else out.ctypes.data_as(u8), None]
    rc = getattr(lib, hook)(*args)
    return rc, lib.p3d_last_error().decode()


@pytest.mark.parametrize("hook", ["p3d_debug_prefilter_u8", "p3d_prefilter_u8"])
def test_refusals(hook):
    from sap3d_tensorflow_amd import dataflow
    sal, frames, _, _, _ = case(SHAPES[0][0], **SHAPES[0][1])
    sal, frames = np.ascontiguousarray(sal), np.ascontiguousarray(frames)
    good = dict(block=8, peak_weight=128, dilate=0, fall=0, rise=0, radius=3, passes=2)

    def refused(words, law=LAW, no_frames=False, null_out=False, H=None, W=None, **change):
        out = np.full(frames.shape, 0x5a, np.uint8)
        rc, msg = raw_call(sal, None if no_frames else frames, dataflow.prefilter_cfg(**dict(good, **change)), law, None if null_out else out,
                           H=H, W=W, hook=hook)
        assert rc == -1 and msg and all(w in msg for w in words), (change, rc, msg)
        assert (out == 0x5a).all()

    rc, _ = raw_call(sal, frames, dataflow.prefilter_cfg(**good), LAW, np.empty(frames.shape, np.uint8), hook=hook)
    assert rc == 0
    for block in (0, 4, 12, 256):
        refused(["block"], block=block)
    refused(["peak_weight"], peak_weight=257)
    refused(["peak_weight"], peak_weight=-1)
    refused(["dilate"], dilate=9)
    refused(["dilate"], dilate=-1)
    refused(["fall"], fall=65)
    refused(["fall"], fall=-1)
    refused(["rise"], rise=65)
    refused(["rise"], rise=-1)
    refused(["radius"], radius=0)
    refused(["radius"], radius=17)
    refused(["passes"], passes=0)
    refused(["passes"], passes=4)
    for v in (65, -1):
        bad = LAW.copy()
        bad[200] = v
        refused(["law[200]", str(v)], law=bad)
    refused(["null"], no_frames=True)
    refused(["null"], null_out=True)
    refused(["H * W"], H=2048, W=4097)                         # above 2^23: refused before anything is read
