"""No-GPU checks of the BatchNorm statistics-partial bookkeeping (host code only): every conv that feeds a BatchNorm writes
at most as many (sum, sum of squares) partials as the network reserves for them, whichever kernel the plan picks -- the tiled
implicit GEMM (one partial per output-row tile of every launch of the group), the K-sliced tail, the residue classes of a
transposed conv, or the weights-resident streaming 1x1x1 kernel (one per block, up to 512).  A producer that wrote more would
make the forward throw "statistics partials overflow their arena slot"."""
import numpy as np
import pytest

from sap3d_tensorflow_amd import _lib, ops


def _rows():
    r = set(range(1, 2049)) | set(range(16384 - 256, 16384 + 257)) | set(range(27648 - 256, 27648 + 257))
    r |= set(range(32, 200001, 32 * 7)) | set(range(64, 200001, 64 * 5)) | {20480, 27616, 50176, 100352, 200000, 199999}
    r |= set(np.geomspace(1, 200000, 400).astype(int).tolist())
    return sorted(r)


ROWS = _rows()
CHANNELS = (4, 8, 16, 64, 128, 192, 256, 504, 512, 520, 1024)
TAPS = ((1, 1, 1), (1, 3, 3), (3, 1, 1), (3, 3, 3))


def _sweep(cins, channels, taps, rows):
    bad = []
    for k in taps:
        for cin in cins:
            for c in channels:
                for m in rows:
                    written, cap = ops.stat_parts((1, 1, 1, m, cin), k + (cin, c), (1, 1, 1))
                    if written > cap:
                        bad.append((k, cin, c, m, written, cap))
    return bad


@pytest.mark.parametrize("taps", TAPS, ids=lambda k: "x".join(map(str, k)))
def test_conv_partials_fit_their_slot(taps):
    """Forward convs, stride 1, over the row sweep (dense around 1024, 16384 and 27648); the K = 64 input covers the streaming
    kernel at 64 / 128 / 256 output channels."""
    rows = ROWS if taps == (1, 1, 1) else ROWS[::3]
    bad = _sweep((4, 64, 256), CHANNELS, [taps], rows)
    assert not bad, "%d overflowing shapes, first: %s" % (len(bad), bad[:5])


def test_streaming_window_fits():
    """The case that overflowed: K = 64 -> 128 channels, 1x1x1, M % 32 == 0 from M = 16384 on (512 streaming blocks against
    M / 64 + 80 reserved below M = 27648)."""
    for m in (16384, 16416, 20480, 27616, 27648, 50176):
        written, cap = ops.stat_parts((1, 1, 1, m, 64), (1, 1, 1, 64, 128), (1, 1, 1))
        assert written == 512 and written <= cap, (m, written, cap)


def test_small_tensor_threshold():
    """M <= 1024 with C % 8 == 0 goes to the one-launch small-tensor BatchNorm: no epilogue partials and no slot."""
    assert ops.stat_parts((1, 1, 1, 1024, 64), (1, 1, 1, 64, 64), (1, 1, 1)) == (0, 0)
    w, c = ops.stat_parts((1, 1, 1, 1025, 64), (1, 1, 1, 64, 64), (1, 1, 1))
    assert 0 < w <= c
    w, c = ops.stat_parts((1, 1, 1, 1024, 64), (1, 1, 1, 64, 12), (1, 1, 1))      # C % 8 != 0: the tiled path's partials
    assert 0 < w <= c


def test_strided_stem_and_transposed_partials_fit():
    bad = []
    for n, d, h, w in ((1, 4, 16, 16), (2, 16, 28, 28), (2, 8, 56, 56), (8, 16, 56, 56), (1, 3, 17, 23), (2, 16, 112, 112)):
        for c in (16, 64, 256, 512):
            for k, s in (((3, 3, 3), (2, 2, 2)), ((1, 3, 3), (1, 2, 2)), ((1, 1, 1), (2, 2, 2))):
                cin = 64
                wr, cap = ops.stat_parts((n, d, h, w, cin), k + (cin, c), s)
                if wr > cap:
                    bad.append(("conv", n, d, h, w, c, k, s, wr, cap))
                wr, cap = ops.stat_parts((n, d, h, w, cin), k + (c, cin), s, transpose=True)
                if wr > cap:
                    bad.append(("deconv", n, d, h, w, c, k, s, wr, cap))
        wr, cap = ops.stat_parts((n, d, h * 2, w * 2, 3), (1, 7, 7, 3, 64), (1, 2, 2))      # the stem on its packed form
        if wr > cap:
            bad.append(("stem", n, d, h, w, wr, cap))
    assert not bad, bad[:5]


def test_forced_plans_fit():
    """Every tile a test may force (p3d_debug_force_plan), with and without K-slices, keeps the streaming kernel out and
    still fits."""
    lib = _lib.lib()
    try:
        for tile in (0, 1, 2):
            for splits in (0, 2, 4):
                _lib.check(lib.p3d_debug_force_plan(tile, splits, 0, 0))
                bad = _sweep((64,), (64, 128, 256, 520), [(1, 1, 1), (1, 3, 3)], ROWS[::9])
                assert not bad, (tile, splits, bad[:5])
    finally:
        _lib.check(lib.p3d_debug_force_plan(-1, 0, 0, 0))


def test_streaming_siblings_are_not_grouped():
    """A grouped launch writes one partial per tile, while a streaming plan reports one per streaming block: two sibling convs
    on the streaming kernel must go out as two launches.  Tiled siblings of one plan still group."""
    for m, c in ((16384, 128), (20480, 128), (50176, 64), (50176, 256)):
        assert not ops.igemm_groupable((1, 1, 1, m, 64), (1, 1, 1, 64, c), (1, 1, 1)), (m, c)
    assert ops.igemm_groupable((2, 8, 28, 28, 64), (1, 3, 3, 64, 64), (1, 1, 1))
