"""The kernels of csrc/score_u8.hip through p3d_debug_score_u8 (every device buffer between guards) against tests/score_u8_ref.py:
the integer tables with tolerance 0; CC, NSS and AUC-Judd -- finals from exact integers -- to relative 1e-12; SIM and KL, whose
order over the pixels is the kernel's, to the project's 1e-9.  Shapes are the smallest at which each path can go wrong: under one
wave and under one 16-byte word (3 x 5), maps that start off a 16-byte boundary with the three sources aligned alike and unalike
(7 x 19 at four offsets), whole words (16 x 16), three blocks per map (263 x 251), and one pair at 1080 x 960."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import score_u8_ref as R        # noqa: E402

COLS = ("CC", "SIM", "AUC", "KL", "NSS")
exact_seen = {}


def run(sal, den, fix, flags=R.ALL, ties=R.EXPECTED, offset=0):
    from sap3d_tensorflow_amd import metrics
    return metrics.score_bytes(sal, den, fix, flags=flags, ties="reference" if ties == R.REFERENCE else "expected", with_tables=True,
                               offset=offset)


def check(sal, den, fix, flags=R.ALL, ties=R.EXPECTED, offset=0, what=""):
    got, tab = run(sal, den, fix, flags, ties, offset)
    n = len(sal)
    for i in range(n):
        t = R.tables(sal[i], den[i], None if fix is None else fix[i])
        for k in ("hs", "hf", "hd"):
            assert np.array_equal(tab[k][i], t[k]), (what, i, k)
        assert int(tab["sd"][i]) == t["sd"], (what, i)
    want = R.score_maps(sal, den, fix, flags, ties)
    assert got.shape == want.shape == (n, 5)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    worst = [max([R.rel(got[i, j], want[i, j]) for i in range(n) if not np.isnan(want[i, j])] or [0.0]) for j in range(5)]
    print(what, "offset", offset, "largest relative error", dict(zip(COLS, worst)))
    for j, gate in ((0, R.FINAL_GATE), (2, R.FINAL_GATE), (4, R.FINAL_GATE), (1, R.GPU_GATE), (3, R.GPU_GATE)):
        assert worst[j] <= gate, (what, COLS[j], worst[j])
    for j in (0, 2, 4):
        exact_seen[COLS[j]] = exact_seen.get(COLS[j], True) and worst[j] == 0.0
    return got


def test_under_one_wave_and_under_one_word():
    c = R.case(3, 5, 1)
    for ties in (R.REFERENCE, R.EXPECTED):
        check(c["sal"], c["den"], c["fix"], ties=ties, what="3x5")


@pytest.mark.parametrize("offset", [0, 1, 5, 15])
def test_maps_off_the_16_byte_boundary(offset):
    """7 x 19 = 133 bytes a map: map m starts 5 m bytes further past a boundary.  At offset 0 the three sources are aligned alike
    (whole words behind a head), at the others unalike (every pixel a byte load)."""
    c = R.case(7, 19, 5)
    for ties in (R.REFERENCE, R.EXPECTED):
        check(c["sal"], c["den"], c["fix"], ties=ties, offset=offset, what="7x19")


def test_whole_words():
    c = R.case(16, 16, 5)
    check(c["sal"], c["den"], c["fix"], what="16x16")
    check(c["sal"], c["den"], c["fix"], ties=R.REFERENCE, what="16x16")


@pytest.mark.parametrize("offset", [0, 3])
def test_three_blocks_per_map_flush_across_blocks(offset):
    from sap3d_tensorflow_amd import metrics
    assert metrics.score_plan(263 * 251, 5, offset)[0] >= 3
    c = R.case(263, 251, 5)
    check(c["sal"], c["den"], c["fix"], offset=offset, what="263x251")


@pytest.mark.parametrize("shape", [(7, 19), (263, 251)])
def test_contents_that_single_out_a_path(shape):
    """A constant map (all lanes in one bin, zero variance), arange % 256 (no two lanes of a wave share a bin), only 0 and 255, no
    fixation, every pixel fixated, fixation bytes 127 / 128 either side of the rule, all-zero maps (the ps / pd branch)."""
    c = R.edge_case(*shape)
    for ties in (R.REFERENCE, R.EXPECTED):
        got = check(c["sal"], c["den"], c["fix"], ties=ties, offset=0 if ties else 7, what="edge %dx%d" % shape)
        k = {n: i for i, n in enumerate(c["names"])}
        assert np.isnan(got[k["constant saliency"]][[0, 1, 4]]).all()
        assert np.isnan(got[k["no fixation"]][[2, 4]]).all()
        assert np.isnan(got[k["every pixel fixated"]][2]) and got[k["every pixel fixated"]][4] == 0.0


def test_full_size_pair_and_sums_beyond_32_bits():
    """One 1080 x 960 pair: an ordinary map, and all 255 against all 255 (S2 and the sum of products exceed 2^32)."""
    H, W = 1080, 960
    c = R.case(H, W, 1)
    full = np.full((1, H, W), 255, np.uint8)
    sal, den, fix = np.concatenate([c["sal"], full]), np.concatenate([c["den"], full]), np.concatenate([c["fix"], c["fix"]])
    got, tab = run(sal, den, fix)
    assert int(tab["sd"][1]) == 255 * 255 * H * W > 2 ** 32
    check(sal, den, fix, what="1080x960")
    assert np.isnan(got[1][[0, 1, 4]]).all() and got[1][2] == got[1][2]


@pytest.mark.parametrize("n", [1, 2, 17])
def test_map_counts_around_the_chunk_of_the_chain(n):
    c = R.case(7, 19, 5)
    idx = np.arange(n) % 5
    check(c["sal"][idx], c["den"][idx], c["fix"][idx], offset=n % 16, what="n=%d" % n)


def test_two_calls_in_a_row_give_equal_bits():
    c = R.case(263, 251, 5)
    a, ta = run(c["sal"], c["den"], c["fix"])
    b, tb = run(c["sal"], c["den"], c["fix"])
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert all(np.array_equal(ta[k], tb[k]) for k in ta)
    from sap3d_tensorflow_amd import metrics
    plain = metrics.score_bytes(c["sal"], c["den"], c["fix"])          # the op-level entry: the same launches, the same bits
    assert np.array_equal(plain.view(np.uint64), a.view(np.uint64))


def test_flags_select_columns_and_pass_b():
    """The .m file's masks leave KL and NSS NaN.  Pass B runs only for SIM or KL: without them the hook finds its buffers untouched
    (it returns -1 otherwise) and both columns are NaN; whatever is selected keeps the bits it has with everything on."""
    c = R.case(7, 19, 5)
    everything = check(c["sal"], c["den"], c["fix"], what="all")
    for flags in (R.MATLAB, R.CC | R.JUDD | R.NSS, R.SIM, R.KL, R.NSS, R.CC):
        got = check(c["sal"], c["den"], c["fix"], flags=flags, what="flags %d" % flags)
        for j, bit in enumerate((R.CC, R.SIM, R.JUDD, R.KL, R.NSS)):
            if flags & bit:
                assert np.array_equal(got[:, j].view(np.uint64), everything[:, j].view(np.uint64)), (flags, j)
            else:
                assert np.isnan(got[:, j]).all(), (flags, j)
    got = check(c["sal"], c["den"], None, flags=R.CC | R.SIM | R.KL, what="no fixation maps")
    assert np.array_equal(got[:, [0, 1, 3]].view(np.uint64), everything[:, [0, 1, 3]].view(np.uint64))


def test_refusals():
    from sap3d_tensorflow_amd import P3dError, metrics
    c = R.case(3, 5, 1)
    for kw in (dict(flags=0), dict(flags=32), dict(flags=-1)):
        with pytest.raises(P3dError, match="flags"):
            metrics.score_bytes(c["sal"], c["den"], c["fix"], **kw)
    with pytest.raises(P3dError, match="fixation"):
        metrics.score_bytes(c["sal"], c["den"], None, flags=("cc", "judd"))
    with pytest.raises(P3dError, match="offset"):
        metrics.score_bytes(c["sal"], c["den"], c["fix"], with_tables=True, offset=16)
    big = np.zeros((1, 2 ** 12, 2 ** 11 + 1), np.uint8)
    with pytest.raises(P3dError, match="2\\^23"):
        metrics.score_bytes(big, big, big)


def test_zz_report_bit_equality_of_the_finals():
    """Not a gate: says whether CC, NSS and AUC-Judd were bit-equal to the replay in every comparison of this module."""
    print("bit-equal to the replay in every comparison:", exact_seen)
