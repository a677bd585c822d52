"""No-GPU checks of histogram matching: the replay of include/p3d_hip.h's law (tests/hist_match_ref.py) against numpy's own
np.histogram and np.interp, bit for bit; the host-side refusals of the C ABI, which come before any device is looked for; the
drivers' flags and table files."""
import ctypes as C
import importlib.util
import os
import zlib

import numpy as np
import pytest

import hist_match_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 7), (37, 53), (130, 257)]


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else a.dtype),
                                                                         b.view(np.uint64 if b.dtype == np.float64 else b.dtype))


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("nb", [256, 7])
@pytest.mark.parametrize("kind", ref.KINDS + ("three",))
def test_replay_is_numpy_histogram_and_interp_bit_for_bit(shape, nb, kind):
    rng = np.random.default_rng(zlib.crc32(repr((shape, nb, kind)).encode()))
    a = ref.values(kind, shape, rng)
    cdf, centre, count = ref.cumulative_distribution(a, nb)
    hist, edge = np.histogram(a.astype(np.float64), nb)
    assert np.array_equal(count, hist) and count.sum() == a.size
    assert _same_bits(ref.edges(a.min(), a.max(), nb)[2], edge)
    assert _same_bits(centre, (edge[:-1] + edge[1:]) / 2.0)
    assert _same_bits(cdf, np.cumsum(hist) / float(a.size))          # skimage: img_cdf = hist.cumsum(); img_cdf / img_cdf[-1]
    for tkind in ("three", "normal", "skewed"):
        tc, tx, _ = ref.cumulative_distribution(ref.values(tkind, shape, rng), nb)
        new = ref.interp(cdf, tc, tx)
        assert _same_bits(new, np.interp(cdf, tc, tx))
        v = a.astype(np.float64)
        assert _same_bits(ref.interp(v, centre, new), np.interp(v, centre, new))
        out = ref.match_hist(a, tc, tx, nb)
        assert out.dtype == np.float32 and _same_bits(out, np.interp(v, centre, new).astype(np.float32))


def test_edge_valued_maps_take_both_fix_ups():
    """The float32 neighbours of the bin edges: (int)((v - mn) * norm) lands a bin off on either side there, and on the top edge."""
    hit = set()
    for seed, nb in ref.EDGE_CASES:
        v = ref.edge_values(seed, nb).astype(np.float64).ravel()
        mn, mx, edge, norm = ref.edges(v.min(), v.max(), nb)
        i = ((v - mn) * norm).astype(np.int64)
        hit |= {"top"} if np.any(i == nb) else set()
        i[i == nb] = nb - 1
        hit |= {"dec"} if np.any(v < edge[i]) else set()
        hit |= {"inc"} if np.any((v >= edge[i + 1]) & (i != nb - 1)) else set()
        hist, e = np.histogram(v, nb)
        assert np.array_equal(ref.cumulative_distribution(v, nb)[2], hist) and _same_bits(e, edge)
    assert hit == {"top", "dec", "inc"}, hit


def test_const_map_follows_the_half_rule():
    a = ref.values("const", (5, 7), None)
    mn, mx, edge, norm = ref.edges(a.min(), a.max(), 7)
    assert mn == np.float64(np.float32(0.37)) - 0.5 and mx == np.float64(np.float32(0.37)) + 0.5 and norm == 7.0
    cdf, centre, count = ref.cumulative_distribution(a, 7)
    assert count.tolist() == [0, 0, 0, 35, 0, 0, 0] and cdf.tolist() == [0, 0, 0, 1, 1, 1, 1]
    assert np.array_equal(count, np.histogram(a.astype(np.float64), 7)[0])
    # matched to any table, a constant map stays constant
    tc, tx, _ = ref.cumulative_distribution(ref.values("uniform", (5, 7), np.random.default_rng(0)), 7)
    assert len(np.unique(ref.match_hist(a, tc, tx, 7))) == 1


def _abi():
    from sap3d_tensorflow_amd import _lib
    return _lib, _lib.lib()


def test_host_side_refusals_come_before_the_device_and_change_nothing():
    _lib, lib = _abi()
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    m = np.arange(35, dtype=np.float32).reshape(1, 5, 7)
    out = np.full_like(m, -7.0)
    cdf, centre = np.empty((1, 8)), np.empty((1, 8))
    good_c, good_x = np.linspace(0.1, 1.0, 8), np.linspace(0.0, 1.0, 8)

    def err():
        return lib.p3d_last_error().decode()

    for nb in (1, 0, -3, 1025):
        assert lib.p3d_cumulative_distribution(0, m.ctypes.data_as(fp), 1, 5, 7, nb, None, cdf.ctypes.data_as(dp), centre.ctypes.data_as(dp)) == -1
        assert "nbins" in err()
        assert lib.p3d_match_hist(0, m.ctypes.data_as(fp), 1, 5, 7, nb, good_c.ctypes.data_as(dp), good_x.ctypes.data_as(dp), 1, 8, out.ctypes.data_as(fp)) == -1
        assert "nbins" in err()
        assert lib.p3d_match_hist_maps(0, m.ctypes.data_as(fp), m.ctypes.data_as(fp), 1, 5, 7, nb, out.ctypes.data_as(fp)) == -1
        assert "nbins" in err()

    def match(c, x, nt, n_tables=1):
        c, x = np.ascontiguousarray(c, np.float64), np.ascontiguousarray(x, np.float64)
        return lib.p3d_match_hist(0, m.ctypes.data_as(fp), 1, 5, 7, 256, c.ctypes.data_as(dp), x.ctypes.data_as(dp), n_tables, nt, out.ctypes.data_as(fp))

    assert match(good_c, good_x, 1) == -1 and "nt" in err()
    assert match(np.linspace(0, 1, 1025), np.linspace(0, 1, 1025), 1025) == -1 and "nt" in err()
    for bad in (np.nan, np.inf, -np.inf):
        c = good_c.copy()
        c[3] = bad
        assert match(c, good_x, 8) == -1 and "finite" in err()
        assert match(good_c, c, 8) == -1 and "finite" in err()
    c = good_c.copy()
    c[4] = c[3] - 1e-9
    assert match(c, good_x, 8) == -1 and "non-decreasing" in err()
    assert match(good_c, c, 8) == -1 and "non-decreasing" in err()
    assert match(good_c, good_x, 8, n_tables=2) == -1 and "table" in err()
    assert lib.p3d_match_hist(0, m.ctypes.data_as(fp), 1, 5, 7, 256, None, None, 1, 8, out.ctypes.data_as(fp)) == -1 and "table" in err()
    assert np.all(out == -7.0)
    # the chain's entry point parses its setting first as well: an unknown mode, NULL tables under TABLE, DENSITY outside evaluation
    post = _lib.P3dPostprocess(0.0, 0, 0)
    for cfg, word in ((_lib.P3dHistMatch(7, 256, 0, None, None), "mode"), (_lib.P3dHistMatch(1, 256, 8, None, None), "table"),
                      (_lib.P3dHistMatch(1, 1, 8, good_c.ctypes.data_as(dp), good_x.ctypes.data_as(dp)), "nbins"),
                      (_lib.P3dHistMatch(2, 256, 0, None, None), "evaluation")):
        assert lib.p3d_postprocess_maps_match(0, m.ctypes.data_as(fp), 1, 5, 7, 1, 5, 7, C.byref(post), C.byref(cfg), 0.0,
                                              out.ctypes.data_as(fp), None) == -1
        assert word in err(), (word, err())
    assert np.all(out == -7.0)
    assert lib.p3d_set_hist_match(None, None) == -1 and lib.p3d_get_hist_match(None, None) == -1


def test_python_wrappers_refuse_malformed_arguments():
    from sap3d_tensorflow_amd import dataflow as gdf
    m = np.zeros((2, 5, 7), np.float32)
    with pytest.raises(ValueError):
        gdf.cumulative_distribution(m, nbins=1)
    with pytest.raises(ValueError):
        gdf.match_hist(m, np.zeros(8), np.zeros(9))
    with pytest.raises(ValueError):
        gdf.match_hist(m, np.zeros((3, 8)), np.zeros((3, 8)))
    with pytest.raises(ValueError):
        gdf.match_hist_maps(m, m[:1])
    with pytest.raises(ValueError):
        gdf._match_cfg("sum")
    cfg, keep = gdf._match_cfg((np.linspace(0, 1, 8), np.linspace(0, 1, 8)), 64)
    assert (cfg.mode, cfg.nbins, cfg.nt) == (1, 64, 8) and cfg.cdf[7] == 1.0
    assert gdf._match_cfg("density", 7)[0].mode == 2 and gdf._match_cfg(None)[0].mode == 0 and gdf._match_cfg("off")[0].mode == 0


def _driver(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "drivers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_flags_and_table_files(tmp_path):
    from sap3d_tensorflow_amd import dataflow as gdf
    cdf, centres = np.linspace(0.01, 1.0, 16), np.linspace(0.0, 0.9, 16)
    table = str(tmp_path / "table.npz")
    np.savez(table, cdf=cdf, bin_centers=centres)
    got = gdf.load_match_table(table)
    assert got[0].dtype == np.float64 and np.array_equal(got[0], cdf) and np.array_equal(got[1], centres)
    np.savez(str(tmp_path / "bad.npz"), cdf=cdf)
    with pytest.raises(ValueError):
        gdf.load_match_table(str(tmp_path / "bad.npz"))
    np.savez(str(tmp_path / "ragged.npz"), cdf=cdf, bin_centers=centres[:5])
    with pytest.raises(ValueError):
        gdf.load_match_table(str(tmp_path / "ragged.npz"))

    tp = _driver("test")
    a = tp.parse_args([])
    assert a.match_hist == "" and a.match_bins == 256 and tp.match_target(a) == "off"
    a = tp.parse_args(["--match-hist", "density", "--match-bins", "64"])
    assert tp.match_target(a) == "density" and a.match_bins == 64
    a = tp.parse_args(["--match-hist", table])
    t = tp.match_target(a)
    assert np.array_equal(t[0], cdf) and np.array_equal(t[1], centres)
    for bins in ("1", "1025"):
        with pytest.raises(SystemExit) as e:
            tp.parse_args(["--match-bins", bins])
        assert e.value.code != 0

    gp = _driver("gen_pred")
    a = gp.parse_args(["--videos", "v", "--write", "png", "--match-hist", table, "--match-bins", "32", "--resident"])
    assert a.match_bins == 32 and a.resident and np.array_equal(gp.match_target(a)[0], cdf)
    assert gp.match_target(gp.parse_args(["--videos", "v"])) == "off"
    for argv in (["--videos", "v", "--write", "npy", "--match-hist", table], ["--videos", "v", "--write", "png", "--match-hist", "density"],
                 ["--videos", "v", "--write", "png", "--match-bins", "1"]):
        with pytest.raises(SystemExit) as e:
            gp.parse_args(argv)
        assert e.value.code != 0


def test_declared_symbols_are_exported_and_bound():
    _lib, lib = _abi()
    for name in ("p3d_cumulative_distribution", "p3d_match_hist", "p3d_match_hist_maps", "p3d_set_hist_match", "p3d_get_hist_match",
                 "p3d_postprocess_maps_match", "p3d_debug_eval_maps_match"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "p3d_hip.h")).read()
    assert "#define P3D_HIST_MAX_BINS %d" % _lib.P3D_HIST_MAX_BINS in hdr
    assert "enum { P3D_MATCH_OFF = 0, P3D_MATCH_TABLE = 1, P3D_MATCH_DENSITY = 2 };" in hdr and _lib.MATCH_MODES == {"off": 0, "table": 1, "density": 2}
