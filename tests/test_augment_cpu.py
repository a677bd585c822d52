"""No-GPU checks of the clip augmentation (P3DSession.set_augment): the numpy replay tests/augment_ref.py against the laws it
restates (oracle.dataflow.resize_linear, fixations_to_grid), its identities, the pinned draws of tests/golden/augment_draws.json,
the host-only draw hook of the library, the header's declarations and the Python front ends."""
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))      # (run as a script to write the fixture: no conftest.py has done it)
from oracle.dataflow import resize_linear      # noqa: E402
import augment_ref as ar                        # noqa: E402

ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "augment_draws.json")
f32 = np.float32
SHAPE = (2, 3, 5, 7)
CFG_KEYS = ("flip", "reverse", "min_scale", "contrast", "brightness")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _u32(v):
    return int(np.array([v], f32).view(np.uint32)[0])


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _row(flip=False, reverse=False, y0=0, x0=0, ch=None, cw=None, a=1.0, b=0.0, shape=SHAPE):
    return (flip, reverse, y0, x0, shape[2] if ch is None else ch, shape[3] if cw is None else cw, f32(a), f32(b))


def fixture_cases():
    """The (seed, g, H, W, settings) sweep of the fixture: tiny min_scale, H = 1, W = 1, large g, every seed bit set, the seed
    that cancels the xor, and seeds whose position draws are the closest to 1 of the first 20000."""
    near = [max(range(20000), key=lambda s: ar.uniform(s, 0, j)) for j in (3, 4)]
    seeds = [0, 1, 12345, 0xA5A5A5A5A5A5A5A5, (1 << 64) - 1] + near
    grids = [(1, 1), (1, 7), (5, 1), (5, 7), (16, 16), (112, 112), (224, 160)]
    cfgs = [dict(flip=0.5, reverse=0.5, min_scale=0.8, contrast=0.2, brightness=0.1),
            dict(flip=1.0, reverse=0.0, min_scale=1e-6, contrast=0.999, brightness=10.0),
            dict(flip=0.0, reverse=1.0, min_scale=0.5, contrast=0.0, brightness=0.0),
            dict(flip=0.3, reverse=0.7, min_scale=1.0, contrast=0.5, brightness=0.0)]
    out = []
    for i, seed in enumerate(seeds):
        for k, (H, W) in enumerate(grids):
            for g in (0, 1, 7 + i, (1 << 40) + k):
                out.append((seed, g, H, W, cfgs[(i + k + g) % len(cfgs)]))
    return out


def make_fixture():
    rows = []
    for seed, g, H, W, cfg in fixture_cases():
        d = ar.draw(seed, g, H, W, **cfg)
        rows.append(dict(seed=seed, g=g, H=H, W=W, cfg=[cfg[k] for k in CFG_KEYS],
                         decision=[int(d[0]), int(d[1]), d[2], d[3], d[4], d[5], _u32(d[6]), _u32(d[7])]))
    with open(FIXTURE, "w") as f:
        json.dump(rows, f, separators=(",", ":"))
        f.write("\n")


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def _decision_ints(d):
    return [int(d[0]), int(d[1]), int(d[2]), int(d[3]), int(d[4]), int(d[5]), _u32(d[6]), _u32(d[7])]


# ---- the transform -----------------------------------------------------------------------------------------------------------
def test_flipping_twice_and_reversing_twice_are_the_identity():
    x, y, fix = ar.random_clip(1, SHAPE, specials=True)
    for row in (_row(flip=True), _row(reverse=True), _row(flip=True, reverse=True)):
        once = ar.batch(x, y, fix, [row] * SHAPE[0])
        assert not _same(once[0], x) and not _same(once[1], y) and not np.array_equal(once[2], fix)
        twice = ar.batch(*once, [row] * SHAPE[0])
        assert _same(twice[0], x) and _same(twice[1], y) and np.array_equal(twice[2], fix)
    fl = ar.batch(x, y, fix, [_row(flip=True)] * 2)
    assert _same(fl[0], x[:, :, :, ::-1]) and _same(fl[1], y[:, :, :, ::-1]) and np.array_equal(fl[2], fix[:, :, :, ::-1])
    rv = ar.batch(x, y, fix, [_row(reverse=True)] * 2)
    assert _same(rv[0], x[:, ::-1]) and _same(rv[1], y[:, ::-1]) and np.array_equal(rv[2], fix[:, ::-1])


def test_neutral_decisions_return_the_input_bits():
    x, y, fix = ar.random_clip(2, SHAPE, specials=True)
    assert np.isnan(x).any() and np.isinf(x).any() and (_bits(x) == 0x80000000).any() and (_bits(x) == 0xffc12345).any()
    xo, yo, fo = ar.batch(x, y, fix, [_row()] * 2)
    assert _same(xo, x) and _same(yo, y) and np.array_equal(fo, fix)
    assert (fo == 200).any()                                 # the full window copies the bytes, it does not binarise them
    assert ar.batch(x, y, None, [_row()] * 2)[2] is None


def test_crop_is_the_oracle_resize_of_the_slice():
    x, y, _ = ar.random_clip(3, SHAPE)
    row = _row(y0=1, x0=2, ch=3, cw=4)
    xo, yo, _ = ar.batch(x, y, None, [row] * 2)
    for b in range(2):
        for t in range(SHAPE[1]):
            assert _same(yo[b, t], resize_linear(y[b, t, 1:4, 2:6], 5, 7))
            for c in range(3):                               # each channel on its own
                assert _same(xo[b, t, :, :, c], resize_linear(x[b, t, 1:4, 2:6, c], 5, 7))
    # one axis full: that axis keeps its samples (weight 0 on the second tap)
    xo, _, _ = ar.batch(x, y, None, [_row(x0=1, cw=5)] * 2)
    assert _same(xo[0, 0, :, :, 1], resize_linear(x[0, 0, :, 1:6, 1], 5, 7))


def test_photometric_is_two_rounded_float32_operations():
    x, y, _ = ar.random_clip(4, SHAPE)
    a, b = f32(1.3), f32(-0.2)
    xo, yo, _ = ar.batch(x, y, None, [_row(a=a, b=b)] * 2)
    assert _same(xo, ((x * a).astype(f32) + b).astype(f32)) and _same(yo, y)
    fused = (x.astype(np.float64) * float(a) + float(b)).astype(f32)
    assert not _same(xo, fused)                              # (a fused multiply-add would round once)


def test_fixations_follow_the_grid_law_and_never_grow():
    from sap3d_tensorflow_amd.dataflow import fixations_to_grid
    rng = np.random.default_rng(5)
    shape = (1, 2, 9, 11)
    x, y, fix = ar.random_clip(5, shape)
    for _ in range(40):
        ch, cw = int(rng.integers(1, 10)), int(rng.integers(1, 12))
        y0, x0 = int(rng.integers(0, 9 - ch + 1)), int(rng.integers(0, 11 - cw + 1))
        row = _row(y0=y0, x0=x0, ch=ch, cw=cw, shape=shape)
        fo = ar.batch(x, y, fix, [row])[2]
        window = fix[0, :, y0:y0 + ch, x0:x0 + cw]
        if (ch, cw) != (9, 11):
            assert np.array_equal(fo[0], fixations_to_grid(np.ascontiguousarray(window), 9, 11))
            assert set(np.unique(fo)) <= {0, 255}
        assert (fo >= 128).sum() <= (window >= 128).sum() and ((fo >= 128).sum() > 0) == ((window >= 128).sum() > 0)
        assert (fo >= 128).sum() == (window >= 128).sum()   # ch <= H, cw <= W: distinct window cells reach distinct grid cells


# ---- the draws -----------------------------------------------------------------------------------------------------------------
def test_splitmix_finaliser():
    # SplitMix64 (Steele, Lea, Flood 2014) seeded with 0 returns 0xE220A8397B1DCDAF first: state 0 + golden, finalised.  Draw j = 0
    # of clip 0 under the seed that cancels the xor is that state.
    z = 0xE220A8397B1DCDAF
    assert ar.uniform(0xA5A5A5A5A5A5A5A5, 0, 0) == (z >> 11) * 2.0 ** -53
    us = [ar.uniform(9, g, j) for g in range(50) for j in range(7)]
    assert len(set(us)) == len(us) and all(0.0 <= u < 1.0 for u in us)
    assert abs(np.mean(us) - 0.5) < 0.1


def test_decisions_stay_within_bounds(monkeypatch):
    for seed, g, H, W, cfg in fixture_cases():
        fl, rv, y0, x0, ch, cw, a, b = ar.draw(seed, g, H, W, **cfg)
        assert 1 <= ch <= H and 1 <= cw <= W and 0 <= y0 and y0 + ch <= H and 0 <= x0 and x0 + cw <= W
        lo = float(f32(cfg["min_scale"]))
        assert ch >= min(H, max(1, int(np.floor(lo * H + 0.5)))) and cw >= min(W, max(1, int(np.floor(lo * W + 0.5))))
        assert abs(float(a) - 1.0) <= float(f32(cfg["contrast"])) * (1 + 2.0 ** -23) and abs(float(b)) <= float(f32(cfg["brightness"]))
        assert a.dtype == f32 and b.dtype == f32 and a > 0
    # the ends of u, on every draw at once
    for u in (0.0, 1.0 - 2.0 ** -53, 0.5):
        monkeypatch.setattr(ar, "uniform", lambda seed, g, j, u=u: u)
        for H, W in [(1, 1), (1, 9), (7, 1), (112, 112), (3, 32768)]:
            for ms in (1e-6, 0.3, 1.0):
                fl, rv, y0, x0, ch, cw, a, b = ar.draw(0, 0, H, W, flip=0.5, reverse=1.0, min_scale=ms, contrast=0.999, brightness=2.0)
                assert 1 <= ch <= H and 1 <= cw <= W and 0 <= y0 <= H - ch and 0 <= x0 <= W - cw, (u, H, W, ms)
                assert a > 0 and rv == (u < 1.0) and fl == (u < 0.5)
                if u == 0.0:
                    assert (ch, cw, y0, x0) == (H, W, 0, 0)
                elif u > 0.9:
                    assert (y0, x0) == (H - ch, W - cw)


def test_pinned_draws():
    rows = load_fixture()
    cases = fixture_cases()
    assert len(rows) == len(cases) >= 100
    hit = dict(flip=0, reverse=0, crop=0, corner=0)
    for row, (seed, g, H, W, cfg) in zip(rows, cases):
        assert (row["seed"], row["g"], row["H"], row["W"], row["cfg"]) == (seed, g, H, W, [cfg[k] for k in CFG_KEYS])
        d = ar.draw(seed, g, H, W, **cfg)
        assert _decision_ints(d) == row["decision"], row
        hit["flip"] += d[0]; hit["reverse"] += d[1]; hit["crop"] += (d[4], d[5]) != (H, W)
        hit["corner"] += (d[4], d[5]) != (H, W) and H > 1 and d[2] + d[4] == H
    assert all(hit.values()), hit


def test_library_draws_are_the_replay():
    """p3d_debug_augment_draw is host only: no device is touched."""
    from sap3d_tensorflow_amd import ops, P3dError
    for row in load_fixture():
        cfg = dict(zip(CFG_KEYS, row["cfg"]))
        assert _decision_ints(ops.augment_draw(row["seed"], row["g"], row["H"], row["W"], **cfg)) == row["decision"], row
    for bad in (dict(flip=1.5), dict(reverse=-0.1), dict(min_scale=0.0), dict(min_scale=1.1), dict(contrast=1.0), dict(brightness=-1.0),
                dict(flip=float("nan")), dict(brightness=float("inf"))):
        with pytest.raises(P3dError):
            ops.augment_draw(0, 0, 4, 4, **bad)
    with pytest.raises(P3dError):
        ops.augment_draw(0, 0, 0, 4)


# ---- the boundary ----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_augmentation_symbols():
    from sap3d_tensorflow_amd import _lib
    src = open(os.path.join(ROOT, "include", "p3d_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(p3d_[a-z0-9_]+)\s*\(", code))
    want = {"p3d_set_augment", "p3d_get_augment", "p3d_augment_inputs", "p3d_last_augment", "p3d_last_augment_ms", "p3d_debug_augment",
            "p3d_debug_augment_draw"}
    assert want <= names
    assert re.search(r"typedef struct p3d_augment \{ float p_flip, p_reverse, min_scale, contrast, brightness; \} p3d_augment;", code)
    lib = _lib.lib()
    for n in want:
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert [f[0] for f in _lib.P3dAugment._fields_] == ["p_flip", "p_reverse", "min_scale", "contrast", "brightness"]
    assert "augment.hip" in open(os.path.join(ROOT, "sap3d_tensorflow_amd", "build.py")).read()


def test_driver_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_driver", os.path.join(ROOT, "drivers", "train.py"))
    tr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tr)
    old = sys.argv
    try:
        sys.argv = ["train.py"]
        a = tr.get_arguments()
        assert (a.aug_flip, a.aug_reverse, a.aug_min_scale, a.aug_contrast, a.aug_brightness) == (0.0, 0.0, 1.0, 0.0, 0.0)
        assert tr.augment_settings(a) is None
        sys.argv = ["train.py", "--aug-flip", "0.5", "--aug-min-scale", "0.8"]
        assert tr.augment_settings(tr.get_arguments()) == dict(flip=0.5, reverse=0.0, min_scale=0.8, contrast=0.0, brightness=0.0)
    finally:
        sys.argv = old
    src = open(os.path.join(ROOT, "drivers", "train.py")).read()
    for flag in ("--aug-flip", "--aug-reverse", "--aug-min-scale", "--aug-contrast", "--aug-brightness"):
        assert re.search(re.escape('"%s"' % flag) + r"[^\n]*\n?[^\n]*\[addition", src), flag


if __name__ == "__main__":
    make_fixture()
    print(FIXTURE, len(load_fixture()), "cases")
