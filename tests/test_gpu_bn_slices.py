"""The BatchNorm passes on channel slices of wider rows (p3d_debug_bn_pass with row strides and column offsets).  The network
normalises conv outputs at their own row stride and writes z into channel views of the decoder's concat buffers, so every
kernel of a pass -- bn_small.hip forward and backward, bn_fold_apply_kernel, bn_apply_kernel, the stand-in statistics and the
three backward kernels -- indexes with up to six row strides (y1, y2, z, dz, dy1, dy2).  A kernel that used C where a stride
belongs, or that wrote past its slice, would pass every dense case.

Every case IS test_gpu_bn.bn_pass_case -- its inputs, its float64 oracle, its tolerances and its run-to-run bit equality,
unchanged: for the duration of a case ops.bn_pass is replaced by a function that embeds the dense operands in wide buffers,
runs the hook on the slices and hands the slices' contents back.  On top of that, per call of the hook:
  * everything outside a slice is filled with a NaN of a recognisable payload, then with 3.25 (conv_launch_ref.nan_fill, as
    test_gpu_conv_launch.py does): in z, dy1 and dy2 it must be bit-identical afterwards;
  * that fill, lying between the rows of y1, y2 and dz, must not reach any result: no NaN comes out, and the results of the two
    fills are equal bit for bit (moving statistics and parameter gradients included);
  * the outputs start from NaN inside their slices too (dy2: the gradient to add to when acc2), and no NaN may remain there.

Shapes: paths 1 (M = 130, 1024) and 3 (M = 130, 1025) at C = 8, 64, 72, 256, and path 2 at (1024, 64) and (2048, 256); every mode
with acc2 off and on, batch and moving statistics.  Slice forms as test_gpu_conv_launch.slice_forms: ld in {C, C + 4, 2C + 12}
with offset in {0, 4, ld - C}; the three operands vary independently over TRIPLES (every form of each operand at least once, one
triple with ld1, ld2 and ldz all different), and the triples rotate against (mode, acc2, statistics) over the shapes so that
each meets several of the other."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conv_launch_ref as ref              # noqa: E402
from test_gpu_bn import bn_pass_case          # noqa: E402

gpu = pytest.mark.gpu          # (the two table checks below need no device)

FILLS = [ref.nan_fill(), np.float32(3.25)]


def slice_forms(C):
    """(ld, offset) of a C-channel slice: (C, 0), (C + 4, 0), (C + 4, 4), (2C + 12, 0), (2C + 12, 4), (2C + 12, C + 12)."""
    return [(ld, off) for ld in (C, C + 4, 2 * C + 12) for off in sorted({0, 4, ld - C}) if off + C <= ld]


# indices into slice_forms for (y1 / dy1, y2 / dy2, z / dz): each operand takes each of the six forms at least once
TRIPLES = [(0, 1, 3), (1, 3, 2), (2, 5, 1), (3, 1, 0), (4, 3, 5), (5, 5, 4), (0, 0, 5), (5, 0, 0), (1, 2, 0), (3, 4, 2)]


def test_triples_cover_every_form():
    for k in range(3):
        assert {t[k] for t in TRIPLES} == set(range(6))
    f = slice_forms(64)
    assert len(f) == 6 and len({f[i][0] for i in TRIPLES[0]}) == 3          # ld1, ld2 and ldz all different
    assert all(ld % 4 == 0 and off % 4 == 0 for C in (8, 64, 72, 256) for ld, off in slice_forms(C))


class Sliced:
    """ops.bn_pass on dense operands, run on slices (see the module docstring); counts the hook calls it made."""
    def __init__(self, real, forms):
        self.real, self.forms, self.calls = real, forms, 0

    def __call__(self, mode, y1, y2, params, moving, dz, batch=(1, 1), update_moving=1, acc2=None, path=0):
        M, C = y1.shape
        f1, f2, fz = self.forms
        nan = np.full((M, C), np.nan, np.float32)
        results = []
        for fill in FILLS:
            def emb(a, form):
                out = np.full((M, form[0]), fill, np.float32)
                out[:, form[1]:form[1] + C] = a
                return out

            def split(buf, form, what):
                inside = np.ascontiguousarray(buf[:, form[1]:form[1] + C])
                outside = np.delete(buf, np.s_[form[1]:form[1] + C], 1)
                assert ref.same_bits(outside, np.full(outside.shape, fill, np.float32)), (what, "floats outside the slice changed")
                assert not np.isnan(inside).any(), (what, "NaN inside the slice", int(np.isnan(inside).sum()))
                return inside
            has2 = mode != 0
            out = self.real(mode, emb(y1, f1), emb(y2, f2) if has2 else None, params, moving, emb(dz, fz), batch=batch,
                            update_moving=update_moving, acc2=acc2, path=path, C_=C, offset=(f1[1], f2[1], fz[1]),
                            z=emb(nan, fz), dy1=emb(nan, f1), dy2=emb(acc2 if acc2 is not None else nan, f2) if has2 else None)
            self.calls += 1
            z, g1 = split(out[0], fz, "z"), split(out[1], f1, "dy1")
            g2 = split(out[2], f2, "dy2") if has2 else None
            assert not np.isnan(out[3]).any() and not np.isnan(out[4]).any()
            results.append((z, g1, g2, out[3], out[4], out[5]))
        for a, b in zip(results[0][:5], results[1][:5]):                  # what lies between the rows reaches no result
            assert (a is None and b is None) or ref.same_bits(a, b)
        assert results[0][5] == results[1][5]
        return results[0]


def sliced_case(monkeypatch, mode, M, C, path, batch, acc2, triple):
    from sap3d_tensorflow_amd import ops
    forms = slice_forms(C)
    hook = Sliced(ops.bn_pass, tuple(forms[i] for i in triple))
    monkeypatch.setattr(ops, "bn_pass", hook)
    info = bn_pass_case(mode, M, C, path, batch=(batch, batch), acc2=acc2)
    assert hook.calls == 4                                                # bn_pass_case ran twice, each on both fills
    assert info[0] == path
    return info


SHAPES = ([(M, C, 1) for M in (130, 1024) for C in (8, 64, 72, 256)] + [(M, C, 3) for M in (130, 1025) for C in (8, 64, 72, 256)] +
          [(1024, 64, 2), (2048, 256, 2)])
COMBOS = [(m, a, b) for b in (1, 0) for (m, a) in [(0, False)] + [(m, a) for m in (1, 2, 3, 4) for a in (False, True)]]
CASES = [(M, C, path, mode, acc2, batch, TRIPLES[(7 * i + j) % len(TRIPLES)])
         for i, (M, C, path) in enumerate(SHAPES) for j, (mode, acc2, batch) in enumerate(COMBOS)]


def test_case_table():
    """Every (mode, acc2, statistics) meets every triple, and every shape meets every triple."""
    assert len(CASES) == 18 * 18
    for key in (lambda c: c[3:6], lambda c: c[:3]):
        seen = {}
        for c in CASES:
            seen.setdefault(key(c), set()).add(c[6])
        assert all(len(v) == len(TRIPLES) for v in seen.values())


@gpu
@pytest.mark.parametrize("M,C,path,mode,acc2,batch,triple", CASES)
def test_bn_pass_on_slices(monkeypatch, M, C, path, mode, acc2, batch, triple):
    sliced_case(monkeypatch, mode, M, C, path, batch, acc2, triple)


@gpu
@pytest.mark.parametrize("bad", [dict(C_=64, offset=(0, 0, 0), ld=(66, 64, 64)), dict(C_=64, offset=(2, 0, 0), ld=(68, 64, 64)),
                                 dict(C_=64, offset=(8, 0, 0), ld=(68, 64, 64)), dict(C_=64, offset=(0, 0, 8), ld=(64, 64, 68)),
                                 dict(C_=64, offset=(0, 4, 0), ld=(64, 64, 64))])
def test_bad_slices_are_refused(bad):
    """Strides and offsets that are no multiples of 4, or a slice that does not fit its row, are an error."""
    from sap3d_tensorflow_amd import ops, P3dError
    M, C = 16, bad["C_"]
    wide = [np.ones((M, ld), np.float32) for ld in bad["ld"]]
    outs = dict(z=np.full((M, bad["ld"][2]), 7.5, np.float32), dy1=np.full((M, bad["ld"][0]), 7.5, np.float32),
                dy2=np.full((M, bad["ld"][1]), 7.5, np.float32))
    params, moving = np.ones((1, 2, C), np.float32), np.ones((1, 2, C), np.float32)
    with pytest.raises(P3dError, match="multiples of 4"):
        ops.bn_pass(1, wide[0], wide[1], params, moving, wide[2], C_=C, offset=bad["offset"], **outs)
