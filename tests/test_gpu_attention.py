"""Op-level parity of the self-attention block (attn_run in net_graphs.inc; attention.hip, attention_flash.hip) against the
float64 restatements of tests/attention_ref.py: the softmax rows forward and backward, the core in BOTH executions -- the
stored-score launch sequence of the graph op (AttnCore, p3d_debug_attention_core mode 1) and the kernels that keep the scores
on chip (mode 2) -- and the mixing with its dropout.

Tolerance, everywhere: within 5 x the float32 restatement's own distance from float64 on the same inputs + 2e-5 (1e-4 for dg
and df, whose ds = p (dp - <p, dp>) cancels), relative to the result's maximum magnitude (attention_ref.rule).  The score
regimes are established on the reference alone in tests/test_attention_ref_cpu.py.  Outputs, stored scores and scratch hold
NaNs before the launches (the hooks fill them), so a buffer the sequence forgets to zero or to write shows."""
import numpy as np
import pytest

import attention_ref as ar
import gates
from conv_launch_ref import nan_fill, same_bits

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
NAN = nan_fill()
GUARD = 2            # guard rows behind the last softmax row


def ops():
    from sap3d_tensorflow_amd import ops as o
    return o


# ---- softmax rows ---------------------------------------------------------------------------------------------------------------
COLS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 4095, 4096, 4097, 6000]      # wave per row | block per row | three passes
ROWS = [1, 3, 4, 5, 1021]


def wide(a, ld, guard=GUARD):
    """[rows, cols] -> [rows + guard, ld] float32, NaN (with a payload) outside."""
    out = np.full((a.shape[0] + guard, ld), NAN, f32)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def softmax_case(rows, cols, ld, rotate, seed):
    o = ops()
    rng = np.random.default_rng([seed, rows, cols, ld, rotate])
    s, _ = ar.softmax_input(rng, rows, cols, rotate)
    tag = "softmax %dx%d ld %d rot %d" % (rows, cols, ld, rotate)
    got = o.softmax_rows_launch(wide(s, ld), cols, guard_rows=GUARD)
    assert same_bits(got[rows:], wide(s, ld)[rows:]), "guard rows"
    assert np.all(got[:rows, cols:] == 0), "pad columns"
    want64, want32 = ar.softmax_rows(s), ar.softmax_rows(s, f32)
    ar.rule(got[:rows, :cols], want64, want32, what=tag + " fwd")
    ar.rule(got[:rows, :cols].sum(-1, dtype=f64), np.ones(rows), want32.sum(-1, dtype=f64), what=tag + " fwd row sums")
    assert same_bits(got, o.softmax_rows_launch(wide(s, ld), cols, guard_rows=GUARD))
    # backward, from the float32 map the forward would have left and a random gradient of it; pad columns of both hold NaNs
    beta = want64.astype(f32)
    d = rng.standard_normal((rows, cols)).astype(f32)
    gd = o.softmax_rows_launch(wide(beta, ld), cols, d=wide(d, ld), guard_rows=GUARD)
    assert same_bits(gd[rows:], wide(d, ld)[rows:]), "guard rows (backward)"
    assert np.all(gd[:rows, cols:] == 0), "pad columns (backward)"
    w64, w32 = ar.softmax_rows_bwd(beta, d), ar.softmax_rows_bwd(beta, d, f32)
    ar.rule(gd[:rows, :cols], w64, w32, what=tag + " bwd")
    scale = max(np.abs(w64).max(), 1e-30)
    ar.rule(gd[:rows, :cols].sum(-1, dtype=f64), np.zeros(rows), w32.sum(-1, dtype=f64), scale=scale, what=tag + " bwd row sums")
    assert same_bits(gd, o.softmax_rows_launch(wide(beta, ld), cols, d=wide(d, ld), guard_rows=GUARD))


@pytest.mark.parametrize("extra", [0, 4])
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_softmax_rows(rows, cols, extra):
    """Every launch shape (one wave per row with a ragged last group of 4 rows, one block per row, rows kept in registers up to
    4096 columns and re-read above) on rows of every value regime: row i is of regime (i + rotate) % 9, and row counts below 9
    are run at every rotation."""
    ld = (cols + 3) // 4 * 4 + extra
    for rotate in (range(9) if rows < 9 else (0,)):
        softmax_case(rows, cols, ld, rotate, 0)


@pytest.mark.parametrize("rows,cols", [(262145, 5), (65537, 257)])
def test_softmax_rows_grid_stride(rows, cols):
    """One row past what the capped grids cover in one sweep: 65535 blocks of 4 rows (wave per row), 65535 blocks (block per row)."""
    softmax_case(rows, cols, (cols + 3) // 4 * 4, 0, 1)


# ---- the core -------------------------------------------------------------------------------------------------------------------
NAMES = ("o", "dg", "df", "dh")
FLOORS = (ar.FLOOR, ar.FLOOR_DS, ar.FLOOR_DS, ar.FLOOR)


def run_core(mode, g, f, h, d):
    o = ops()
    fwd = o.attention_core_launch(mode, g, f, h)
    got = o.attention_core_launch(mode, g, f, h, d)
    assert same_bits(fwd, got[0]), "forward-only o"
    again = o.attention_core_launch(mode, g, f, h, d)
    assert all(same_bits(a, b) for a, b in zip(got, again)), "two calls"
    return got


def check_core(mode, key, got, want64, want32, scales):
    """The stored-score execution meets the rule.  So does the on-chip one, except where gates.py holds a figure measured on the
    MI355X for the case under attention_op/ (the fixed ceiling there is the path's 1e-3)."""
    excess = 0.0
    for name, a, w64, w32, floor, scale in zip(NAMES, got, want64, want32, FLOORS, scales):
        assert np.all(np.isfinite(a)), (mode, key, name)
        err, lim = ar.rel_err(a, w64, scale), ar.bound(w32, w64, floor, scale)
        print("core %s %s %s err %.3e bound %.3e" % (key, mode, name, err, lim))
        if mode == "stored":
            assert err <= lim, (key, name, err, lim)
        excess = max(excess, err - lim)
    if excess > 0:
        gates.check("attention_op/" + key, excess, margin=2.0, floor=0.0)
    return max(excess, 0.0)


def core_case(B, ng, nf, ch, regime, modes=("stored", "flash")):
    g, f, h, d = ar.core_input(regime, B, ng, nf, ch)
    want64, want32 = ar.core(g, f, h, d), ar.core(g, f, h, d, f32)
    key = "%dx%dx%dx%d-%s" % (B, ng, nf, ch, regime)
    scales = ar.core_scales(g, f, h, d)          # the results' maximum magnitudes (attention_ref.core_scales on a zero result)
    got, excess = {}, 0.0
    for mode in modes:
        got[mode] = run_core(mode, g, f, h, d)
        excess = max(excess, check_core(mode, key, got[mode], want64, want32, scales))
    if len(modes) == 2:       # the two executions agree within twice the rule (plus what the gate above granted the on-chip one)
        for name, a, b, w64, w32, floor, scale in zip(NAMES, got["stored"], got["flash"], want64, want32, FLOORS, scales):
            diff = ar.rel_err(a, b.astype(f64), scale)
            print("core %s stored-flash %s diff %.3e" % (key, name, diff))
            assert diff <= 2 * ar.bound(w32, w64, floor, scale) + excess, (key, name, diff)


@pytest.mark.parametrize("regime", ar.CORE_REGIMES)
@pytest.mark.parametrize("B,ng,nf,ch", ar.CORE_CASES)
def test_core_both_executions(B, ng, nf, ch, regime):
    core_case(B, ng, nf, ch, regime)


@pytest.mark.parametrize("regime", ar.CORE_REGIMES)
@pytest.mark.parametrize("B,ng,nf,ch", ar.STORED_ONLY_CASES)
def test_core_stored_scores_at_other_widths(B, ng, nf, ch, regime):
    """512 channels (x_4_0 at base 32) and 96: the on-chip kernels do not exist there and the GEMMs are the only execution."""
    core_case(B, ng, nf, ch, regime, modes=("stored",))


@pytest.mark.parametrize("B,ng,nf,ch", ar.STORED_ONLY_CASES)
def test_core_on_chip_refuses_other_widths(B, ng, nf, ch):
    from sap3d_tensorflow_amd import P3dError
    g, f, h, d = ar.core_input("units", B, ng, nf, ch)
    with pytest.raises(P3dError, match="32, 64, 128 or 256"):
        ops().attention_core_launch("flash", g, f, h, d)
    with pytest.raises(P3dError, match="32, 64, 128 or 256"):
        ops().attention_core(g, f, h)


def test_k_sliced_products():
    """Few queries over many keys: the plan cuts K of the beta h and ds f products (p3d_debug_attention_splits asks AttnCore, the
    description that launches them, for the plans: 8 slices each at this shape), and a forced slice count cuts g f^T and
    d_o h^T as well (p3d_debug_force_plan).  The sliced launches add to an output zeroed once, from NaN here."""
    from sap3d_tensorflow_amd._lib import lib
    o = ops()
    B, ng, nf, ch = 1, 8, 1024, 32
    assert (B, ng, nf, ch) in ar.CORE_CASES
    sp = o.attention_splits(B, ng, nf, ch)
    assert sp[1] > 1 and sp[3] > 1, sp
    assert o.attention_splits(2, 300, 77, 32) == (1, 1, 1, 1)
    assert o.attention_splits(1, 130, 4101, 32)[1] > 1          # the three-pass softmax case feeds a sliced product too
    B, ng, nf, ch = 2, 24, 264, 256
    lib().p3d_debug_force_plan(-1, 2, 0, 0)
    try:
        assert o.attention_splits(B, ng, nf, ch) == (1, 2, 2, 2)        # (g f^T has 32 channels to cut: one K step)
        for regime in ("units", "offset"):
            core_case(B, ng, nf, ch, regime, modes=("stored",))
    finally:
        lib().p3d_debug_force_plan(-1, 0, 0, 0)


# ---- the mixing -----------------------------------------------------------------------------------------------------------------
def mix_case(M, C, gamma, accx, drop, ld_extra=(0, 0, 0), offset=(0, 0, 0), seed=7, dgamma_prior=0.375, stats=False):
    o = ops()
    rng = np.random.default_rng([M % 9973, C, int(gamma * 10) + 20, accx, int(drop * 10)])
    r, x, dz, prior = (rng.standard_normal((M, C)).astype(f32) for _ in range(4))
    lds = [C + e for e in ld_extra]

    def emb(a, k):
        out = np.full((M, lds[k]), NAN, f32)
        out[:, offset[k]:offset[k] + C] = a
        return out

    def cut(buf, k):
        return buf[:, offset[k]:offset[k] + C]

    def guards_kept(buf, k):
        ref = np.full((M, lds[k]), NAN, f32)
        return same_bits(np.delete(buf, np.s_[offset[k]:offset[k] + C], 1), np.delete(ref, np.s_[offset[k]:offset[k] + C], 1))

    kw = dict(offset=offset, drop_rate=drop, seed=seed, accx=accx, dgamma=dgamma_prior)
    args = (emb(r, 0), emb(x, 1), gamma, C)
    bufs = dict(z=emb(np.full((M, C), NAN, f32), 2), dz=emb(dz, 2), dr=emb(np.full((M, C), NAN, f32), 0),
                dx=emb(prior if accx else np.full((M, C), NAN, f32), 1))
    zb, drb, dxb, dgm = o.attn_mix(*args, **bufs, **kw)
    assert same_bits(o.attn_mix(*args, z=bufs["z"], offset=offset, drop_rate=drop, seed=seed), zb), "forward-only z"
    for buf, k in ((zb, 2), (drb, 0), (dxb, 1)):
        assert guards_kept(buf, k), "guard columns"
    z, dr, dx = cut(zb, 2), cut(drb, 0), cut(dxb, 1)
    keep = None
    if drop > 0:
        # the seed in device memory gives the same bits as the seed as an argument
        other = o.attn_mix(*args, **bufs, **dict(kw, seed_dev=True))
        assert all(same_bits(a, b) for a, b in zip((zb, drb, dxb), other[:3])) and other[3] == dgm, "seed in device memory"
        base = ar.mix(r, x, gamma, dtype=f32)
        keep = np.where(base != 0, z != 0, True)
        dropped = (base != 0) & (z == 0)
        assert np.all(dr[dropped] == 0)
        assert np.all(dx[dropped] == (prior[dropped] if accx else 0))
        if stats:
            n = M * C
            share, sd = keep.mean(), (drop * (1 - drop) / n) ** 0.5
            assert abs(share - (1 - drop)) <= 4 * sd, (share, sd)
            z2 = cut(o.attn_mix(*args, z=bufs["z"], offset=offset, drop_rate=drop, seed=seed + 1), 2)
            assert 0.3 < ((z2 != 0) != (z != 0)).mean() < 0.7, "a second seed gives another mask"
    tag = "mix %dx%d gamma %g accx %d drop %g" % (M, C, gamma, accx, drop)
    ar.rule(z, ar.mix(r, x, gamma, keep, drop), ar.mix(r, x, gamma, keep, drop, f32), what=tag + " z")
    pr = prior if accx else None
    w64 = ar.mix_bwd(dz, r, gamma, keep, drop, pr, dgamma_prior)
    w32 = ar.mix_bwd(dz, r, gamma, keep, drop, pr, dgamma_prior, f32)
    ar.rule(dr, w64[0], w32[0], what=tag + " dr")
    ar.rule(dx, w64[1], w32[1], what=tag + " dx")
    ar.rule(np.array([dgm]), np.array([w64[2]]), np.array([w32[2]]), what=tag + " dgamma")      # (the prior is part of the result)


def cap_sizes(C):
    out = []
    for cap in (524288, 2097152):          # float4s one sweep of the capped grids covers: 2048 blocks backward, 8192 forward
        m0 = cap // (C // 4)
        out += [(m0 - 1, C), (m0, C), (m0 + 1, C)]
    return out


@pytest.mark.parametrize("M,C", [mc for C in (4, 32, 36, 512) for mc in cap_sizes(C)])
def test_mix_around_the_grid_caps(M, C):
    """Float4 counts below, at (where C / 4 divides it) and above what the capped grids cover in one sweep."""
    k = (M + C) % 2
    mix_case(M, C, -0.7, accx=k, drop=0.5 * (1 - k))


@pytest.mark.parametrize("drop", [0.0, 0.5])
@pytest.mark.parametrize("accx", [0, 1])
@pytest.mark.parametrize("gamma", [0.0, 1.0, -0.7])
@pytest.mark.parametrize("C", [4, 32, 36, 512])
def test_mix_slices(C, gamma, accx, drop):
    """r, x and z as channel slices of wider rows at non-zero offsets; everything outside keeps its NaN bits."""
    mix_case(777, C, gamma, accx, drop, ld_extra=(8, 12, 16), offset=(4, 8, 12))
    mix_case(3, C, gamma, accx, drop, ld_extra=(4, 0, 8), offset=(4, 0, 0), dgamma_prior=-2.5)


def test_mix_dropout_statistics():
    mix_case(65537, 32, 1.0, accx=0, drop=0.5, stats=True)
    mix_case(4099, 36, -0.7, accx=1, drop=0.5, ld_extra=(4, 4, 4), offset=(0, 4, 0), stats=True)
