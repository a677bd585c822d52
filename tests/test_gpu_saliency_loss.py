"""The per-map loss with NSS and SIM terms and a fixation map, P3D_LOSS_SALIENCY (map_loss.hip, the saliency_loss_* kernels):
w_kld KL + w_cc (1 - CC) + w_nss (-NSS) + w_sim (1 - SIM) per [H, W] map, at op level through p3d_debug_saliency_loss against
the float64 restatement in saliency_loss_ref.py, bit for bit against P3D_LOSS_KLD_CC when the new weights are 0, and in small
networks.  Every op-level call runs twice and must be bit-equal run to run.

Bounds at op level, per map of N elements (eps64, eps32 the float64 / float32 machine epsilons).  KL, CC and their parts of a
dlogit are bounded as tests/test_gpu_map_loss.py derives (8 N eps64 (sum |q log(.)| + 1); 16 N eps64; one float32 rounding plus a
cancellation floor of 8 N eps64 of the term magnitudes).  The new terms, on sigmoid heads (kernel and reference read the same
float32 s, so they differ by float64 rounding only):
* NSS = (S_f/F - sbar) / sigma.  S_f and S are sums of at most N terms: the numerator is within N eps64 of |S_f|/F + |sbar|,
  which over sigma is nss_mag.  sigma = sqrt(A/N): A moves with sbar by 2 sum |s - sbar| dsbar <= 2 N eps64 sbar sqrt(N A), a
  relative N eps64 sbar/sigma <= N eps64 nss_mag of sigma, plus its own N eps64.  So NSS is within
  8 N eps64 (nss_mag + |NSS| (1 + nss_mag)).
* SIM = sum min(p', q') with p'_i = (s_i - lo)/Ds.  The kernel forms Ds = (hi - lo) U as S - N lo, a difference of two
  quantities each within N eps64 of its magnitude: a relative N eps64 amp_s of Ds, amp_s = (sum |s| + N |lo|)/Ds (and amp_y
  for q').  min is 1-Lipschitz and sum p' = sum q' = 1, so SIM is within 8 N eps64 (amp_s + amp_y + 1).
* dlogits: the NSS part of dL/ds is formed from f_i/(F sigma), 1/(N sigma) and NSS (s_i - sbar)/A (dnss_mag), each carrying the
  relative errors above, 8 N eps64 (1 + nss_mag); the SIM part from [p' < q']/Ds and G/Ds (dsim_mag) with 8 N eps64 (1 + amp_s
  + amp_y).  The indicator [p'_i < q'_i] is decided on values that carry that relative error: the test maps are drawn without
  ties closer than it (asserted), since a flipped indicator is a different, equally valid subgradient, not an error.
* Raw heads: the kernel's s = 1/(1+expf(-z)) may differ from numpy's float32 form by delta_i <= 4 eps32 s_i.  To first order
  (taken twice for the second) NSS moves by sum |dNSS/ds_i| delta_i; SIM by sum |dp'_i| <= 2 (sum delta + N delta_lo)/Ds =
  8 eps32 amp_s.  In a dlogit, |dL/ds_i| delta_i through s (1 - s), the shift of A (16 eps32 (1 + sum |s - sbar| s / A) of the
  term magnitudes, as for CC), the shift of NSS times |s_i - sbar|/A, and for SIM 16 eps32 amp_s/Ds (G by 8 eps32 amp_s, 1/Ds by
  4 eps32 amp_s of dsim_mag <= 2/Ds); an element whose p' and q' are closer than 32 eps32 amp_s (p' + q') may have its
  indicator decided the other way: w_sim/Ds more.
* The total folds the weighted map terms in map order: the sum of the maps' bounds plus (maps + 2) eps64 of the sum of |terms|."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import saliency_loss_ref as ref      # noqa: E402
from sap3d_tensorflow_amd import ops, P3dError, P3DSession, synthetic    # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)
TINY32 = float(np.finfo(np.float32).tiny)
SHAPES = [(3, (7, 9)), (2, (32, 32)), (2, (64, 65)), (32, (112, 112))]
WEIGHTS = [(1.0, 1.0, 1.0, 0.0), (1.0, 1.0, 1.0, 1.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0), (0.25, 2.5, 0.5, 3.0)]


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def blocks_per_map(n):
    return max(1, min(256, -(-n // 2048)))


def twice(z, p, y, f, maps, ts, offset, w, loss0=0.0):
    a = ops.saliency_loss(z, p, y, f, maps, z.size // maps, ts, offset, w[0], w[1], w[2], w[3], loss0)
    b = ops.saliency_loss(z, p, y, f, maps, z.size // maps, ts, offset, w[0], w[1], w[2], w[3], loss0)
    assert a[0] == b[0] and bits_equal(a[1], b[1]) and bits_equal(a[2], b[2]) and a[3] == b[3], "run-to-run difference"
    return a


def random_maps(maps, h, w, seed):
    """Logits, a blob-plus-noise density and fixations drawn from it (bytes on both sides of the threshold)."""
    rng = np.random.default_rng(seed)
    z = rng.normal(0, 2, (maps, h, w)).astype(np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = rng.uniform(0, h, (maps, 1, 1)), rng.uniform(0, w, (maps, 1, 1))
    y = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * (0.2 * max(h, w)) ** 2)) * 0.8 + 0.2 * rng.random((maps, h, w))
    hit = rng.random((maps, h, w)) < 0.05 + 0.1 * y
    f = np.where(hit, rng.integers(128, 256, (maps, h, w)), rng.integers(0, 128, (maps, h, w))).astype(np.uint8)
    return z, y.astype(np.float32), f


def check(z, y, f, maps, ts, offset, w, loss0=0.0):
    """Runs the hook on logits z (pred = their float32 sigmoid), targets y and bytes f, checks it against saliency_loss_ref
    within the module's bounds, and returns (loss, dlogits, per_map)."""
    kw, cw, nw, sw = w
    z = np.asarray(z, np.float32).ravel()
    y = np.asarray(y, np.float32).ravel()
    f = np.asarray(f, np.uint8).ravel()
    s = ref.sigmoid32(z)
    n = z.size // maps
    loss, dl, per, info = twice(z, s, y, f, maps, ts, offset, w, loss0)
    assert info == (3, blocks_per_map(n), 1 if offset == 0 and n % 4 == 0 else 2), (info, n, offset)
    assert np.isfinite(loss) and np.all(np.isfinite(dl))
    s64 = s.astype(np.float64).reshape(maps, n)
    y64 = y.astype(np.float64).reshape(maps, n)
    fb = f.reshape(maps, n)
    delta = np.zeros_like(s64) if ts else 4 * EPS32 * s64
    dl = dl.reshape(maps, n)
    want_total, bound_total, mag_total = 0.0, 0.0, abs(loss0)
    for m in range(maps):
        r = ref.one_map(s64[m], y64[m], fb[m], kw, cw, nw, sw)
        rk = ref.klcc.one_map(s64[m], y64[m], 1.0, 0.0)
        rc = ref.klcc.one_map(s64[m], y64[m], 0.0, 1.0)
        dsum = lambda g: float((np.abs(g) * delta[m]).sum())      # noqa: E731
        b_kl = 8 * n * EPS64 * (rk["kl_mag"] + 1) + 2 * dsum(rk["dlds"])
        b_cc = 16 * n * EPS64 + 2 * dsum(rc["dlds"])
        assert abs(per[m, 0] - r["kl"]) <= b_kl, (m, per[m, 0], r["kl"], b_kl)
        if r["defined"]:
            assert abs(per[m, 1] - r["cc"]) <= b_cc, (m, per[m, 1], r["cc"], b_cc)
        else:
            assert np.isnan(per[m, 1]), (m, per[m, 1])
        nss_on = nw > 0 and r["nss_defined"]      # with w_nss = 0 the fixations are not read: NSS is reported undefined
        b_nss = b_sim = 0.0
        if nss_on:
            b_nss = 8 * n * EPS64 * (r["nss_mag"] + abs(r["nss"]) * (1 + r["nss_mag"])) + 2 * dsum(r["dnss"])
            print("map %d NSS %.17g want %.17g bound %.3g" % (m, per[m, 2], r["nss"], b_nss))
            assert abs(per[m, 2] - r["nss"]) <= b_nss, (m, per[m, 2], r["nss"], b_nss)
        else:
            assert np.isnan(per[m, 2]), (m, per[m, 2])
        if r["sim_defined"]:
            b_sim = 8 * n * EPS64 * (r["amp_s"] + r["amp_y"] + 1) + (0.0 if ts else 16 * EPS32 * r["amp_s"])
            print("map %d SIM %.17g want %.17g bound %.3g" % (m, per[m, 3], r["sim"], b_sim))
            assert abs(per[m, 3] - r["sim"]) <= b_sim, (m, per[m, 3], r["sim"], b_sim)
        else:
            assert np.isnan(per[m, 3]), (m, per[m, 3])
        want_total += r["loss"]
        mag_total += abs(r["loss"])
        bound_total += kw * b_kl + (cw * b_cc if r["defined"] else 0.0) + nw * b_nss + (sw * b_sim if r["sim_defined"] else 0.0)
        # dlogits
        sig = s64[m] * (1 - s64[m])
        want = r["dlds"] * sig
        kl_cc_mag = r["termmag"] - nw * r["dnss_mag"] - sw * r["dsim_mag"]
        ds = s64[m] - s64[m].mean()
        raw = 0.0 if ts else 16 * EPS32 * (1 + (float((np.abs(ds) * s64[m]).sum()) / r["A"] if r["A"] > 0 else 0.0))
        floor = (8 * n * EPS64 + raw) * kl_cc_mag
        if nss_on:
            floor = floor + nw * ((8 * n * EPS64 * (1 + r["nss_mag"]) + raw) * r["dnss_mag"] + 2 * dsum(r["dnss"]) * np.abs(ds) / r["A"])
        if sw > 0 and r["sim_defined"]:
            pp, qp = r["pq"]
            rel = 8 * n * EPS64 * (1 + r["amp_s"] + r["amp_y"])
            floor = floor + sw * rel * r["dsim_mag"]
            tie = rel if ts else 32 * EPS32 * r["amp_s"]
            near = (np.abs(pp - qp) <= tie * (pp + qp)) & (pp + qp > 0)      # (both minima at one element: 0 < 0 on either side)
            if ts:
                assert not near.any(), "test maps must have no ties in p', q'"
            else:
                floor = floor + sw * (16 * EPS32 * r["amp_s"] + near) / r["Ds"]
        tol = EPS32 * np.abs(want) + floor * sig + np.abs(r["dlds"]) * delta[m] + TINY32
        err = np.abs(dl[m] - want)
        print("map %d dlogits max err %.3g, max err/tol %.3g" % (m, err.max(), (err / tol).max()))
        bad = err > tol
        assert not bad.any(), (m, np.flatnonzero(bad)[:5], dl[m][bad][:5], want[bad][:5], tol[bad][:5])
    assert abs(loss - (loss0 + want_total)) <= bound_total + (maps + 2) * EPS64 * mag_total, (loss, loss0 + want_total)
    return loss, dl.ravel(), per


@pytest.mark.parametrize("maps,hw", SHAPES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("ts", [1, 0])
def test_op_level(maps, hw, offset, ts):
    z, y, f = random_maps(maps, hw[0], hw[1], seed=maps * 7 + hw[0] + offset * 3 + ts)
    weights = WEIGHTS if maps < 32 else [WEIGHTS[1], WEIGHTS[-1]]
    for w in weights:
        check(z, y, f, maps, ts, offset, w)


def test_adds_to_the_loss():
    z, y, f = random_maps(3, 7, 9, 1)
    l0, d0, p0 = check(z, y, f, 3, 1, 0, WEIGHTS[1])
    l1, d1, p1 = check(z, y, f, 3, 1, 0, WEIGHTS[1], loss0=123.25)
    assert l1 == 123.25 + l0 and bits_equal(d0, d1) and bits_equal(p0, p1)


# ---- edge maps -----------------------------------------------------------------------------------------------------------
def edge_maps(h, w):
    rng = np.random.default_rng(11)
    n = h * w
    z = rng.normal(0, 2, (7, n))
    y = rng.random((7, n))
    f = np.where(rng.random((7, n)) < 0.2, 255, 0).astype(np.uint8)
    f[:, 3] = 255
    f[0] = rng.integers(0, 128, n)                   # 0: no fixated byte (every byte below the threshold, 127 among them)
    f[0, 1] = 127
    f[1] = rng.integers(128, 256, n)                 # 1: every byte fixated (S_f / F = sbar: NSS = 0 up to rounding)
    f[1, 1] = 128
    z[2] = 0.7                                       # 2: constant s: no CC, NSS, SIM
    y[3] = 0.5                                       # 3: constant y: no CC, SIM
    y[4] = 0.0                                       # 4: an all-zero y: no CC, SIM; KL = 0
    f[5] = np.where(np.arange(n) % 2 == 0, 127, 128)   # 5: the two bytes that straddle the threshold
    return z.astype(np.float32), y.astype(np.float32), f      # 6: an ordinary map


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("ts", [1, 0])
@pytest.mark.parametrize("hw", [(7, 9), (16, 16)], ids=lambda v: "%dx%d" % v)
def test_edge_maps(offset, ts, hw):
    z, y, f = edge_maps(*hw)
    n = hw[0] * hw[1]
    for w in WEIGHTS:
        loss, dl, per = check(z, y, f, 7, ts, offset, w)
        dl = dl.reshape(7, n)
        assert np.isnan(per[2, 1]) and np.isnan(per[2, 2]) and np.isnan(per[2, 3])
        assert np.isnan(per[0, 2]) and np.isnan(per[3, 3]) and np.isnan(per[4, 3]) and per[4, 0] == 0
        if w[2] > 0:
            assert abs(per[1, 2]) <= 1e-12                           # every element fixated
            s5 = ref.sigmoid32(z[5]).astype(np.float64)
            want = (s5[1::2].mean() - s5.mean()) / s5.std()          # byte 128 is a fixation, byte 127 is not
            assert abs(per[5, 2] - want) <= 1e-6
        if w[0] == 0 and w[1] == 0:
            assert np.all(dl[2] == 0)            # constant s: every term that is on is undefined there and adds nothing
            if w[2] > 0:
                assert np.all(dl[0] == 0)        # no fixation: the NSS term adds nothing
            else:
                assert np.all(dl[3] == 0) and np.all(dl[4] == 0)      # constant y: the SIM term adds nothing


# ---- bit identity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maps,hw", SHAPES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("ts", [1, 0])
def test_without_the_new_terms_it_is_kld_cc_bit_for_bit(maps, hw, ts):
    z, y, f = random_maps(maps, hw[0], hw[1], 5)
    z, y = z.ravel(), y.ravel()
    s = ref.sigmoid32(z)
    garbage = np.random.default_rng(0).integers(0, 256, z.size).astype(np.uint8)
    for a, b in [(1.0, 1.0), (0.25, 2.5), (1.0, 0.0), (0.0, 1.0)]:
        for offset in (0, 1):
            want = ops.map_loss(z, s, y, maps, z.size // maps, ts, offset, a, b, 0.5)
            for fix in (f, garbage, None):
                got = ops.saliency_loss(z, s, y, fix, maps, z.size // maps, ts, offset, a, b, 0.0, 0.0, 0.5)
                assert got[0] == want[0] and bits_equal(got[1], want[1]) and bits_equal(got[2][:, :2], want[2]) and got[3] == want[3]
                assert np.all(np.isnan(got[2][:, 2]))


def test_edge_maps_without_the_new_terms_are_kld_cc_bit_for_bit():
    z, y, f = edge_maps(7, 9)
    s = ref.sigmoid32(z.ravel())
    for ts in (1, 0):
        want = ops.map_loss(z.ravel(), s, y.ravel(), 7, 63, ts, 0, 1.0, 1.0)
        got = ops.saliency_loss(z.ravel(), s, y.ravel(), f, 7, 63, ts, 0, 1.0, 1.0, 0.0, 0.0)
        assert got[0] == want[0] and bits_equal(got[1], want[1]) and bits_equal(got[2][:, :2], want[2])


@pytest.mark.parametrize("hw", [(7, 9), (64, 65), (112, 112)], ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("ts", [1, 0])
def test_a_map_does_not_depend_on_its_position_or_alignment(hw, ts):
    z, y, f = random_maps(8, hw[0], hw[1], 21)
    z, y, f = z.reshape(8, -1), y.reshape(8, -1), f.reshape(8, -1)
    s = ref.sigmoid32(z)
    w = WEIGHTS[-1]
    full = twice(z.ravel(), s.ravel(), y.ravel(), f.ravel(), 8, ts, 0, w)
    for off in (1, 2, 3):
        r = twice(z.ravel(), s.ravel(), y.ravel(), f.ravel(), 8, ts, off, w)
        assert r[3][2] == 2 and r[0] == full[0] and bits_equal(r[1], full[1]) and bits_equal(r[2], full[2])
    n = z.shape[1]
    # map 5 alone, and as the second of a batch of three
    one = twice(z[5], s[5], y[5], f[5], 1, ts, 0, w)
    pick = [2, 5, 0]
    three = twice(z[pick].ravel(), s[pick].ravel(), y[pick].ravel(), f[pick].ravel(), 3, ts, 3, w)
    assert bits_equal(one[1], full[1][5 * n:6 * n]) and bits_equal(one[2][0], full[2][5])
    assert bits_equal(three[1][n:2 * n], one[1]) and bits_equal(three[2][1], one[2][0])


# ---- networks --------------------------------------------------------------------------------------------------------------
SHAPE = (2, 16, 32, 32)
NETS = [("unet", True), ("concat", False)]          # a sigmoid head and a raw one


def net_inputs(seed=0):
    x, y = synthetic.synthetic_clip(seed, SHAPE + (3,)), synthetic.synthetic_target(seed + 3, SHAPE)
    return x, y, synthetic.synthetic_fixations(seed + 7, y)


def small_session(structure, seed=1):
    return P3DSession(structure, batch=SHAPE[0], frames=SHAPE[1], height=SHAPE[2], width=SHAPE[3], base=8, blocks=(1, 1, 2), seed=seed)


@pytest.mark.parametrize("structure,sigmoid_head", NETS)
def test_network_loss_and_terms_match_float64_on_the_fetched_pred(structure, sigmoid_head):
    x, y, f = net_inputs()
    s = small_session(structure)
    maps = SHAPE[0] * SHAPE[1]
    for name, w in (("kld_cc_nss", (1, 1, 1, 0)), ("kld_cc_nss_sim", (1, 1, 1, 1))):
        s.set_loss(name)
        loss, pred = s.backward(x, y, 0.0, fixations=f)
        sal = pred if sigmoid_head else ref.sigmoid32(pred)
        want, per, _, _ = ref.saliency_loss(sal, y, f, maps, *w)
        assert np.isfinite(loss) and abs(loss - want) <= 1e-5 * abs(want), (name, loss, want)
        t = s.last_loss_terms()
        assert t["counts"] == dict(kld=maps, cc=maps, nss=maps, sim=maps)
        for k, col in (("kld", 0), ("cc", 1), ("nss", 2), ("sim", 3)):
            assert abs(t[k] - per[:, col].mean()) <= 1e-5 * max(1.0, abs(per[:, col].mean())), (k, t[k], per[:, col].mean())
    # a map without fixations counts for KL, CC and SIM only
    f0 = f.copy()
    f0[0, 3] = 0
    s.backward(x, y, 0.0, fixations=f0)
    assert s.last_loss_terms()["counts"] == dict(kld=maps, cc=maps, nss=maps - 1, sim=maps)
    s.set_loss("kld_cc")
    s.backward(x, y, 0.0)
    with pytest.raises(P3dError):
        s.last_loss_terms()
    s.close()


def test_stale_fixations_are_refused():
    x, y, f = net_inputs()
    s = small_session("unet")
    s.set_loss("kld_cc_nss")
    with pytest.raises(P3dError, match="p3d_upload_fixations"):
        s.train_step(x, y, seed=1)                       # never uploaded
    s.upload(x, y)
    with pytest.raises(P3dError, match="p3d_upload_fixations"):
        s.train_step_device(0.5, seed=1)
    assert np.isfinite(s.train_step(x, y, seed=1, fixations=f))
    with pytest.raises(P3dError, match="p3d_upload_fixations"):
        s.train_step(x, y, seed=2)                       # those of the previous batch
    with pytest.raises(P3dError, match="p3d_upload_fixations"):
        s.backward(x, y)
    s.train_step_device(0.5, seed=2)                     # device-resident: reuses them, as it reuses x and y
    assert np.isfinite(s.last_loss())
    s.upload_fixations(f)
    assert np.isfinite(s.backward(x, y)[0])
    s.set_loss("kld_cc_nss", nss_weight=0.0)             # no NSS term: no fixations needed
    assert np.isfinite(s.train_step(x, y, seed=3))
    s.close()
    s = small_session("unet")
    s.set_loss("kld_cc_nss_sim", nss_weight=0.0)         # nor ever uploaded
    assert np.isfinite(s.train_step(x, y, seed=3))
    assert s.last_loss_terms()["counts"]["nss"] == 0
    s.close()


def test_setter_refusals_change_nothing():
    import ctypes as C
    from sap3d_tensorflow_amd._lib import lib
    x, y, f = net_inputs()
    s = small_session("unet")
    s.set_loss("kld_cc_nss_sim", cc_weight=0.5, sim_weight=2.0)
    a = s.backward(x, y, 0.0, fixations=f)
    for w in ((-1.0, 1, 1, 1), (1, float("nan"), 1, 1), (1, 1, float("inf"), 1), (0, 0, 0, 0)):
        assert lib().p3d_set_saliency_weights(s._h, *[C.c_float(v) for v in w]) == -1
    assert lib().p3d_set_loss(s._h, 5) == -1
    b = s.backward(x, y, 0.0, fixations=f)
    assert a[0] == b[0] and bits_equal(a[1], b[1])
    s.close()


def trajectory(s, steps):
    out = []
    for i in range(steps):
        x, y, _ = net_inputs(i)
        out.append(np.float32(s.train_step(x, y, dropout=0.5, seed=10 + i)))
    return out, {n: s.get_param(n) for n, _, _ in s.variables()}


@pytest.mark.parametrize("name", ["smooth_l1", "kld_cc"])
def test_other_losses_are_untouched_by_the_new_setters(name):
    """The default loss and kld_cc train the same bits after the new kind was selected, weighted, fed fixations, run (a
    backward: no update) and switched away from."""
    runs = []
    for touch in (False, True):
        s = small_session("unet")
        s.set_loss(name)
        if touch:
            x, y, f = net_inputs(5)
            s.set_loss("kld_cc_nss_sim", kld_weight=0.5, cc_weight=0.25, nss_weight=3.0, sim_weight=2.0)
            s.backward(x, y, 0.0, fixations=f)
            s.set_loss(name)
        runs.append(trajectory(s, 2))
        s.close()
    assert [v.tobytes() for v in runs[0][0]] == [v.tobytes() for v in runs[1][0]]
    assert all(bits_equal(v, runs[1][1][n]) for n, v in runs[0][1].items())


def test_schedule_replaces_the_loss_launches_only():
    x, y, f = net_inputs()
    s = small_session("unet")
    s.upload(x, y, fixations=f)
    s.set_loss("kld_cc")
    s.schedule()
    base = s.schedule()
    s.set_loss("kld_cc_nss_sim")
    sal = s.schedule()
    s.close()
    assert len(sal) == len(base)
    diff = [(a, b) for a, b in zip(base, sal) if a != b]
    assert [b for _, b in diff] == [a.replace("map_loss_", "saliency_loss_") for a, _ in diff] and len(diff) == 3


def test_captured_step_gives_the_eager_trajectory():
    """P3D_GRAPH=1: kind-4 steps with the fixations uploaded anew before each, then a weight change (which drops the captured
    step), give the eager trajectory bit for bit."""
    script = (
        "import sys, hashlib, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "from sap3d_tensorflow_amd import P3DSession, synthetic\n"
        "shape = (2, 16, 32, 32)\n"
        "s = P3DSession('unet', batch=2, frames=16, height=32, width=32, base=8, blocks=(1, 1, 2), seed=3)\n"
        "s.set_adam(1e-3)\n"
        "losses = []\n"
        "for sw, k in ((0.0, 3), (0.5, 2)):\n"
        "    s.set_loss('kld_cc_nss_sim', sim_weight=sw)\n"
        "    for i in range(k):\n"
        "        j = len(losses)\n"
        "        y = synthetic.synthetic_target(100 + j, shape)\n"
        "        losses.append(np.float32(s.train_step(synthetic.synthetic_clip(j, shape + (3,)), y, 0.5, seed=50 + j,\n"
        "                                              fixations=synthetic.synthetic_fixations(200 + j, y))).tobytes().hex())\n"
        "        t = s.last_loss_terms()\n"
        "        losses.append(np.float64(t['nss']).tobytes().hex())\n"
        "h = hashlib.sha256()\n"
        "for n, _, _ in s.variables():\n"
        "    h.update(s.get_param(n).tobytes())\n"
        "print('RESULT', ' '.join(losses), h.hexdigest())\n"
        "s.close()\n" % ROOT)
    outs = []
    for graph in ("0", "1"):
        env = dict(os.environ, P3D_GRAPH=graph)
        r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")]
        assert line, r.stdout[-2000:]
        outs.append(line[0])
        if graph == "1":
            assert "capture failed" not in r.stderr, r.stderr[-2000:]
    assert outs[0] == outs[1]
    losses = [np.frombuffer(bytes.fromhex(v), np.float32)[0] for v in outs[0].split()[1:11:2]]
    assert np.all(np.isfinite(losses))


def test_train_driver_with_kld_cc_nss_and_accumulation(tmp_path):
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "drivers", "train.py"), "--loss", "kld_cc_nss",
                        "--accum-steps", "2", "--batch", "2", "--imagesize", "32", "32", "--steps", "4", "--plotiter", "1",
                        "--validiter", "100", "--saveiter", "100"],
                       cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    losses = [float(v) for v in re.findall(r"Training Loss (\S+)", r.stdout)]
    terms = re.findall(r"KLD (\S+) CC (\S+) NSS (\S+) SIM (\S+)", r.stdout)
    assert len(losses) == 2 and np.all(np.isfinite(losses)), r.stdout[-3000:]
    assert len(terms) == 2 and np.all(np.isfinite(np.array(terms, np.float64))), r.stdout[-3000:]
