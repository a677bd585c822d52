"""Decision-pinned gradient parity.

The whole-graph gradient tests allow a case what was MEASURED above the fp32-noise bound (tests/gates.py), on the grounds that
a float32 forward takes a handful of ReLU / max-pool decisions differently from the float64 oracle's and that each such flip
moves gradient tensors by per cent.  This file turns that explanation into something a test can fail: the oracle is
differentiated on the SAME piecewise-linear branch as the HIP pass -- its ReLU masks and max-pool choices are taken from the HIP
forward (P3DSession.decisions(): the gates come out of the product's own backward kernels, the pools' arg-max from the
product's own pool input) -- and the HIP gradients then have to meet the PLAIN bound against that, every tensor, with nothing
measured and nothing allowed.  What is left between the two is summation order.

How much summation order may leave is not a constant either.  The float32 oracle is evaluated on the same pins (same masks, same
pool choices, same dropout pattern), and with e32[n] its rel-L2 against float64 on tensor n and m the median of e32 over the
tensors, every HIP tensor has to be within
    bound[n] = 5 * max(e32[n], m)
AND within the flat bound (tests/pinned_ref.py: the rule can only ask more than PLAIN did).  Its two ingredients: the factor 5 is
that of every noise bound of this suite (gates.noise_excess, attention_ref.rule, test_gpu_full.py: 5 x the float32 oracle's own
distance); the floor m keeps a tensor that numpy happens to sum almost exactly from asking the same of the HIP order, and it is
computed from the reference in the run itself -- no measured constant is committed.  (The three GroupNorm cases print the rule's
figures and stay on the flat bound: see the comment in their test.)  tests/test_pinned_yardstick_cpu.py shows on
the reference alone that two honest float32 orders stay within a ratio of 3.4 of each other while one conv's input gradient off by
1e-3 -- which no tensor shows above PLAIN -- reaches 23 - 31.  For the typical tensor the rule sits at 1e-4, PLAIN at 2e-3.

Every case of tests/golden/measured_gates.json on a BatchNorm graph that sits above the noise bound is here, with the graph
sizes of those tests; the number of decisions that differed and their share of all decisions is printed and bounded."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from oracle import p3d
import pinned_ref            # noqa: E402

pytestmark = pytest.mark.gpu

PLAIN = pinned_ref.PLAIN          # the absolute part of the fp32-noise bound of the gradient tests: the flat bound of this file


def _randomised(structure, cfg):
    from test_gpu_net import randomise_norm_params      # (attention mixing scalars off zero too)
    return randomise_norm_params(p3d.init_params(1, structure, cfg, dtype=np.float64))


def _pinned_errors(s, p64, x, y, structure, cfg, dropout=0.0, keep=None, pool_tol=1e-3):
    """rel-L2 of every HIP gradient, and of the float32 oracle's, against the float64 oracle differentiated on the HIP pass's own
    decisions."""
    pins = s.decisions()
    pins["pool_tol"] = pool_tol
    assert len(pins["relu"]) > 10 and len(pins["pool"]) >= 4

    def oracle(dtype):
        params = p64 if dtype is np.float64 else {k: v.astype(dtype) for k, v in p64.items()}
        return p3d.loss_and_grads(params, x.astype(dtype), y.astype(dtype), dropout, True, structure, cfg, dtype,
                                  keep_mask=None if keep is None else keep.astype(dtype), pins=pins)
    l64, pr64, g64, g = oracle(np.float64)
    log = g.tape.pin_log
    assert log["relu"] >= pins["relu_sites"], (log, pins["relu_sites"])      # every gated pass of the HIP graph found its ReLU(s) in the oracle
    assert log["pool"] >= 4
    errs, log["zero_gradients"] = pinned_ref.errors(s.get_grad, g64)
    _, _, g32, g = oracle(np.float32)
    assert g.tape.pin_log["relu"] == log["relu"] and g.tape.pin_log["pool"] == log["pool"]
    e32, _ = pinned_ref.errors(g32, g64)
    return l64, pr64, errs, e32, log


def _check(tag, errs, e32, log, bound=PLAIN, flip_share=1e-4, rule=True):
    worst = sorted(((e, n) for n, e in errs.items()), reverse=True)[:3]
    print("%s: %d gradient tensors, worst %.2e (%s), median %.2e | %d of %d ReLU decisions and %d max-pool choices differed from the "
          "float64 oracle's own" % (tag, len(errs), worst[0][0], worst[0][1], float(np.median(list(errs.values()))), log["relu_flips"],
                                    log["elements"], log["pool_flips"]))
    print("%s: median HIP %.2e, float32 oracle on the same decisions %.2e (worst %.2e) | largest e_hip / max(e32, median e32): %s"
          % (tag, float(np.median(list(errs.values()))), float(np.median(list(e32.values()))), max(e32.values()), pinned_ref.table(errs, e32, 5)))
    assert worst[0][0] <= bound, worst
    # the flips are the rare near-zero decisions the tolerances speak of, not a different function
    assert log["relu_flips"] <= flip_share * log["elements"] + 8, log
    # the rule: every tensor within 5 x the float32 oracle's own error on these decisions (floored at its median) and within `bound`
    fails = pinned_ref.failures(errs, e32, flat=bound)
    if not rule:
        print("%s: NOT held to the rule: %d of %d tensors above it" % (tag, len(fails), len(errs)))
        return
    assert not fails, ("%d tensors above 5 x max(e32, median e32): (error, bound, name)" % len(fails), fails[:5])


CASES = [
    ("unet", p3d.NetConfig(base=8, blocks=(3, 3, 3)), (2, 16, 32, 32)),            # golden/unet_b8_333 (gate 8.8e-3), backward_small
    ("unet", p3d.NetConfig(base=16, blocks=(1, 2, 4)), (1, 16, 48, 32)),           # golden/unet_b16_124, backward_small
    ("concat", p3d.NetConfig(base=16, blocks=(1, 2, 4)), (1, 16, 48, 32)),
    ("unet++nonsa", p3d.NetConfig(base=16, blocks=(1, 2, 4)), (1, 16, 48, 32)),    # unetpp_nonsa/base16_1x16x48x32 (gate 7.2e-3)
    ("unet++ds", p3d.NetConfig(base=16, blocks=(1, 1, 2)), (2, 16, 32, 32)),       # unetpp_ds/base16_2x16x32x32 (gate 4.3e-3)
    # full width (base 64): the head's 3x3x3 convs have 128-wide outputs over >= 2048 positions, so their grouped filter-gradient
    # launches take the 64x128 tile (conv_wgrad2.hip, p3d_launch_wgrad2_group) -- and the stem's runs on stem_wgrad.hip
    ("unet++nonsa", p3d.NetConfig(base=64, blocks=(1, 1, 1)), (2, 16, 64, 64)),
]


@pytest.mark.parametrize("structure,cfg,shape", CASES)
def test_gradients_on_the_hip_pass_own_decisions(structure, cfg, shape):
    from test_gpu_net import make_session
    p64 = _randomised(structure, cfg)
    p32 = {k: v.astype(np.float32) for k, v in p64.items()}
    x = p3d.synthetic_clip(0, shape + (3,))
    y = p3d.synthetic_target(3, shape)
    s = make_session(cfg, shape, p32, structure)
    loss, pred = s.backward(x, y, 0.0)
    l64, pr64, errs, e32, log = _pinned_errors(s, p64, x, y, structure, cfg)
    assert abs(loss - l64) <= 1e-5 * abs(l64)
    assert np.abs(pred - pr64).max() <= 3e-4
    _check("%s base%d %s" % (structure, cfg.base, "x".join(map(str, shape))), errs, e32, log)
    if cfg.base == 64:          # the full-width case is here for two kernels: make sure the launch list holds them
        s.upload(x, y)
        launches = [ln for ln in s.schedule(0.0, seed=0) if ln.startswith("L ")]
        assert any("wgrad2_kernel<64,128>(grouped)" in ln for ln in launches), "no grouped filter-gradient launch on 64x128 tiles"
        assert any("stem_wgrad" in ln for ln in launches), "the stem's filter gradient did not run on stem_wgrad.hip"
    s.close()


def test_dropout_case_on_the_hip_pass_own_decisions():
    """unetpp_ds_dropout/base16_2x16x32x32, the largest measured gate of the suite (2.3e-2): dropout 0.5 on the last attention
    block's output doubles the weight of every flipped element."""
    from test_gpu_net import make_session
    structure, cfg, shape = "unet++ds", p3d.NetConfig(base=16, blocks=(1, 1, 2)), (2, 16, 32, 32)
    p64 = _randomised(structure, cfg)
    p32 = {k: v.astype(np.float32) for k, v in p64.items()}
    x = p3d.synthetic_clip(0, shape + (3,))
    y = p3d.synthetic_target(3, shape)
    s = make_session(cfg, shape, p32, structure)
    s.forward(x, 0.0, True)
    base = s.activation('x_1_3_sa')
    loss, pred = s.backward(x, y, dropout=0.5, seed=11)
    dropped = s.activation('x_1_3_sa')
    keep = np.where(base != 0, dropped != 0, True)
    l64, pr64, errs, e32, log = _pinned_errors(s, p64, x, y, structure, cfg, dropout=0.5, keep=keep)
    assert abs(loss - l64) <= 1e-5 * abs(l64)
    _check("unet++ds dropout 0.5", errs, e32, log)
    s.close()


def test_reference_architecture_on_the_hip_pass_own_decisions():
    """config2/worst_ratio: P3D-199 (199 layers) at two clips of 16x112x112.  Unpinned, two float32 evaluations of this graph sit
    0.14-0.21 rel-L2 apart on the deep gradients and the test can only compare error levels; pinned, HIP and the float64 oracle
    differentiate one and the same branch and every one of the ~590 gradient tensors has to agree to the plain bound."""
    from sap3d_tensorflow_amd import P3DSession
    params = p3d.init_params(1, 'unet', None)
    x = p3d.synthetic_clip(0, (2, 16, 112, 112, 3))
    y = p3d.synthetic_target(3, (2, 16, 112, 112))
    s = P3DSession('unet', batch=2)
    s.load(params)
    loss, pred = s.backward(x, y, 0.0)
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    # (block 46's output sits 3e-3 from the float64 oracle's at this depth -- the forward amplification of this random-init net,
    #  DESIGN.md section 2 -- so the pool inputs are matched with a wider tolerance and more gates differ: 1e-4 of 55.6 M)
    l64, pr64, errs, e32, log = _pinned_errors(s, p64, x, y, 'unet', None, pool_tol=2e-2)
    assert abs(loss - l64) <= 1e-5 * abs(l64)
    # (the saliency maps are compared by the unpinned tests; pinning moves the oracle's forward by the flipped elements' 1e-7)
    # Tensors whose true gradient is zero (the biases of convS / convT sit in front of a batch-statistics BatchNorm: 94 of them)
    # are noise against the floor on both sides; every other tensor -- ~590 -- within 2e-2, the median within 3e-3 (measured
    # 1.6e-3: the forward of this random-init net itself sits 3e-3 from float64 at block 46, and that enters every gradient
    # upstream of it).  Unpinned, the same comparison reads 0.14 (median) / 0.21 (max), test_config2_forward_backward.
    zero = set(log["zero_gradients"])
    live = {n: e for n, e in errs.items() if n not in zero}
    assert len(live) > 500 and len(zero) < 150, (len(live), len(zero))
    # The rule on the live tensors turns the sentence about forward amplification into a test: the float32 oracle's forward is
    # amplified by the same net on the same decisions, so 5 x its error (floored at its median over the live tensors) is what
    # that amplification may explain, tensor by tensor.
    _check("P3D-199 2x16x112x112 (tensors with a gradient)", live, {n: e32[n] for n in live}, log, bound=2e-2, flip_share=3e-4)
    assert float(np.median(list(live.values()))) <= 3e-3
    assert max(errs[n] for n in zero) <= 2e-1, sorted(((errs[n], n) for n in zero), reverse=True)[:3]
    s.close()


# ---- GroupNorm + CBAM graphs (BASELINE configs[3]) --------------------------------------------------------------------------
GN_CASES = [
    ("gn_p3d", "p3d", p3d.NetConfig(base=16, blocks=(1, 1, 2)), (1, 16, 32, 32)),            # golden/gn_p3d_b16_112 (gate 1.1e-2)
    ("gn_p3d_decoder", "decoder", p3d.NetConfig(base=16, blocks=(1, 1, 2)), (1, 16, 32, 32)),  # golden/gn_decoder_b16_112 (gate 1.3e-2)
    ("gn_p3d_decoder", "decoder", p3d.NetConfig(base=16, blocks=(1, 1, 2)), (2, 16, 32, 32)),  # gn_decoder/base16_2x16x32x32 (gate 1.7e-2)
]


@pytest.mark.parametrize("structure,head,cfg,shape", GN_CASES)
def test_gn_gradients_on_the_hip_pass_own_relu_and_pool_decisions(structure, head, cfg, shape):
    """The GroupNorm + CBAM graphs with the ReLU gates of every GroupNorm pass and the max-pool choices pinned to the HIP pass's
    (CBAM's own decisions -- the arg-max of its two max-pools and the ReLU of its 1/8-width MLP -- stay the oracle's: a flip there
    would show here as an excess, and the printed line says whether one does)."""
    from oracle import p3d_gn
    from test_gpu_net import make_session
    p64 = p3d_gn.init_params(1, cfg, dtype=np.float64, head=head)
    rng = np.random.default_rng(7)
    for k, v in p64.items():
        if k.endswith('gamma'):
            v[:] = rng.uniform(0.5, 1.5, v.shape)
        elif k.endswith(('beta', '/bias')):
            v[:] = rng.uniform(-0.3, 0.3, v.shape)
    p32 = {k: v.astype(np.float32) for k, v in p64.items()}
    x = p3d.synthetic_clip(0, shape + (3,))
    y = p3d.synthetic_target(3, shape)
    s = make_session(cfg, shape, p32, structure)
    loss, pred = s.backward(x, y, 0.0)
    pins = s.decisions()
    assert pins["relu_sites"] > 10 and len(pins["pool"]) >= 3
    pins["relu"] = {k.split('/')[-1]: v for k, v in pins["relu"].items()}      # (the decoder head's variables live in scope 'P3D/')
    l64, pr64, g64, g = p3d_gn.loss_and_grads(p64, x.astype(np.float64), y.astype(np.float64), 0.0, True, cfg, np.float64, head=head, pins=pins)
    log = g.tape.pin_log
    assert log["relu"] >= pins["relu_sites"], (log, pins["relu_sites"])
    assert abs(loss - l64) <= 1e-5 * abs(l64)
    errs, _ = pinned_ref.errors(s.get_grad, g64)
    g32 = p3d_gn.loss_and_grads(p32, x, y, 0.0, True, cfg, np.float32, head=head, pins=pins)[2]
    e32, _ = pinned_ref.errors(g32, g64)
    # These three cases stay on the flat bound.  Measured: medians 8.5e-6 / 4.7e-5 / 6.6e-5 against the float32 oracle's 2.8e-6 /
    # 1.6e-5 / 1.3e-5, worst ratios 6.4 / 9.2 / 11.0, up to 49 of 130 tensors above the rule.  The cause is known and is no
    # summation order: gn_stats_kernel sums y and y^2 in float32 partials, so var = E[y^2] - mean^2 carries eps32 * (sigma^2 +
    # mu^2), and group_norm_1 has a nearly constant channel (mu^2 / sigma^2 = 43) whose inverse std comes out 6e-6 off
    # (EXPERIMENTS.md, "The pinned gate at the float32 oracle's own error").  With partials of y - pivot the same cases read
    # ratios 2.4 / 3.0 / 4.7 and pass; that kernel is not in, because it changes the forward's near-zero decisions and two
    # decision-sensitive tests outside this file's reach then fail.  The lines are printed so that the fix can be judged here.
    _check("%s base%d %s" % (structure, cfg.base, "x".join(map(str, shape))), errs, e32, log, rule=False)
    s.close()
