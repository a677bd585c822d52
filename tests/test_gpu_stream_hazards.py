"""Cross-stream ordering of the train step under perturbed schedules (csrc/net_sched.inc: filter gradients on a low-priority side
stream, parked decoder jobs, arenas zeroed beside the forward pass, the two-part optimiser step, all-reduce buckets on a comm
stream).  The step is bit-reproducible by design, so a correct schedule gives the same bits however its streams drift against
each other.  P3DSession.perturb (p3d_debug_perturb) lets them drift:

 * "serial": the issuing stream is synchronised after every launch, fill and all-reduce -- the host's issue order.  It is ONE
   legal order, the one in which nothing overlaps: it shows what the step computes when no race can fall either way, and it
   cannot show a missing wait (the self-test's last row);
 * "slow" producer: a delay kernel ahead of everything on one stream lets the others run ahead as far as the events allow, so
   a consumer that lacks the wait for its producer reads stale data (a missing read-after-write edge);
 * "slow" consumer: the same on the reader's stream shows a buffer that its writer's stream reuses while the reader still has
   to read it (a missing write-after-read edge).

Every run is compared bit for bit with the unperturbed run of the same script on a fresh session of the same seed, and every
perturbed run proves through perturb_count() that it was perturbed.  test_perturbation_exposes_a_missing_wait shows on a
two-launch example with the same launch / event funnel that a slow producer does expose a missing wait, at which delays."""
import os
import re
import sys

import numpy as np
import pytest

from oracle import p3d

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_gpu_determinism import CASES          # noqa: E402

pytestmark = pytest.mark.gpu

DELAY_US = 200           # P3DSession.perturb's default; DESIGN.md ("Schedule perturbation") has the ladder behind it
LADDER = (50, 200, 1000)
MODES = [("serial", None), ("slow", "main"), ("slow", "side")]
UNET = [c for c in CASES if c[0] == "unet"][0]                     # base 16, blocks (2, 2, 3), 2x16x48x48
UNETPP_DS = [c for c in CASES if c[0] == "unet++ds"][0]


# ---- the self-test ----------------------------------------------------------------------------------------------------------------
def test_perturbation_exposes_a_missing_wait():
    """p3d_debug_perturb_selftest: a producer on stream A overwrites a buffer of 1.0 with 2.0, a consumer on stream B copies it.
    With the wait between them every mode reads 2.0.  Without it a slow producer must read 1.0 everywhere -- the stale read is
    exposed -- while serial reads 2.0: serial alone cannot show the missing wait.  (Without wait and unperturbed is a race and
    is not asserted.)"""
    from sap3d_tensorflow_amd import ops
    for mode, slow in (("off", "producer"), ("serial", "producer"), ("slow", "producer"), ("slow", "consumer")):
        out = ops.perturb_selftest(mode, slow, DELAY_US, with_wait=True)
        assert np.array_equal(out, np.full(4096, 2.0, np.float32)), (mode, slow, np.unique(out))
    exposed = {}
    for us in LADDER:
        out = ops.perturb_selftest("slow", "producer", us, with_wait=False)
        exposed[us] = bool(np.array_equal(out, np.full(4096, 1.0, np.float32)))
        print("perturb ladder: slow producer %4d us, no wait -> stale read %s (values read: %s)"
              % (us, "exposed" if exposed[us] else "NOT exposed", np.unique(out)))
    assert exposed[DELAY_US], exposed
    out = ops.perturb_selftest("serial", "producer", DELAY_US, with_wait=False)
    assert np.array_equal(out, np.full(4096, 2.0, np.float32)), np.unique(out)


def test_perturb_hook_refuses_bad_arguments():
    from sap3d_tensorflow_amd import P3dError
    structure, cfg, shape = CASES[2]
    s = _session(structure, cfg, shape, 1)
    for delay in (0, 2001):
        with pytest.raises(P3dError):
            s.perturb("slow", "side", delay)
    with pytest.raises(ValueError):
        s.perturb("slow", None)
    s.perturb("slow", "side", 1)
    assert s.perturb_count() == (0, 0)
    s.perturb("off")
    s.close()


# ---- the harness ------------------------------------------------------------------------------------------------------------------
def _session(structure, cfg, shape, seed):
    from sap3d_tensorflow_amd import P3DSession
    return P3DSession(structure, batch=shape[0], frames=shape[1], height=shape[2], width=shape[3], base=cfg.base,
                      blocks=cfg.blocks, seed=seed)


def _inputs(shape):
    return p3d.synthetic_clip(0, shape + (3,)), p3d.synthetic_target(3, shape)


def _fixations(shape):
    rng = np.random.RandomState(7)
    return np.where(rng.rand(*shape) < 0.02, 255, 0).astype(np.uint8)


def observe(s, out, tag, opts):
    """Everything observable of the session, as bytes, under `tag`."""
    from sap3d_tensorflow_amd import _lib
    out[tag + "/loss"] = np.float32(s.last_loss()).tobytes()
    if opts.get("clip"):
        out[tag + "/grad_norm"] = np.array(s.last_grad_norm(with_sumsq=True), np.float64).tobytes()
    if opts.get("saliency"):
        t = s.last_loss_terms()
        out[tag + "/loss_terms"] = np.array([t[k] for k in ("kld", "cc", "nss", "sim")], np.float64).tobytes()
    for n, _, trainable in s.variables():
        out[tag + "/param/" + n] = s.get_param(n).tobytes()            # (BatchNorm moving statistics included)
        if trainable:
            out[tag + "/grad/" + n] = s.get_grad(n).tobytes()
            for k in range(len(_lib.SLOT_NAMES[opts.get("optimizer", "adam")])):
                out[tag + "/slot%d/" % k + n] = s.get_slot(n, k).tobytes()
            if opts.get("ema"):
                out[tag + "/ema/" + n] = s.get_ema(n).tobytes()


def seq_device_steps(s, shape, opts, out):
    """(a) train_step_device back to back with NO host synchronisation between the steps: zero_early of step N+1 runs beside the
    tail of step N.  (The losses of the earlier steps cannot be read without synchronising; the weights they led to are.)"""
    x, y = _inputs(shape)
    s.upload(x, y, fixations=_fixations(shape) if opts.get("saliency") else None)
    for i in range(opts.get("steps", 3)):
        s.train_step_device(0.5, seed=20 + i)
    observe(s, out, "end", opts)


def seq_entry_points(s, shape, opts, out):
    """(b) backward -> read gradients -> forward (inference) -> train_step -> backward: the boundaries between entry points."""
    x, y = _inputs(shape)
    loss, pred = s.backward(x, y, 0.5, seed=31)
    out["b0/loss"], out["b0/pred"] = np.float32(loss).tobytes(), pred.tobytes()
    for n, _, trainable in s.variables():
        if trainable:
            out["b0/grad/" + n] = s.get_grad(n).tobytes()
    out["f/pred"] = s.forward(x).tobytes()
    out["t/loss"] = np.float32(s.train_step(x, y, dropout=0.5, seed=32)).tobytes()
    loss, pred = s.backward(x, y, 0.5, seed=33)
    out["b1/loss"], out["b1/pred"] = np.float32(loss).tobytes(), pred.tobytes()
    observe(s, out, "end", opts)


def seq_host_steps(s, shape, opts, out):
    """train_step with host inputs (the path p3d_set_augment transforms), three steps."""
    x, y = _inputs(shape)
    for i in range(3):
        out["t%d/loss" % i] = np.float32(s.train_step(x, y, dropout=0.5, seed=40 + i)).tobytes()
    observe(s, out, "end", opts)


def run(case, sequence, setup, opts, mode, stream):
    structure, cfg, shape = case
    s = _session(structure, cfg, shape, seed=5)
    try:
        if setup:
            setup(s)
        if mode:
            s.perturb(mode, stream, DELAY_US)
        out = {}
        sequence(s, shape, opts, out)
        counts = s.perturb_count()
        s.perturb("off")
    finally:
        s.close()
    return out, counts


_BASELINES = {}


def check_invariance(key, case, sequence, mode, stream, setup=None, opts=None, prepare=None):
    """The scripted sequence under (mode, stream) against its unperturbed run (computed once per key, shared, never modified)."""
    opts = opts or {}
    if prepare:
        prepare()
    if key not in _BASELINES:
        _BASELINES[key] = run(case, sequence, setup, opts, None, None)[0]
    want = _BASELINES[key]
    got, (delays, syncs) = run(case, sequence, setup, opts, mode, stream)
    print("perturb %s %s %s: %d delays, %d syncs inserted" % (key, mode, stream or "", delays, syncs))
    # the vacuity guard: a run that was not perturbed proves nothing
    assert (syncs if mode == "serial" else delays) > 0, (key, mode, stream, delays, syncs)
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, "%d of %d observables differ under %s %s, e.g. %s" % (len(differ), len(want), mode, stream or "", differ[:6])


def _id(v):
    return v if isinstance(v, str) else None


# ---- the seven structures, both sequences ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,stream", MODES, ids=_id)
@pytest.mark.parametrize("sequence", [seq_device_steps, seq_entry_points], ids=lambda f: f.__name__)
@pytest.mark.parametrize("index", range(len(CASES)), ids=lambda i: "%s-b%d" % (CASES[i][0], CASES[i][1].base))
def test_structures_are_schedule_invariant(index, sequence, mode, stream):
    check_invariance(("structure", index, sequence.__name__), CASES[index], sequence, mode, stream)


# ---- parked decoder jobs ----------------------------------------------------------------------------------------------------------
# Parking does not depend on the clip size below the budget's threshold (net_plan.inc: on whenever the encoder's last stage has
# at most 2048 rows), so the smallest shapes of test_gpu_determinism.CASES already park; the test asserts it from the trace
# before it relies on it.
PARKED = [UNET, [c for c in CASES if c[0] == "gn_p3d_decoder"][0]]


HEAD_FILTER = re.compile(r"headc?_bwd_filter_kernel\b")    # the head's filter gradient (net.hip, head_filter_gradient): no other op launches it
HEAD_INPUT = re.compile(r"headc?_bwd_input_kernel\b")


def released_late(lines):
    """The side-stream launches of a decoder job that the walk held back until it reached the encoder.  A released job's launches
    carry the tag of the op that released them (run_backward releases as the walk REACHES the encoder, ahead of that op's own
    launches), so the job is recognised by the one decoder kernel that names its op: the head's filter gradient, which the first
    op of the backward walk queues first -- parked whenever anything is.  Released late: on the side stream under the tag of an
    encoder op (block<k>/..) instead of the head's, issued after main-stream launches of ops walked after the head, and followed
    by main-stream launches of the encoder, beside which it runs."""
    ops = [ln.split(None, 2) for ln in lines]
    launches = [(i, o[1], o[2].rsplit(" @", 1)) for i, o in enumerate(ops) if o[0] == "L" and " @" in o[2]]
    heads = [tag for _, stream, (kernel, tag) in launches if stream == "main" and HEAD_INPUT.match(kernel)]
    assert len(heads) == 1, heads
    out = []
    for i, stream, (kernel, tag) in launches:
        if stream != "side" or not HEAD_FILTER.match(kernel):
            continue
        passed = any(j < i and s == "main" and t != heads[0] for j, s, (_, t) in launches)
        beside = any(j > i and s == "main" and t.startswith("block") for j, s, (_, t) in launches)
        if tag != heads[0] and tag.startswith("block") and passed and beside:
            out.append(lines[i])
    return out


@pytest.mark.parametrize("mode,stream", [("slow", "side"), ("slow", "main")], ids=_id)
@pytest.mark.parametrize("index", range(len(PARKED)), ids=lambda i: "%s-%s" % (PARKED[i][0], "x".join(map(str, PARKED[i][2]))))
def test_parked_decoder_jobs_are_schedule_invariant(index, mode, stream):
    structure, cfg, shape = PARKED[index]
    key = ("parked", index)
    if key not in _BASELINES:
        s = _session(structure, cfg, shape, seed=5)
        s.upload(*_inputs(shape))
        late = released_late(s.schedule(0.5, seed=0))
        s.close()
        print("parked %s %s: released late: %s" % (structure, shape, late))
        assert late, "no decoder job of %s at %s is released late: the case does not exercise release_parked" % (structure, shape)
    check_invariance(key, PARKED[index], seq_device_steps, mode, stream)


# ---- options that reshape the schedule (p3d_unet at the small size, sequence (a), all modes) ----------------------------------------
def _tail(s):
    s.set_grad_clip(1.0)
    s.set_optimizer("momentum", lr=1e-3, momentum=0.9, use_nesterov=True)
    s.set_regularization(("weightdecay",))
    s.set_ema(0.9)


def _accum(s):
    s.set_grad_accum(2)
    s.set_ema(0.9)


OPTIONS = {
    "clip+nesterov+decay+ema": (UNET, seq_device_steps, _tail, dict(clip=True, optimizer="momentum", ema=True)),
    "grad_accum2+ema": (UNET, seq_device_steps, _accum, dict(ema=True, steps=4)),
    "kld_cc_nss_sim": (UNET, seq_device_steps, lambda s: s.set_loss("kld_cc_nss_sim"), dict(saliency=True)),
    "bn_fusion1": (UNET, seq_device_steps, lambda s: s.set_bn_fusion(1), {}),
    "bn_fusion2": (UNET, seq_device_steps, lambda s: s.set_bn_fusion(2), {}),
    "pointwise_fp16": (UNET, seq_device_steps, lambda s: s.set_pointwise_fp16(True), {}),
    "augment": (UNET, seq_host_steps, lambda s: s.set_augment(flip=0.5, reverse=0.5, min_scale=0.7, contrast=0.2, brightness=0.1), {}),
    "unet++ds-gemm": (UNETPP_DS, seq_device_steps, lambda s: s.set_attention_mode("gemm"), {}),
    "unet++ds-flash": (UNETPP_DS, seq_device_steps, lambda s: s.set_attention_mode("flash"), {}),
}


@pytest.mark.parametrize("mode,stream", MODES, ids=_id)
@pytest.mark.parametrize("option", sorted(OPTIONS))
def test_options_are_schedule_invariant(option, mode, stream):
    case, sequence, setup, opts = OPTIONS[option]
    check_invariance(("option", option), case, sequence, mode, stream, setup, opts)


@pytest.mark.parametrize("mode,stream", MODES + [("slow", "comm")], ids=_id)
def test_one_rank_communicator_is_schedule_invariant(mode, stream, monkeypatch):
    """The data-parallel step: buckets of 1 MB on the comm stream (several on this graph), sums of one rank."""
    from sap3d_tensorflow_amd import P3DSession
    monkeypatch.setenv("P3D_BUCKET_MB", "1")
    check_invariance(("comm",), UNET, seq_device_steps, mode, stream, lambda s: s.comm_init(P3DSession.comm_unique_id()))
