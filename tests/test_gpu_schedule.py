"""Scheduler-level test: the stream operations of ONE train step -- launches on the main, side (filter
gradients) and comm (all-reduce) streams, async fills, event records / waits -- as p3d_debug_schedule reports them, checked as a
happens-before graph.  check_generic holds for every structure and option (all seven structures, clipping, both micro-steps of
gradient accumulation); check_unet adds what is designed into p3d_unet's plain step (two adam_kernel launches, the stem overlap)
and check_schedule compares its skeleton with the committed one:

 * every wait names an event that was recorded before it in the same pass;
 * the gradient buffer's zero fill (side stream, beside the forward pass) precedes every launch of the backward pass, on
   every stream;
 * every all-reduce hand-over comes after every launch issued before it on the main and side streams (the gradients of its
   range are final), and Adam comes after every all-reduce;
 * the last optimiser launch comes after EVERY launch of the step, the first after everything but the stem's filter gradient
   (the designed overlap: that part updates every variable but the stem kernel);
 * at the end of the step the main stream has joined the side and comm streams, so whatever the next call enqueues is ordered
   behind all of it;
 * and the synchronisation skeleton (who records, who waits, in which order, around which runs of launches) equals the
   committed one (tests/golden/schedule_unet_*.txt) -- a change of the scheduler has to be looked at and re-recorded:
       P3D_WRITE_SCHEDULE_GOLDEN=gpurun_out/sched python -m pytest tests/test_gpu_schedule.py -m gpu

The ordering bugs this code can have (round 3: a fill that was not ordered against the launch behind it) do not show as wrong
numbers until another session reuses the state; they do show here."""
import os
import re
import sys

import numpy as np
import pytest

from oracle import p3d

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
WRITE_TO = os.environ.get("P3D_WRITE_SCHEDULE_GOLDEN")
NOTES = ("G",)               # lines that annotate the launch behind them (include/p3d_hip.h): not stream operations
# the optimiser's kernel families (elementwise.hip, opt_kernels): <kind>[_decay][_scaled]_kernel
OPTIMISER = re.compile(r"(adam|momentum|sgd)(_decay)?(_scaled)?_kernel\b")


def parse(lines):
    ops = []
    for ln in lines:
        parts = ln.split()
        kind, stream = parts[0], parts[1]
        rest = " ".join(parts[2:])
        if kind not in NOTES:
            ops.append((kind, stream, rest))
    return ops


def happens_before(ops):
    """Vector clocks over the trace: clock[i][s] = number of operations of stream s that are ordered before operation i
    (operation i itself included on its own stream)."""
    streams = sorted({s for _, s, _ in ops})
    cur = {s: {t: 0 for t in streams} for s in streams}          # per stream: what it has seen of every stream
    at_record = {}
    out = []
    for kind, s, rest in ops:
        cur[s][s] += 1
        if kind == "R":
            at_record[rest] = dict(cur[s])
        elif kind == "W":
            assert rest in at_record, "stream %s waits for %s, which no operation of this pass has recorded" % (s, rest)
            for t, v in at_record[rest].items():
                cur[s][t] = max(cur[s][t], v)
        out.append(dict(cur[s]))
    return streams, out


def ordered(i, j, ops, clocks, pos):
    """operation i happens-before operation j"""
    si = ops[i][1]
    return clocks[j][si] >= pos[i]


def skeleton(ops):
    """The synchronisation skeleton: fills, records, waits and all-reduces as they are; every run of launches of one stream
    between them as one line with its length and its first and last kernel."""
    out, run = [], []

    def flush():
        if run:
            first, last = run[0], run[-1]
            out.append("L %s x%d  %s .. %s" % (first[1], len(run), first[2], last[2]))
            run.clear()
    for op in ops:
        if op[0] == "L":
            if run and run[0][1] != op[1]:
                flush()
            run.append(op)
        else:
            flush()
            rest = re.sub(r"allreduce \d+ \d+", "allreduce", op[2])
            out.append("%s %s %s" % (op[0], op[1], rest))
    flush()
    return out


class Trace:
    """A parsed trace with its vector clocks: ops, streams, clocks, pos (1-based position of each operation on its stream),
    count (operations per stream), launches (indices of the "L" lines)."""

    def __init__(self, lines):
        self.ops = parse(lines)
        self.streams, self.clocks = happens_before(self.ops)        # (asserts every wait's event was recorded in this pass)
        self.pos, self.count = [], {s: 0 for s in self.streams}
        for _, s, _ in self.ops:
            self.count[s] += 1
            self.pos.append(self.count[s])
        self.launches = [i for i, op in enumerate(self.ops) if op[0] == "L"]
        self.optimiser = [i for i in self.launches if OPTIMISER.match(self.ops[i][2])]

    def ordered(self, i, j):
        return ordered(i, j, self.ops, self.clocks, self.pos)

    def tag(self, i):
        return self.ops[i][2].rsplit("@", 1)[1] if "@" in self.ops[i][2] else None


def check_generic(lines, with_comm, with_optimiser=True):
    """What every train step must satisfy, whatever the structure and the options: every wait names an event recorded earlier in
    the pass (Trace); the gradient fill precedes every backward launch; every optimiser launch is ordered after the launches it
    must follow -- the last after every launch issued before it, an earlier one after all of them but the side stream's launches
    of the op the walk ended on (its filter gradient, which the early part is designed to overlap); every all-reduce is ordered
    after its producers and ahead of an optimiser launch; the main stream ends joined to every stream."""
    tr = Trace(lines)
    ops, launches = tr.ops, tr.launches
    assert "main" in tr.streams and "side" in tr.streams and launches
    # -- the gradient buffer is zeroed before anything of the backward pass runs, on whichever stream
    fills = [i for i, op in enumerate(ops) if op[0] == "M" and op[2] == "gradients"]
    assert len(fills) == 1
    backward = [i for i in launches if "@" in ops[i][2]]
    assert backward
    for i in backward:
        assert tr.ordered(fills[0], i), ("launch not ordered behind the gradient fill", ops[i])
    # -- the optimiser
    opt = tr.optimiser
    assert bool(opt) == with_optimiser, [ops[i] for i in opt]
    assert all(ops[i][1] == "main" for i in opt)
    # the op the backward walk ended on: the tag of the last launch issued ahead of the first optimiser launch
    ended_on = tr.tag(max(i for i in launches if i < opt[0])) if opt else None
    for k, o in enumerate(opt):
        last = k == len(opt) - 1
        which = "last" if last else "first" if k == 0 else "next"
        for i in launches:
            if i >= o or i in opt:
                continue
            if not last and ops[i][1] == "side" and ended_on is not None and tr.tag(i) == ended_on:
                continue
            assert tr.ordered(i, o), ("the %s optimiser launch does not wait for" % which, ops[i])
    # -- all-reduce hand-overs
    comms = [i for i, op in enumerate(ops) if op[0] == "C"]
    assert bool(comms) == with_comm
    covered = 0
    for c in comms:
        lo, hi = [int(v) for v in ops[c][2].split()[1:3]]
        assert 0 <= lo < hi
        covered += hi - lo
        for i in launches:
            if i < c and ops[i][1] in ("main", "side") and i not in opt:
                assert tr.ordered(i, c), ("all-reduce handed over before", ops[i])
        assert any(tr.ordered(c, a) for a in opt), "no optimiser launch behind this all-reduce"
    if comms:
        los = sorted(int(ops[c][2].split()[1]) for c in comms)
        assert los[0] == 0                                      # the buckets reach the start of the buffer ...
        assert tr.ordered(max(comms), opt[-1])
    # -- the step ends joined: the main stream has seen everything
    last_main = max(i for i, op in enumerate(ops) if op[1] == "main")
    for s in tr.streams:
        assert tr.clocks[last_main][s] == tr.count[s], ("main stream ends the step without having joined", s, tr.clocks[last_main][s], tr.count[s])
    return tr


def check_unet(tr):
    """p3d_unet's plain step on top of check_generic: exactly two adam_kernel launches; the last after EVERY launch of the step,
    the first after everything but the stem's filter gradient, which it is designed to overlap."""
    ops, launches = tr.ops, tr.launches
    assert len(launches) > 100
    adam = [i for i in launches if ops[i][2].startswith("adam_kernel")]
    assert len(adam) == 2 and adam == tr.optimiser and all(ops[i][1] == "main" for i in adam)
    others = [i for i in launches if i not in adam]
    for i in others:
        assert tr.ordered(i, adam[-1]), ("the last optimiser launch does not wait for", ops[i])
        if not (ops[i][1] == "side" and ops[i][2].endswith("@stem/conv")):
            assert tr.ordered(i, adam[0]), ("the first optimiser launch does not wait for", ops[i])
    stem_side = [i for i in launches if ops[i][1] == "side" and ops[i][2].endswith("@stem/conv")]
    assert stem_side and not tr.ordered(stem_side[0], adam[0]), "the designed overlap is gone (or the trace lost its tags)"


def check_schedule(lines, with_comm):
    tr = check_generic(lines, with_comm)
    check_unet(tr)
    return skeleton(tr.ops)


def compare_or_write(name, skel):
    path = os.path.join(HERE, "golden", name)
    if WRITE_TO:
        os.makedirs(WRITE_TO, exist_ok=True)
        with open(os.path.join(WRITE_TO, name), "w") as f:
            f.write("\n".join(skel) + "\n")
        return
    want = open(path).read().splitlines()
    assert skel == want, "\n".join(["the synchronisation skeleton of the step changed (tests/test_gpu_schedule.py):"] +
                                   [a if a == b else "  now: %s\n  was: %s" % (a, b) for a, b in zip(skel, want)][:40] +
                                   ["lengths %d / %d" % (len(skel), len(want))])


@pytest.mark.gpu
@pytest.mark.parametrize("with_comm", [False, True])
def test_train_step_schedule_of_unet(with_comm, monkeypatch):
    from sap3d_tensorflow_amd import P3DSession
    cfg, shape = p3d.NetConfig(base=16, blocks=(1, 1, 2)), (2, 16, 32, 32)
    if with_comm:
        monkeypatch.setenv("P3D_BUCKET_MB", "1")                # several buckets on this small graph
    s = P3DSession('unet', batch=shape[0], frames=shape[1], height=shape[2], width=shape[3], base=cfg.base, blocks=cfg.blocks, seed=1)
    if with_comm:
        s.comm_init(P3DSession.comm_unique_id())                # one rank: the schedule of the data-parallel step, sums of one
    s.upload(p3d.synthetic_clip(0, shape + (3,)), p3d.synthetic_target(3, shape))
    s.train_step_device(0.5, seed=0)                            # scratch buffers sized, plans made
    s.synchronize()
    first = s.schedule(0.5, seed=1)
    again = s.schedule(0.5, seed=2)
    assert first == again                                       # the launch list is static
    skel = check_schedule(first, with_comm)
    compare_or_write("schedule_unet_b16_112%s.txt" % ("_comm" if with_comm else ""), skel)
    assert np.isfinite(s.last_loss())
    s.close()


def _generic_cases():
    from test_gpu_determinism import CASES
    out = [(st, cfg, shape, None) for st, cfg, shape in CASES]
    small = [c for c in CASES if c[0] == "unet"][0]
    return out + [small + ("clip",), small + ("accum",)]


@pytest.mark.gpu
@pytest.mark.parametrize("structure,cfg,shape,option", _generic_cases(),
                         ids=lambda v: v if isinstance(v, str) else "x".join(str(d) for d in v) if isinstance(v, tuple) else None)
def test_train_step_schedule_generic_invariants(structure, cfg, shape, option):
    """check_generic on every structure of test_gpu_determinism.CASES, on p3d_unet under clipping, and on both micro-steps of
    p3d_set_grad_accum(2) (include/p3d_hip.h: the accumulating one launches no optimiser, the applying one the usual tail)."""
    from sap3d_tensorflow_amd import P3DSession
    s = P3DSession(structure, batch=shape[0], frames=shape[1], height=shape[2], width=shape[3], base=cfg.base, blocks=cfg.blocks, seed=1)
    if option == "clip":
        s.set_grad_clip(1.0)
    if option == "accum":
        s.set_grad_accum(2)
    s.upload(p3d.synthetic_clip(0, shape + (3,)), p3d.synthetic_target(3, shape))
    for i in range(2 if option == "accum" else 1):               # scratch buffers sized, plans made; a whole cycle under accumulation
        s.train_step_device(0.5, seed=i)
    s.synchronize()
    if option == "accum":
        assert s.grad_accum == (2, 0)
        first, second = s.schedule(0.5, seed=1), s.schedule(0.5, seed=2)
        assert any(ln.startswith("G main store") for ln in first) and any(ln.startswith("G main finish") for ln in second)
        tr = check_generic(first, False, with_optimiser=False)
        check_generic(second, False)
    else:
        first = s.schedule(0.5, seed=1)
        assert first == s.schedule(0.5, seed=2)                  # the launch list is static
        tr = check_generic(first, False)
        if option == "clip":
            assert any(tr.ops[i][2].startswith("grad_sumsq_kernel") for i in tr.launches)
            assert all("_scaled_kernel" in tr.ops[i][2] for i in tr.optimiser)
    assert len(tr.launches) > 100 and np.isfinite(s.last_loss())
    s.close()


def test_happens_before_machinery_catches_a_missing_join():
    """CPU: the checker itself -- a trace whose optimiser does not wait for the side stream must fail."""
    good = ["R main e0", "W side e0", "M side gradients", "R side e1", "M main loss", "W main e1"] + \
           ["L main k%d" % i for i in range(100)] + ["L main bwd @op"] + \
           ["R main e2", "W side e2", "L side wgrad2 @op", "R main e3", "W side e3", "L side wgrad2 @stem/conv", "R side e4",
            "L main adam_kernel @x", "W main e4", "L main adam_kernel @x"]
    with pytest.raises(AssertionError, match="first optimiser launch does not wait"):
        check_schedule(good, False)          # (the first Adam part must at least wait for the non-stem filter gradient)
    fixed = good[:-6] + ["R side e5", "R main e3", "W side e3", "L side wgrad2 @stem/conv", "R side e4", "W main e5",
                         "L main adam_kernel @x", "W main e4", "L main adam_kernel @x"]
    check_schedule(fixed, False)
    unjoined = fixed[:-2] + ["L main adam_kernel @x"]
    with pytest.raises(AssertionError):
        check_schedule(unjoined, False)
    with pytest.raises(AssertionError, match="no operation of this pass has recorded"):
        check_schedule(["W main e9"] + fixed, False)
    # -- the generic invariants on their own (check_generic): the good trace passes, and one trace per invariant fails
    check_generic(fixed, False)
    with pytest.raises(AssertionError, match="last optimiser launch does not wait"):
        check_generic(unjoined, False)
    trailing = fixed + ["R main e6", "W side e6", "L side late_kernel"]           # work left on the side stream when the step ends
    with pytest.raises(AssertionError, match="without having joined"):
        check_generic(trailing, False)
    check_generic(trailing + ["R side e7", "W main e7"], False)
    with pytest.raises(AssertionError, match="no operation of this pass has recorded"):
        check_generic(["W main e9"] + fixed, False)
    unfilled = [ln for ln in fixed if ln != "W main e1"]                           # the backward starts without the fill's event
    with pytest.raises(AssertionError, match="not ordered behind the gradient fill"):
        check_generic(unfilled, False)
    # every optimiser family is recognised: a Momentum step with decay and clipping that does not wait for a filter gradient
    for kernel in ("momentum_decay_scaled_kernel", "sgd_kernel", "adam_decay_kernel", "sgd_scaled_kernel"):
        check_generic([ln.replace("adam_kernel", kernel) for ln in fixed], False)
        with pytest.raises(AssertionError, match="first optimiser launch does not wait"):
            check_generic([ln.replace("adam_kernel", kernel) for ln in good], False)
    tail = ["L main ema_kernel @x"]                                                # a launch behind the optimiser is no optimiser launch
    assert len(check_generic(fixed + tail, False).optimiser) == 2
    with pytest.raises(AssertionError):                                           # a step that must have an optimiser and has none
        check_generic([ln for ln in fixed if "adam_kernel" not in ln], False)
    check_generic([ln for ln in fixed if "adam_kernel" not in ln], False, with_optimiser=False)
    # all-reduce: handed over behind the main and the side stream's launches, ahead of the optimiser
    body = fixed[:-9]                                                             # ... up to the first side-stream filter gradient
    reduced = body + ["R main e6", "W comm e6", "R side e7", "W comm e7", "C comm allreduce 0 64", "R side e5", "W main e5",
                      "R comm e8", "W main e8", "L main adam_kernel @x"]
    check_generic(reduced, True)
    early = [ln for ln in reduced if ln != "W comm e7"]                            # the bucket's filter gradient is not waited for
    with pytest.raises(AssertionError, match="all-reduce handed over before"):
        check_generic(early, True)
    unread = [ln for ln in reduced if ln != "W main e8"]                           # the optimiser does not wait for the all-reduce
    with pytest.raises(AssertionError):
        check_generic(unread, True)
