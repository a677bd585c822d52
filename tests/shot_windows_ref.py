"""numpy replay of include/p3d_hip.h's "Shot-aware windows" (p3d_video_predict_shots), written from that text alone on top of
shots_ref.refl / shot_of and video_ref: LEGAL as a validation, SLOTS and LIVE per window, the counts of a call, the scatter of the live
slots only, the driver's window law, and the whole loop on the host.  Integers compare exactly, maps bit for bit."""
import numpy as np

import shots_ref
import video_ref as vr
from video_ref import MEAN, NEWEST, Refused      # noqa: F401

EXAMPLE_F, EXAMPLE_TABLE = 41, [0, 20, 25, 26, 28]      # the header's example: shots of 20, 5, 1, 2, 13 frames


def check_table(table, F):
    table = [int(s) for s in table]
    if not table or table[0] != 0 or any(b <= a for a, b in zip(table, table[1:])) or table[-1] >= F:
        raise Refused("shot table")
    return table


def window(table, F, T, s):
    """(frames read by slots 0 .. T - 1, live) of the window that starts at s."""
    lo, hi = shots_ref.shot_of(table, F, s)
    L = hi - lo + 1
    return [lo + shots_ref.refl(s - lo + t, L) for t in range(T)], min(T, hi - s + 1)


def validate(mode, F, T, B, last_start, table, starts, put=None):
    """Raises Refused as p3d_video_predict_shots refuses, in the header's order."""
    if mode not in (NEWEST, MEAN):
        raise Refused("mode")
    if F < T:
        raise Refused("fewer frames than a window")
    table = check_table(table, F)
    if not 1 <= len(starts) <= B:
        raise Refused("n_windows")
    prev = last_start
    for k, s in enumerate(starts):
        s = int(s)
        if s < 0 or s > F - 1:
            raise Refused("window %d outside [0, F - 1]" % k)
        if s <= prev:
            raise Refused("window %d not ascending" % k)
        lo, hi = shots_ref.shot_of(table, F, s)
        if s != lo and s + T - 1 > hi:
            raise Refused("window %d is neither at the first frame of [%d, %d] nor T - 1 frames from its end" % (k, lo, hi))
        if put is not None:
            for g in window(table, F, T, s)[0]:
                if not put[g]:
                    raise Refused("window %d reads frame %d, never put" % (k, g))
        prev = s


def slots(table, F, T, B, starts):
    """(slots [B, T], live [B]) of one legal call: the padding clips repeat the last window's row and have live 0."""
    rows = [window(table, F, T, int(s)) for s in starts]
    g = [r[0] for r in rows] + [rows[-1][0]] * (B - len(rows))
    return np.array(g, np.int64).reshape(B, T), [r[1] for r in rows] + [0] * (B - len(rows))


def plan_counts(mode, F, T, B, last_start, count, table, starts):
    """The counts after one call."""
    validate(mode, F, T, B, last_start, table, starts)
    out = [int(c) for c in count]
    _, live = slots(table, F, T, B, starts)
    for k, s in enumerate(starts):
        for t in range(live[k]):
            f = int(s) + t
            out[f] = 1 if mode == NEWEST else out[f] + 1
    return out


def scatter(mode, store, count, pred, starts, live):
    """video_ref.scatter over the live slots only: store [F, hw] float32 and count (a list) in place; pred [>= len(starts), T, hw]."""
    assert store.dtype == np.float32 and pred.dtype == np.float32
    su, pu = store.view(np.uint32), np.ascontiguousarray(pred).view(np.uint32)
    with np.errstate(all="ignore"):
        for k, s in enumerate(starts):
            for t in range(live[k]):
                f = int(s) + t
                if count[f] == 0:
                    su[f] = pu[k, t]
                    count[f] = 1
                elif mode == MEAN:
                    store[f] = store[f] + pred[k, t]
                    count[f] += 1
    return store, count


def window_starts(table, F, stride, T=16):
    """The driver's law: per shot [lo] if it is shorter than T, else lo + 0, stride, 2 stride, ... and a last one at L - T."""
    table = check_table(table, F)
    out = []
    for lo, end in zip(table, table[1:] + [F]):
        L = end - lo
        if L < T:
            out.append(lo)
        else:
            out.extend(lo + o for o in vr.window_starts(L, T, stride))
    return out


def run_video(mode, F, T, batch, table, starts, predict):
    """The whole loop on the host: predict(frames [batch, T], the reflected windows padded with the last one) -> [batch, T, hw] float32.
    Returns (maps or sums [F, hw], counts)."""
    store, count, last = None, [0] * F, -1
    for i in range(0, len(starts), batch):
        chunk = [int(s) for s in starts[i:i + batch]]
        validate(mode, F, T, batch, last, table, chunk)
        g, live = slots(table, F, T, batch, chunk)
        pred = np.asarray(predict(g), np.float32).reshape(batch, T, -1)
        if store is None:
            store = np.zeros((F, pred.shape[2]), np.float32)
        scatter(mode, store, count, pred, chunk, live)
        last = chunk[-1]
    return store, count
