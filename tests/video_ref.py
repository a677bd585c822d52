"""numpy replay of resident video inference (include/p3d_hip.h, "Resident video inference"): the validation of
p3d_video_predict, the NEWEST and MEAN scatter rules and MEAN's read-out, in np.float32 arithmetic with Python ints for the
counts.  Bit for bit what the kernels of csrc/video.hip must produce."""
import numpy as np

NEWEST, MEAN = 0, 1


class Refused(ValueError):
    pass


def validate(mode, F, T, B, last_start, starts, put=None):
    """Raises Refused as p3d_video_predict refuses; put (or None: every frame counts as put) marks the frames that arrived."""
    if mode not in (NEWEST, MEAN):
        raise Refused("mode")
    if F < T:
        raise Refused("fewer frames than a window")
    n = len(starts)
    if not 1 <= n <= B:
        raise Refused("n_windows")
    prev = last_start
    for k, s in enumerate(starts):
        s = int(s)
        if s < 0 or s > F - T:
            raise Refused("window %d outside [0, F - T]" % k)
        if s <= prev:
            raise Refused("window %d not ascending" % k)
        if put is not None and not all(put[s:s + T]):
            raise Refused("window %d holds a frame never put" % k)
        prev = s


def plan_counts(mode, F, T, B, last_start, count, starts):
    """The counts after one call (the host's authoritative copy)."""
    validate(mode, F, T, B, last_start, starts)
    out = [int(c) for c in count]
    for s in starts:
        for t in range(T):
            f = int(s) + t
            if mode == NEWEST:
                out[f] = 1
            else:
                out[f] += 1
    return out


def scatter(mode, store, count, pred, starts):
    """One call's update, in place: store [F, hw] float32 (maps or sums), count a list of ints, pred [n_windows.., T, hw] float32
    (rows past len(starts) are padding and contribute nothing).  Copies move bits (uint32 views), sums are float32 adds in
    ascending window order."""
    assert store.dtype == np.float32 and pred.dtype == np.float32
    su, pu = store.view(np.uint32), np.ascontiguousarray(pred).view(np.uint32)
    T = pred.shape[1]
    with np.errstate(all="ignore"):
        for k, s in enumerate(starts):
            for t in range(T):
                f = int(s) + t
                if count[f] == 0:
                    su[f] = pu[k, t]
                    count[f] = 1
                elif mode == MEAN:
                    store[f] = store[f] + pred[k, t]          # np.float32 + np.float32: one rounding
                    count[f] += 1
    return store, count


def read_out(mode, store, count):
    """Maps of every frame (count >= 1 each): NEWEST the store; MEAN sum / float32(count), a count of 1 the sum's bits."""
    if mode == NEWEST:
        return store.copy()
    out = store.copy()
    with np.errstate(all="ignore"):
        for f, c in enumerate(count):
            assert c >= 1
            if c != 1:
                out[f] = store[f] / np.float32(c)
    return out


def window_starts(F, T, stride):
    """The driver's windows: 0, stride, 2 stride, ... and a last one at F - T so that every frame is covered."""
    starts = list(range(0, F - T + 1, stride))
    if starts[-1] != F - T:
        starts.append(F - T)
    return starts


def run_video(mode, F, T, batch, starts, predict):
    """The whole driver loop on the host: predict(list of starts, padded to batch with the last one) -> [batch, T, hw] float32.
    Returns (maps [F, hw], counts)."""
    store, count, last = None, [0] * F, -1
    for i in range(0, len(starts), batch):
        chunk = [int(s) for s in starts[i:i + batch]]
        validate(mode, F, T, batch, last, chunk)
        pred = np.asarray(predict(chunk + [chunk[-1]] * (batch - len(chunk))), np.float32)
        pred = pred.reshape(batch, T, -1)
        if store is None:
            store = np.zeros((F, pred.shape[2]), np.float32)
        scatter(mode, store, count, pred, chunk)
        last = chunk[-1]
    return store, count
