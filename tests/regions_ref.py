"""A numpy replay of include/p3d_hip.h, "Salient regions of 8-bit maps": a plain union-find per map, the statistics, the
selection, the label map and the link over the frames of a call -- integers only.  Also the maps the GPU tests share."""
import numpy as np

FIELDS = 15
ROOT, AREA, MASS, Y0, X0, Y1, X1, PEAK, PEAK_Y, PEAK_X, CY, CX, ID, PREV, OVERLAP = range(FIELDS)
K_MAX = 64


def root_map(s, gate, conn):
    """int64 [H, W]: every foreground pixel's ROOT (the smallest linear index of its component), -1 for background."""
    H, W = s.shape
    fg = (s >= gate)
    par = list(range(H * W))

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x

    def union(p, q):
        rp, rq = find(p), find(q)
        if rp != rq:
            par[max(rp, rq)] = min(rp, rq)

    rows = fg.tolist()
    for y in range(H):
        for x in range(W):
            if not rows[y][x]:
                continue
            p = y * W + x
            if x > 0 and rows[y][x - 1]:
                union(p, p - 1)
            if y > 0:
                if rows[y - 1][x]:
                    union(p, p - W)
                if conn == 8:
                    if x > 0 and rows[y - 1][x - 1]:
                        union(p, p - W - 1)
                    if x + 1 < W and rows[y - 1][x + 1]:
                        union(p, p - W + 1)
    out = np.full(H * W, -1, np.int64)
    for p in np.flatnonzero(fg.ravel()):
        out[p] = find(int(p))
    return out.reshape(H, W)


def component_stats(s, roots):
    """{ROOT: the twelve statistics of RECORD (ROOT .. CX) as a list of ints} from a map and its root map."""
    H, W = s.shape
    flat, sv = roots.ravel(), s.ravel().astype(np.int64)
    idx = np.flatnonzero(flat >= 0)
    order = idx[np.argsort(flat[idx], kind="stable")]
    res = {}
    if order.size == 0:
        return res
    cuts = np.flatnonzero(np.diff(flat[order])) + 1
    for pix in np.split(order, cuts):
        r = int(flat[pix[0]])
        v, y, x = sv[pix], pix // W, pix % W
        mass, peak = int(v.sum()), int(v.max())
        at = int(pix[v == peak].min())
        sy, sx = int((v * y).sum()), int((v * x).sum())
        res[r] = [r, int(pix.size), mass, int(y.min()), int(x.min()), int(y.max()), int(x.max()), peak, at // W, at % W,
                  (2 * sy + mass) // (2 * mass), (2 * sx + mass) // (2 * mass)]
    return res


def frame_regions(s, gate, conn, min_area, K, roots=None):
    """One frame: (records int64 [K, FIELDS] with ID = PREV = -1 and OVERLAP = 0, counts [3], labels uint8 [H, W])."""
    roots = root_map(s, gate, conn) if roots is None else roots
    st = component_stats(s, roots)
    big = sorted((v for v in st.values() if v[AREA] >= min_area), key=lambda v: (-v[MASS], v[ROOT]))
    kept = big[:K]
    rec = np.full((K, FIELDS), -1, np.int64)
    lab = np.full(s.shape, 255, np.uint8)
    for j, v in enumerate(kept):
        rec[j, :CX + 1] = v
        rec[j, ID], rec[j, PREV], rec[j, OVERLAP] = -1, -1, 0
        lab[roots == v[ROOT]] = j
    return rec, np.array([len(st), len(big), len(kept)], np.int64), lab


def link_frames(rec, counts, labels, shots=None):
    """LINK over the frames of a call, in place on rec [n, K, FIELDS]."""
    n, K = rec.shape[:2]
    starts = {0} | set(int(v) for v in (shots if shots is not None else ()))
    counter = 0
    for f in range(n):
        kept = int(counts[f, 2])
        if f in starts:
            for j in range(kept):
                rec[f, j, ID], rec[f, j, PREV], rec[f, j, OVERLAP] = counter, -1, 0
                counter += 1
            continue
        pk = int(counts[f - 1, 2])
        O = np.zeros((K, K), np.int64)
        both = (labels[f] != 255) & (labels[f - 1] != 255)
        np.add.at(O, (labels[f][both].astype(np.int64), labels[f - 1][both].astype(np.int64)), 1)
        prev = [-1] * kept
        for j in range(kept):
            if pk and O[j, :pk].max() >= 1:
                prev[j] = int(np.argmax(O[j, :pk]))             # the first of the largest: the smallest i
        heir = {}
        for i in set(p for p in prev if p >= 0):
            cand = [j for j in range(kept) if prev[j] == i]
            heir[i] = max(cand, key=lambda j: (O[j, i], -j))
        for j in range(kept):
            i = prev[j]
            if i >= 0 and heir[i] == j:
                rec[f, j, ID] = rec[f - 1, i, ID]
            else:
                rec[f, j, ID] = counter
                counter += 1
            rec[f, j, PREV] = i
            rec[f, j, OVERLAP] = O[j, i] if i >= 0 else 0
    return rec


def regions(sal, gate, conn=8, min_area=1, K=K_MAX, link=False, shots=None):
    """The contract on maps uint8 [n, H, W] -> (regions int32 [n, K, FIELDS], counts int32 [n, 3], labels uint8 [n, H, W])."""
    s3 = sal[None] if sal.ndim == 2 else sal
    out = [frame_regions(s, gate, conn, min_area, K) for s in s3]
    rec = np.stack([o[0] for o in out])
    counts = np.stack([o[1] for o in out])
    labels = np.stack([o[2] for o in out])
    if link:
        link_frames(rec, counts, labels, shots)
    return rec.astype(np.int32), counts.astype(np.int32), labels


# ---- maps ---------------------------------------------------------------------------------------------------------------------
def blobs(n, H, W, seed, count=5, drift=1.5):
    """Gaussian blobs that drift from frame to frame, quantised to bytes (seeded)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    cy, cx = rng.uniform(0, H, count), rng.uniform(0, W, count)
    sg = rng.uniform(1.0, max(1.5, min(H, W) / 8.0), count)
    amp = rng.uniform(120, 255, count)
    vy, vx = rng.uniform(-drift, drift, count), rng.uniform(-drift, drift, count)
    out = np.empty((n, H, W), np.uint8)
    for f in range(n):
        m = np.zeros((H, W))
        for k in range(count):
            m = np.maximum(m, amp[k] * np.exp(-((yy - cy[k] - f * vy[k]) ** 2 + (xx - cx[k] - f * vx[k]) ** 2) / (2 * sg[k] ** 2)))
        out[f] = np.floor(m).astype(np.uint8)
    return out


def checkerboard(H, W, value=200):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where((yy + xx) % 2 == 0, value, 0).astype(np.uint8)


def serpentine(H, W, value=180):
    """Full even rows joined alternately at the right and the left end: one 4-connected path through every column of every row pair."""
    m = np.zeros((H, W), np.uint8)
    m[0::2] = value
    for k, y in enumerate(range(1, H, 2)):
        if y + 1 < H:
            m[y, W - 1 if k % 2 == 0 else 0] = value
    return m


def spiral(H, W, value=220):
    """A one-pixel path that winds inwards from (0, 0) with a one-pixel gap between its turns."""
    g = np.zeros((H, W), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    g[0, 0] = value

    def free(py, px):
        return not (0 <= py < H and 0 <= px < W) or g[py, px] == 0

    while True:
        for _ in range(2):
            ny, nx = y + dy, x + dx
            if 0 <= ny < H and 0 <= nx < W and g[ny, nx] == 0 and free(ny + dy, nx + dx):
                break
            dy, dx = dx, -dy
        else:
            return g
        y, x = ny, nx
        g[y, x] = value


def comb(H, W, value=150):
    """Teeth in every other column that join only in the last row."""
    m = np.zeros((H, W), np.uint8)
    m[:, 0::2] = value
    m[H - 1] = value
    return m


def _row(*spans):
    m = np.zeros((1, 10), np.uint8)
    for a, b, v in spans:
        m[0, a:b] = v
    return m


def merge_split():
    """Five frames of one row: two regions, merged into one, split again (the lighter part overlaps more), nothing, one back."""
    return np.stack([_row((0, 3, 10), (6, 9, 20)), _row((0, 9, 10)), _row((0, 3, 10), (6, 8, 20)), _row(), _row((0, 3, 10))])


# merge_split's [ROOT, ID, PREV, OVERLAP] of its K = 2 slots under link, written out by hand: without a shot table, and with [0, 2]
MERGE_SPLIT_LINK = [[[6, 0, -1, 0], [0, 1, -1, 0]],           # a start: new IDs in rank order, the heavier first
                    [[0, 0, 0, 3], [-1, -1, -1, -1]],         # the merged region overlaps both by 3: the smaller index, its ID
                    [[6, 2, 0, 2], [0, 0, 0, 3]],             # a split: the part that overlaps more is the heir, the other is new
                    [[-1, -1, -1, -1], [-1, -1, -1, -1]],
                    [[0, 3, -1, 0], [-1, -1, -1, -1]]]        # back after a gap: a new ID
MERGE_SPLIT_LINK_SHOTS = [MERGE_SPLIT_LINK[0], MERGE_SPLIT_LINK[1],
                          [[6, 2, -1, 0], [0, 3, -1, 0]],     # a start between two overlapping frames: new IDs, no PREV
                          MERGE_SPLIT_LINK[3], [[0, 4, -1, 0], [-1, -1, -1, -1]]]


def heir_tie():
    """Two frames: a 3 x 4 block, then its first and last row -- equal masses, equal overlaps: rank and heir go to the smaller."""
    a = np.full((3, 4), 10, np.uint8)
    b = a.copy()
    b[1] = 0
    return np.stack([a, b])


HEIR_TIE_LINK = [[0, 0, 0, 4], [8, 1, 0, 4]]                  # frame 1's [ROOT, ID, PREV, OVERLAP]


def ring_island(H, W):
    """A ring (200) whose top-left and bottom-right corner pixels are missing, so that its two halves touch only diagonally, around
    an island (90) it does not touch: two components under c = 8, three under c = 4."""
    m = np.zeros((H, W), np.uint8)
    m[1, 2:W - 1] = 200
    m[1:H - 2, W - 2] = 200
    m[H - 2, 1:W - 2] = 200
    m[2:H - 1, 1] = 200
    m[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = 90
    return m
