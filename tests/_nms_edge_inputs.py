"""Seeded numpy inputs for tests/test_nms_grid_edges.py: images that steer
csrc/nms.hip's grid producer and pull scan into the branches ordinary
clustered boxes never reach.  Nothing here touches the device.

Every builder returns (boxes [1,n,4] f32, scores [1,n] f32).  N = 20481 is the
smallest row count that takes the grid producer (nms.hip's dense-rows limit
is 20480).  The rows a builder planted are found again from the data alone
(cluster_rows, far_rows, inactive_rows), so a test needs no side channel.

cluster_incoming() counts, per 64-row block of the rank order, the suppressing
pairs that enter the block from an earlier block: the length of the list the
pull scan receives for that block (a lower bound: only the given rows are
paired).  The ring of nms_scan_pull holds 16384 of them.
"""
import numpy as np

from jabd_amd import synth

N = 20481
RING = 16384          # nms.hip kEntRing
OVF_PER_BOX = 16      # nms.hip kOvfPerBox


def order_desc(scores):
    """Rank order of the pipeline: descending score, stable, NaN first,
    -0.0 == 0.0 (oracle/nms_ref.c's cmp_desc)."""
    s = np.asarray(scores, np.float32).reshape(-1)
    nan = np.isnan(s)
    return np.lexsort((np.arange(len(s)), np.where(nan, np.float32(0), -s), ~nan))


def _background(n, seed):
    b, s = synth.nms_boxes(1, n, seed=seed)
    return b.copy(), s.copy()


def _plant(boxes, scores, rows, new, rank_of_row):
    """new[k] into row rows[k] with the score 2.0 - rank * 1e-4: above every
    background score (< 1), distinct in fp32, so the planted rows hold ranks
    0..M-1 in the order rank_of_row gives."""
    boxes[0, rows] = new.astype(np.float32)
    scores[0, rows] = (2.0 - np.asarray(rank_of_row) * 1e-4).astype(np.float32)


def cluster_rows(scores):
    """The rows chain_cluster / solid_cluster planted (scores above 1.5), in
    rank order."""
    s = np.asarray(scores, np.float32).reshape(-1)
    rows = np.nonzero(s > 1.5)[0]
    return rows[np.argsort(-s[rows], kind="stable")]


def chain_cluster(n=N, M=1024, K=200, thr=0.5, w=0.1, seed=1, p_scale=1.0):
    """M boxes [x0 + p, y0, x0 + p + w, y0 + w] along a line, p = k * step with
    step = p_scale * w (1 - thr) / ((1 + thr) K): box k has IoU > thr with
    about K / p_scale neighbours on each side, so the greedy result inside the
    chain is not trivial (kept rows other than the best one suppress).  Chain
    position k is given to a random rank, ranks 0..M-1."""
    boxes, scores = _background(n, seed + 100)
    rng = np.random.default_rng(seed)
    rows = rng.choice(n, M, replace=False)
    pos = rng.permutation(M)                   # rank r sits at chain position pos[r]
    step = p_scale * w * (1.0 - thr) / ((1.0 + thr) * K)
    x0, y0 = 0.3, 0.6
    p = pos * step
    new = np.stack([x0 + p, np.full(M, y0), x0 + p + w, np.full(M, y0 + w)], 1)
    _plant(boxes, scores, rows, new, np.arange(M))
    return boxes, scores


def solid_cluster(n=N, M=448, seed=2):
    """M near-identical boxes (centre jitter 0.001, size jitter 2 %) at ranks
    0..M-1: every pair of them suppresses at thr 0.5, so block c of the rank
    order receives exactly 64 c * 64 pairs; block 4 exactly fills the ring."""
    boxes, scores = _background(n, seed + 100)
    rng = np.random.default_rng(seed)
    rows = rng.choice(n, M, replace=False)
    ctr = np.array([0.3, 0.6]) + rng.normal(0, 0.001, (M, 2))
    wh = 0.08 * (1 + rng.uniform(0, 0.02, (M, 2)))
    _plant(boxes, scores, rows, np.concatenate([ctr - wh / 2, ctr + wh / 2], 1), np.arange(M))
    return boxes, scores


def far_tiny(n=N, m=32, seed=3):
    """The background plus m disjoint boxes of width 1e-4 near x = y = 50: at
    thr 0.5 their cells are 3.5e-5 wide, cell index about 1.4e6, far beyond the
    grid keys' +-2^14."""
    boxes, scores = _background(n, seed + 100)
    rng = np.random.default_rng(seed)
    rows = rng.choice(n, m, replace=False)
    ctr = 50.0 + 0.01 * np.arange(m)
    boxes[0, rows] = np.stack([ctr - 5e-5, ctr - 5e-5, ctr + 5e-5, ctr + 5e-5], 1).astype(np.float32)
    return boxes, scores


def far_rows(boxes):
    return np.nonzero(np.asarray(boxes).reshape(-1, 4)[:, 0] > 10.0)[0]


def inactive_rows(boxes):
    """Rows the grid producer does not bin (nms.hip grid_active): x2 <= x1,
    y2 <= y1 or an fp32 area that is not finite."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return np.nonzero(~((b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1]) & (area < np.inf)))[0]


def inactive_mix(n=N, frac=0.01, seed=4):
    """The background with frac of the rows each made zero-width, inverted
    (x2 < x1), x2 = +inf, and w = h = 1e20 (the fp32 area overflows to inf).
    None of them can suppress or be suppressed at thr >= 0: every IoU they
    take part in is 0 or NaN."""
    boxes, scores = _background(n, seed + 100)
    rng = np.random.default_rng(seed)
    k = max(int(n * frac), 1)
    rows = rng.choice(n, 4 * k, replace=False)
    b = boxes[0]
    r = rows[:k]
    b[r, 2] = b[r, 0]                                   # zero width
    r = rows[k:2 * k]
    b[r, 0], b[r, 2] = b[r, 2].copy(), b[r, 0].copy()   # inverted
    r = rows[2 * k:3 * k]
    b[r, 2] = np.inf
    r = rows[3 * k:]
    c = (b[r, :2] + b[r, 2:]) / 2
    b[r, :2] = c - np.float32(5e19)
    b[r, 2:] = c + np.float32(5e19)
    return boxes, scores


def all_inactive(n=N, seed=5):
    """Every row zero-area: even rows zero-width, odd rows zero-height."""
    boxes, scores = _background(n, seed + 100)
    b = boxes[0]
    b[0::2, 2] = b[0::2, 0]
    b[1::2, 3] = b[1::2, 1]
    return boxes, scores


def signed_pixels(n=N, smin=1e-3, smax=1e3, seed=6, groups=40, points=4000):
    """Pixel-scale boxes on both sides of the origin: centres uniform in
    [-1024, 1024]^2, extents log-uniform in [smin, smax].  `groups` size
    prototypes (w, h); each of `points` centre points belongs to one prototype
    and every row is a near-duplicate of a point (centre jitter 10 % of the
    extent, extent jitter 5 %), so rows suppress each other at every scale."""
    rng = np.random.default_rng(seed)
    proto = np.exp(rng.uniform(np.log(smin), np.log(smax), (groups, 2)))
    pt_c = rng.uniform(-1024, 1024, (points, 2))
    pt_g = rng.integers(0, groups, points)
    pick = rng.integers(0, points, n)
    wh = proto[pt_g[pick]] * (1 + rng.uniform(-0.05, 0.05, (n, 2)))
    ctr = pt_c[pick] + rng.normal(0, 0.1, (n, 2)) * wh
    boxes = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)[None]
    scores = rng.uniform(0.5, 1.0, (1, n)).astype(np.float32)
    return boxes, scores


def sparse_small(n=N, seed=7, points=2000, wmin=0.002, wmax=0.01):
    """Small boxes (extents log-uniform in [wmin, wmax]) around `points`
    cluster points in [0, 1]^2, centre jitter half an extent: few enough
    overlapping pairs that thr = 0 (every overlapping pair suppresses, one
    size class) stays within the grid producer's pair capacity, and wide
    enough that the 0.05-extent cells of thr >= 1 stay inside +-2^14."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, 1, (points, 2))
    pick = rng.integers(0, points, n)
    wh = np.exp(rng.uniform(np.log(wmin), np.log(wmax), (n, 2)))
    ctr = c[pick] + rng.uniform(-0.5, 0.5, (n, 2)) * wh
    boxes = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)[None]
    scores = rng.uniform(0.5, 1.0, (1, n)).astype(np.float32)
    return boxes, scores


# ----------------------------------------------------------------------------- pair predicate
def suppresses(bi, bj, thr, kind="iou"):
    """bool [len(bi), len(bj)]: box bi[a] (the kept, lower-rank one) suppresses
    bj[c].  fp32, one ufunc per operation: kind "iou" in torchvision's order
    (oracle/nms_ref.c), "diou" in the reference diounms' order
    (tests/_diou_ref.py, beta1 = 1)."""
    f = np.float32
    bi, bj = np.asarray(bi, f).reshape(-1, 4), np.asarray(bj, f).reshape(-1, 4)
    x1i, y1i, x2i, y2i = (bi[:, k][:, None] for k in range(4))
    x1j, y1j, x2j, y2j = (bj[:, k][None, :] for k in range(4))
    with np.errstate(all="ignore"):
        ai = (x2i - x1i) * (y2i - y1i)
        aj = (x2j - x1j) * (y2j - y1j)
        w = np.maximum(np.minimum(x2i, x2j) - np.maximum(x1i, x1j), f(0))
        h = np.maximum(np.minimum(y2i, y2j) - np.maximum(y1i, y1j), f(0))
        inter = w * h
        if kind == "iou":
            val = inter / ((ai + aj) - inter)
        else:
            assert kind == "diou"
            union = (aj - inter) + ai
            dx = (x1i + x2i) / f(2) - (x1j + x2j) / f(2)
            dy = (y1i + y2i) / f(2) - (y1j + y2j) / f(2)
            d = dx * dx + dy * dy
            ex = np.maximum(x2i, x2j) - np.minimum(x1i, x1j)
            ey = np.maximum(y2i, y2j) - np.minimum(y1i, y1j)
            val = inter / union - d / (ex * ex + ey * ey)
        assert val.dtype == f
        return val.astype(np.float64) > float(thr)


def cluster_pairs(boxes, scores, rows, thr, kind="iou"):
    """(rank [M] of the given rows in the whole image's order, ascending;
    S bool [M, M]: S[a, c] = the row of rank[a] suppresses the row of rank[c],
    a < c)."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    order = order_desc(scores)
    rank_of = np.empty(len(order), np.int64)
    rank_of[order] = np.arange(len(order))
    rows = np.asarray(rows)
    rows = rows[np.argsort(rank_of[rows])]
    S = suppresses(b[rows], b[rows], thr, kind)
    return rank_of[rows], np.triu(S, 1)


def cluster_incoming(boxes, scores, rows, thr, kind="iou"):
    """Per 64-row block of the rank order, up to the last block holding one of
    `rows`: the number of suppressing pairs (i, j) among `rows` with
    block(i) < block(j) = that block."""
    rank, S = cluster_pairs(boxes, scores, rows, thr, kind)
    blk = rank >> 6
    off = S & (blk[:, None] < blk[None, :])
    return np.bincount(blk, weights=off.sum(0), minlength=int(blk.max()) + 1).astype(np.int64)
