"""CPU restatement of the box-voting rule (jabd_box_vote_f32 in include/jabd.h)
and of the un-mirror of jabd_tta_collect_f32, for tests/test_box_vote.py,
tests/test_tta_collect.py and tests/test_predict_tta.py.

    order = candidates (row < n_valid, score >= threshold; a NaN score fails)
            by descending score, stable
    for seed in order, if alive:
        o_j     = IoU(seed, j), alive j        fp32, "+offset" form
        members = { j alive : o_j >= float32(thresh) } + { seed }
        alive  -= members
        if |members| >= min_votes:
            box = float32(sum score_j * coord_j / sum score_j)     in float64
            emit (box, seed's score, seed's columns 5..)
    result: the first max_out emitted rows

The IoU is the text of _softnms_ref.iou_matrix (every fp32 operation rounded
on its own), evaluated for one seed against the alive rows instead of all
pairs, so that a few thousand rows need no n x n matrices.
"""
import numpy as np


def iou_row(seed_box, boxes, offset):
    """fp32 [n]: IoU of one box with each of `boxes`, the operations and their
    order as in _softnms_ref.iou_matrix."""
    a = np.asarray(seed_box, np.float32)
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    off = np.float32(offset)
    zero = np.float32(0)
    x1, y1, x2, y2 = (b[:, k] for k in range(4))
    with np.errstate(all="ignore"):
        area = ((x2 - x1) + off) * ((y2 - y1) + off)
        area_a = ((a[2] - a[0]) + off) * ((a[3] - a[1]) + off)
        w = np.maximum(zero, (np.minimum(a[2], x2) - np.maximum(a[0], x1)) + off)
        h = np.maximum(zero, (np.minimum(a[3], y2) - np.maximum(a[1], y1)) + off)
        inter = w * h
        o = inter / ((area_a + area) - inter)
    assert o.dtype == np.float32
    return o


def vote(rows, thresh=0.4, offset=1.0, score_threshold=-np.inf, min_votes=1, max_out=0,
         n_valid=None, member_order=None):
    """One image's rows [n, C>=5] -> dict with
      rows   float32 [K, C]  the result rows
      seeds  int64 [K]       the input row of each result row's seed
      votes  int32 [K]       its member count
      owner  int32 [n]       the result row each input row joined, or -1
      margin float           the smallest |IoU - thresh| that was decided
    member_order: a numpy Generator; the members are then summed in a random
    order (the sums are float64: the rounded box must not depend on it)."""
    r = np.asarray(rows, np.float32)
    n, C = r.shape
    s = r[:, 4]
    nv = n if n_valid is None else max(0, min(n, int(n_valid)))
    with np.errstate(invalid="ignore"):
        cand = np.nonzero((np.arange(n) < nv) & (s >= np.float32(score_threshold)))[0]
    order = cand[np.argsort(-s[cand].astype(np.float64), kind="stable")]
    thr = np.float32(thresh)
    alive = np.zeros(n, bool)
    alive[cand] = True
    owner = np.full(n, -1, np.int32)
    out, seeds, votes = [], [], []
    margin = np.inf
    for sd in order:
        if not alive[sd]:
            continue
        idx = np.nonzero(alive)[0]
        o = iou_row(r[sd, :4], r[idx, :4], offset)
        with np.errstate(invalid="ignore"):
            mem = o >= thr                     # a NaN overlap is no member
        others = (idx != sd) & ~np.isnan(o)
        if others.any():
            margin = min(margin, float(np.abs(o[others].astype(np.float64) - float(thr)).min()))
        mem |= idx == sd
        members = idx[mem]
        alive[members] = False
        if len(members) < min_votes:
            continue
        if max_out > 0 and len(out) >= max_out:
            continue                           # cut: its members own nothing
        if member_order is not None:
            members = member_order.permutation(members)
        w = s[members].astype(np.float64)
        with np.errstate(all="ignore"):
            box = ((w[:, None] * r[members, :4].astype(np.float64)).sum(0) / w.sum())
        row = r[sd].copy()
        row[:4] = box.astype(np.float32)
        owner[members] = len(out)
        out.append(row)
        seeds.append(int(sd))
        votes.append(len(members))
    return {"rows": np.asarray(out, np.float32).reshape(-1, C),
            "seeds": np.asarray(seeds, np.int64), "votes": np.asarray(votes, np.int32),
            "owner": owner, "margin": margin}


def unmirror(rows):
    """Detect rows [n, 15] of a pass on the mirrored canvas, in normalised
    canvas coordinates -> the rows of the unmirrored canvas: x -> 1 - x in
    fp32, x1 and x2 exchanged, landmark pairs 0 <-> 1 and 3 <-> 4 exchanged."""
    r = np.asarray(rows, np.float32)
    one = np.float32(1)
    out = r.copy()
    out[:, 0] = one - r[:, 2]
    out[:, 2] = one - r[:, 0]
    lm = r[:, 5:].reshape(-1, 5, 2)[:, [1, 0, 2, 4, 3]].copy()
    lm[:, :, 0] = one - lm[:, :, 0]
    out[:, 5:] = lm.reshape(-1, 10)
    return out


def ulp_diff(a, b):
    """Distance in fp32 units in the last place, elementwise (equal NaNs: 0)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)

    def lin(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    d = np.abs(lin(a) - lin(b))
    both_nan = np.isnan(a) & np.isnan(b)
    one_nan = np.isnan(a) ^ np.isnan(b)
    return np.where(both_nan, 0, np.where(one_nan, np.int64(1) << 40, d))
