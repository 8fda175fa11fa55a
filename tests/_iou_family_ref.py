"""Torch-CPU restatement of the IoU-family box losses of the reference
nets/retinaface_training_DIOU.py: bbox_overlaps_iou/giou/diou/ciou (:339-490)
for paired rows (rows == cols, so the exchange branch never runs), decode
(:319-337) and IouLoss.forward (:491-522).  dtype-generic: runs in fp32 and
fp64, with autograd.  Test-only; the product path is csrc/box_ops.hip."""
import math

import torch

from oracle import box_ref

KINDS = ("Iou", "Giou", "Diou", "Ciou")


def _parts(b1, b2):
    w1 = b1[:, 2] - b1[:, 0]
    h1 = b1[:, 3] - b1[:, 1]
    w2 = b2[:, 2] - b2[:, 0]
    h2 = b2[:, 3] - b2[:, 1]
    inter = torch.clamp(torch.min(b1[:, 2:], b2[:, 2:]) - torch.max(b1[:, :2], b2[:, :2]), min=0)
    outer = torch.clamp(torch.max(b1[:, 2:], b2[:, 2:]) - torch.min(b1[:, :2], b2[:, :2]), min=0)
    inter_area = inter[:, 0] * inter[:, 1]
    union = w1 * h1 + w2 * h2 - inter_area
    return w1, h1, w2, h2, inter_area, outer, union


def _center_term(b1, b2, outer):
    cx1 = (b1[:, 2] + b1[:, 0]) / 2
    cy1 = (b1[:, 3] + b1[:, 1]) / 2
    cx2 = (b2[:, 2] + b2[:, 0]) / 2
    cy2 = (b2[:, 3] + b2[:, 1]) / 2
    inter_diag = (cx2 - cx1) ** 2 + (cy2 - cy1) ** 2
    outer_diag = outer[:, 0] ** 2 + outer[:, 1] ** 2
    return inter_diag / outer_diag


def raw_overlaps(kind, b1, b2):
    """The value before the final clamp, [P]."""
    w1, h1, w2, h2, inter_area, outer, union = _parts(b1, b2)
    if kind == "Iou":                                   # :339-365
        return inter_area / union
    if kind == "Giou":                                  # :366-401
        closure = outer[:, 0] * outer[:, 1]
        return inter_area / union - (closure - union) / closure
    if kind == "Diou":                                  # :402-442
        return inter_area / union - _center_term(b1, b2, outer)
    if kind == "Ciou":                                  # :444-490
        u = _center_term(b1, b2, outer)
        iou = inter_area / union
        v = (4 / (math.pi ** 2)) * torch.pow(torch.atan(w2 / h2) - torch.atan(w1 / h1), 2)
        with torch.no_grad():
            alpha = v / ((1 - iou) + v)
        return iou - (u + alpha * v)
    raise ValueError(f"losstype must be one of {KINDS}, got {kind!r}")


def overlaps(kind, b1, b2):
    """bbox_overlaps_<kind>(b1, b2) for paired rows: the clamped [P] values."""
    if b1.shape[0] != b2.shape[0]:
        raise ValueError(f"paired rows only: {b1.shape[0]} vs {b2.shape[0]}")
    return torch.clamp(raw_overlaps(kind, b1, b2), min=0.0 if kind == "Iou" else -1.0, max=1.0)


def decode(loc, priors, var):
    """:319-337, without the in-place updates (autograd-friendly, same arithmetic)."""
    b = torch.cat((priors[:, :2] + loc[:, :2] * var[0] * priors[:, 2:],
                   priors[:, 2:] * torch.exp(loc[:, 2:] * var[1])), 1)
    b = torch.cat((b[:, :2] - b[:, 2:] / 2, b[:, 2:]), 1)
    return torch.cat((b[:, :2], b[:, 2:] + b[:, :2]), 1)


def iou_loss(kind, loc_p, loc_t, priors=None, var=(0.1, 0.2), pred_mode="Center",
             size_sum=True):
    """IouLoss(pred_mode, size_sum, var, kind).forward(loc_p, loc_t, priors) (:500-522)."""
    b = decode(loc_p, priors, var) if pred_mode == "Center" else loc_p
    loss = torch.sum(1.0 - overlaps(kind, b, loc_t))
    return loss if size_sum else loss / loc_p.shape[0]


def multibox_loss(kind, loc, conf, landm, loc_t, conf_t, landm_t, priors, var=(0.1, 0.2),
                  neg_pos=7, check_regular=False):
    """MultiBoxLoss (:524-665) with IouLoss(losstype=kind) as the box term: this
    file's box term over the positives, the CE and landmark terms and the counts
    from oracle.box_ref.multibox_loss (the terms are independent).
    check_regular: assert that no positive is clamped at -1 and none is NaN."""
    _, loss_c, loss_lm, info = box_ref.multibox_loss(loc, conf, landm, loc_t, conf_t, landm_t,
                                                     neg_pos=neg_pos, diou=(priors, list(var)))
    pos = info["pos"]
    pri_b = priors.to(loc.dtype).unsqueeze(0).expand_as(loc)
    loc_p, truth, pri_p = (loc[pos].view(-1, 4), loc_t[pos].view(-1, 4).to(loc.dtype),
                           pri_b[pos].view(-1, 4))
    if check_regular:
        with torch.no_grad():
            raw = raw_overlaps(kind, decode(loc_p, pri_p, var), truth)
        assert not bool(torch.isnan(raw).any()), "a positive is NaN"
        assert bool((raw > -1.0).all()), "a positive is clamped at -1"
    s_loc = iou_loss(kind, loc_p, truth, pri_p, var)
    n = max(float(info["counts"][0]), 1.0)
    return s_loc / n, loss_c, loss_lm, info


def positives(loc, loc_t, conf_t, priors):
    """The fused loss's positive rows as the rows op sees them:
    (loc_p [P,4], truth [P,4], priors [P,4])."""
    pos = conf_t != 0
    pri_b = priors.unsqueeze(0).expand_as(loc)
    return loc[pos].view(-1, 4), loc_t[pos].view(-1, 4), pri_b[pos].view(-1, 4)
