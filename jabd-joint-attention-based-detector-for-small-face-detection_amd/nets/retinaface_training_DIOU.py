"""The IoU-family MultiBoxLoss variant — drop-in for the reference
nets/retinaface_training_DIOU.py: match_iou (:176-246), decode (:319-337),
bbox_overlaps_iou/giou/diou/ciou (:339-490), IouLoss (:491-522) and the
MultiBoxLoss built on it (:524-665).

Differences from nets/retinaface_training.py, all on the device:
  * match_iou() assigns priors exactly like match() but keeps the matched
    truth corners as loc_t (:230 `loc = matches`), one batched kernel
    (`jabd_match_iou_f32`);
  * the box term is Σ_pos 1 - clamp(overlap(decode(loc, prior), truth)) with
    the overlap IouLoss's losstype names ('Iou', 'Giou', 'Diou', 'Ciou'; the
    reference's MultiBoxLoss hard-wires 'Diou', :541), fused into the loss
    kernel (`jabd_multibox_iou_loss_fwd_f32`) with an analytic backward
    (`jabd_multibox_iou_loss_bwd_f32`).
The CE hard-negative mining, landmark term and normalisation are the base
loss's (:604-665 == nets/retinaface_training.py:238-303).

IouLoss and the bbox_overlaps_* functions on their own run the paired-rows
kernels (`jabd_iou_rows_fwd_f32` / `jabd_iou_rows_bwd_f32`).  Two deliberate
deviations from the reference: a losstype other than the four exact names
raises ValueError (the reference silently treats it as CIoU), and the
overlap functions take paired rows only (no row swap, no broadcasting).
NaN follows the reference arithmetic: under CIoU a prediction bit-equal to
its truth has alpha = 0/0, so its value and gradient are NaN.
"""
import torch
import torch.nn as nn

from jabd_amd import ops
from nets.retinaface_training import (  # noqa: F401  (reference module surface)
    MultiBoxLoss as _BaseMultiBoxLoss, _MultiBoxLossFn, log_sum_exp, match, weights_init)
from utils.utils_bbox import decode  # noqa: F401  (:319-337, the same arithmetic)


def match_iou(threshold, truths, priors, variances, labels, landms, loc_t, conf_t, landm_t, idx):
    """Single-image match_iou() with the reference's in-place output contract (:176-246)."""
    t = torch.cat([truths, landms, labels.reshape(-1, 1)], 1)
    lt, ct, lmt = ops.match_encode([t.to(priors.device).float()], priors, threshold, variances,
                                   raw_loc=True)
    loc_t[idx] = lt[0].to(loc_t.device)
    conf_t[idx] = ct[0].to(conf_t.device)
    landm_t[idx] = lmt[0].to(landm_t.device)


class _IouRowsFn(torch.autograd.Function):
    """val[P] = clamped overlap of pred row i against truth row i; autograd to pred."""

    @staticmethod
    def forward(ctx, pred, truth, priors, variances, kind):
        val = ops.iou_rows(pred, truth, kind, priors, variances)
        ctx.save_for_backward(pred, truth, priors)
        ctx.args = (variances, kind)
        return val

    @staticmethod
    def backward(ctx, gval):
        pred, truth, priors = ctx.saved_tensors
        variances, kind = ctx.args
        gpred = ops.iou_rows_backward(pred, truth, kind, gval.float().contiguous(), priors,
                                      variances)
        return gpred, None, None, None, None


class _FixedSumFn(torch.autograd.Function):
    """Σ x in a fixed order (ops.fixed_sum) as a scalar."""

    @staticmethod
    def forward(ctx, x):
        ctx.n = x.shape[0]
        return ops.fixed_sum(x)[0]

    @staticmethod
    def backward(ctx, g):
        return g.expand(ctx.n)


def _rows(pred, truth, kind, priors=None, variances=(0.1, 0.2)):
    kind = ops.iou_kind(kind)
    if pred.shape[0] != truth.shape[0]:
        raise ValueError(f"paired rows only: {pred.shape[0]} boxes vs {truth.shape[0]} (the "
                         "reference's row swap and broadcasting are not reproduced)")
    if truth.requires_grad or (priors is not None and priors.requires_grad):
        raise ValueError("autograd flows to the first argument only; detach() the others")
    return _IouRowsFn.apply(pred.float().contiguous(), truth.float().contiguous(),
                            None if priors is None else priors.float().contiguous(),
                            tuple(float(v) for v in variances), kind)


def bbox_overlaps_iou(bboxes1, bboxes2):
    """:339-365 for paired rows: clamp(I/U, 0, 1), [P] on the device."""
    return _rows(bboxes1, bboxes2, "Iou")


def bbox_overlaps_giou(bboxes1, bboxes2):
    """:366-401 for paired rows: clamp(I/U - (C - U)/C, -1, 1)."""
    return _rows(bboxes1, bboxes2, "Giou")


def bbox_overlaps_diou(bboxes1, bboxes2):
    """:402-442 for paired rows: clamp(I/U - rho^2/c^2, -1, 1)."""
    return _rows(bboxes1, bboxes2, "Diou")


def bbox_overlaps_ciou(bboxes1, bboxes2):
    """:444-490 for paired rows: clamp(I/U - (rho^2/c^2 + alpha v), -1, 1)."""
    return _rows(bboxes1, bboxes2, "Ciou")


class IouLoss(nn.Module):
    """IouLoss(pred_mode, size_sum, variances, losstype) (:491-522).
    forward(loc_p [P,4], loc_t [P,4], prior_data [P,4]) -> Σ (1 - overlap), a
    scalar (divided by P when size_sum is False; 0 when P == 0).  pred_mode
    'Center': loc_p holds offsets decoded against prior_data; anything else:
    corner boxes.  `loss` (the losstype) is read on every call."""

    def __init__(self, pred_mode="Center", size_sum=True, variances=None, losstype="Diou"):
        super().__init__()
        ops.iou_kind(losstype)
        self.size_sum = size_sum
        self.pred_mode = pred_mode
        self.variances = variances
        self.loss = losstype

    def forward(self, loc_p, loc_t, prior_data=None):
        kind = ops.iou_kind(self.loss)
        num = loc_p.shape[0]
        if num == 0:
            return loc_p.sum()   # the reference's sum over no rows: 0, still on the graph
        if self.pred_mode == "Center":
            if self.variances is None or prior_data is None:
                raise ValueError("IouLoss: pred_mode 'Center' needs variances and prior_data")
            val = _rows(loc_p, loc_t, kind, prior_data, self.variances)
        else:
            val = _rows(loc_p, loc_t, kind)
        loss = _FixedSumFn.apply(1.0 - val)
        return loss if self.size_sum else loss / num


class MultiBoxLoss(_BaseMultiBoxLoss):
    """MultiBoxLoss(num_classes, overlap_thresh, neg_pos, variance, cuda, losstype)
    with the IoU-family box loss (:524-665; the reference fixes losstype at
    'Diou').  forward((loc, conf, landm), priors, targets) ->
    (loss_l, loss_c, loss_landm).  The kind is `self.gious.loss`, read on every
    call, so `criterion.gious.loss = 'Ciou'` switches the fused kernel's kind."""

    def __init__(self, num_classes, overlap_thresh, neg_pos, variance, cuda=True,
                 losstype="Diou"):
        super().__init__(num_classes, overlap_thresh, neg_pos, variance, cuda)
        self.gious = IouLoss("Center", True, self.variance, losstype)

    def forward(self, predictions, priors, targets):
        loc_data, conf_data, landm_data = predictions
        kind = ops.iou_kind(self.gious.loss)
        priors = priors.to(loc_data.device).float().contiguous()
        tg = [t.to(loc_data.device).float() for t in targets]
        with torch.no_grad():
            loc_t, conf_t, landm_t = ops.match_encode(tg, priors, self.threshold, self.variance,
                                                      raw_loc=True)
        return _MultiBoxLossFn.apply(loc_data.contiguous(), conf_data.contiguous(),
                                     landm_data.contiguous(), loc_t, conf_t, landm_t,
                                     int(self.negpos_ratio), self._count_group,
                                     (priors, tuple(float(v) for v in self.variance), kind))
