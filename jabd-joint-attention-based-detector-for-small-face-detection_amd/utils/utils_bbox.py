"""Box decoding and NMS — drop-in for the reference utils/utils_bbox.py
(decode :29-34, decode_landm :39-46, softer_nms :65-114, diounms :182-258, non_max_suppression
:260-296, retinaface_correct_boxes :9-24) with the device work on the HIP path.

`nms` replaces `torchvision.ops.nms` (same signature and result); the
reference imports it at utils/utils_bbox.py:3.
"""
import math

import numpy as np
import torch

from jabd_amd import ops


def retinaface_correct_boxes(result, input_shape, image_shape):
    """Undo the letterbox (reference :9-24).  A device tensor [n, 15] is corrected
    in place by jabd_correct_boxes_f32; host numpy rows (the reference's own
    contract) keep the numpy bookkeeping."""
    if isinstance(result, torch.Tensor):
        return ops.correct_boxes(result, [int(v) for v in input_shape],
                                 [int(v) for v in image_shape], letterbox=True,
                                 to_pixels=False)
    new_shape = image_shape * np.min(input_shape / image_shape)
    offset = (input_shape - new_shape) / 2. / input_shape
    scale = input_shape / new_shape
    sb = np.array([scale[1], scale[0]] * 2)
    sl = np.array([scale[1], scale[0]] * 5)
    ob = np.array([offset[1], offset[0]] * 2)
    ol = np.array([offset[1], offset[0]] * 5)
    result[:, :4] = (result[:, :4] - ob) * sb
    result[:, 5:] = (result[:, 5:] - ol) * sl
    return result


def decode(loc, priors, variances):
    return ops.decode(loc, priors, variances)


def decode_landm(pre, priors, variances):
    return ops.decode_landm(pre, priors, variances)


def nms(boxes, scores, iou_threshold):
    return ops.nms(boxes, scores, iou_threshold)


def diounms(boxes, scores, overlap=0.5, top_k=200, beta1=1.0):
    """DIoU-NMS on the device (reference :182-258): boxes [N,4], scores [N].
    Returns (keep, count) with the reference's contract: keep is an int64
    tensor of length N, zero past count, and keep[:count] are the kept row
    indices in decreasing-score order (only the top_k best-scored rows are
    candidates).  A pair whose DIoU is NaN keeps both boxes."""
    if boxes.dim() != 2 or boxes.shape[-1] != 4:
        raise ValueError(f"diounms: boxes must be [N,4], got {tuple(boxes.shape)}")
    n = boxes.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=boxes.device), 0
    keep, n_keep = ops.batched_nms(boxes.unsqueeze(0), scores.unsqueeze(0), overlap,
                                   kind="diou", beta1=beta1, top_k=top_k)
    count = int(n_keep[0].item())
    keep = keep[0]
    keep[count:] = 0
    return keep, count


def softer_nms(dets, confidence=None, thresh=0.01, sigma=0.5, ax=None, offset=1.0):
    """Gaussian Soft-NMS on the device (reference :65-114): dets [N, C>=5] rows
    (x1, y1, x2, y2, score, ...).  Each selected row decays the score of every
    later row it overlaps by exp(-IoU^2 / sigma) (IoU with the reference's
    "+offset" of pixel boxes); a decayed score below 0.001 drops its row.
    Returns (rows, keep): rows is a [K, C] device tensor in the reference's
    result order with the decayed score in column 4, keep the int64 original
    row indices of those rows.

    Where this departs from the reference (which cannot run as written):
    * dets is not modified (the reference swaps and rescales it in place);
    * confidence is not permuted: use confidence[keep];
    * keep is the original row index of every result row, not range(K).
    thresh and ax are accepted and ignored, as the reference ignores them."""
    if dets.dim() != 2 or dets.shape[1] < 5:
        raise ValueError(f"softer_nms: dets must be [N, >=5], got {tuple(dets.shape)}")
    det = dets.contiguous()
    keep, keep_scores, n_keep = ops.batched_soft_nms(
        det.unsqueeze(0), det[:, 4].contiguous().unsqueeze(0), sigma=sigma, offset=offset)
    k = int(n_keep[0].item())
    keep = keep[0, :k]
    rows = det[keep]
    rows[:, 4] = keep_scores[0, :k]
    return rows, keep


def bbox_vote(det, thresh=0.4, min_votes=1, max_out=750, offset=1.0):
    """Box voting on the device (ops.box_vote) for one image's rows [N, C>=5]
    (x1, y1, x2, y2, score, ...), a device tensor or a numpy array: the merge
    step of multi-scale / flip testing.  Taking the rows in descending score
    order, each still unmerged row gathers the unmerged rows whose IoU with it
    ("+offset" form: 1 for pixel boxes) is >= thresh; the cluster becomes one
    row with the score-weighted mean box, the best row's score and its other
    columns.  Clusters of fewer than min_votes rows are dropped, at most
    max_out rows returned.  Returns numpy [K, C], or [] when K is 0."""
    if not isinstance(det, torch.Tensor):
        det = torch.from_numpy(np.ascontiguousarray(np.asarray(det, np.float32))).to("cuda")
    if det.dim() != 2 or det.shape[1] < 5:
        raise ValueError(f"bbox_vote: det must be [N, >=5], got {tuple(det.shape)}")
    out, n_out, _, _ = ops.box_vote(det.contiguous().unsqueeze(0), vote_threshold=thresh,
                                    offset=offset, min_votes=min_votes, max_out=max_out)
    k = int(n_out[0].item())
    if k == 0:
        return []
    return out[0, :k].cpu().numpy()


def non_max_suppression(detection, conf_thres=0.5, nms_thres=0.3, nms_kind="greedynms",
                        beta1=1.0, top_k=0, sigma=0.5, soft_offset=0.0):
    """Score filter + NMS (greedy IoU, "diounms", or "softnms") on the device;
    returns numpy [K,15] or [].

    nms_kind "softnms" (alias "softernms"): Gaussian Soft-NMS with `sigma` and
    `soft_offset`; nms_thres and beta1 are ignored, the rows come in the
    Soft-NMS's result order and carry their decayed scores.  soft_offset
    defaults to 0, not softer_nms's pixel +1: the rows here hold normalised
    decode() output, where +1 would make every pair overlap."""
    if detection.dim() != 2 or detection.shape[1] < 5:
        raise ValueError("non_max_suppression expects [N, >=5] rows")
    det = detection.contiguous()
    if ops.is_soft_kind(nms_kind):
        keep, keep_scores, n_keep = ops.batched_soft_nms(
            det.unsqueeze(0), det[:, 4].contiguous().unsqueeze(0), sigma=sigma,
            offset=soft_offset, score_threshold=conf_thres, top_k=top_k)
        k = int(n_keep[0].item())
        if k == 0:
            return []
        rows = det[keep[0, :k]]
        rows[:, 4] = keep_scores[0, :k]
        return rows.cpu().numpy()
    keep, n_keep = ops.batched_nms(det.unsqueeze(0), det[:, 4].contiguous().unsqueeze(0),
                                   nms_thres, score_threshold=conf_thres, kind=nms_kind,
                                   beta1=beta1, top_k=top_k)
    k = int(n_keep[0].item())
    if k == 0:
        return []
    return det[keep[0, :k]].cpu().numpy()
