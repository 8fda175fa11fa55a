"""Tensor-level wrappers over the libjabd C-ABI (box ops, NMS, match, loss).

Each wrapper validates device/dtype/shape, allocates outputs and workspace
through torch's caching allocator, and launches on torch's current HIP
stream.  CPU tensors are rejected: there is no CPU fallback on the product
path (the CPU restatement lives in oracle/ and is test-only).
"""
import math

import numpy as np
import torch

from ._lib import call, c_size, lib
import ctypes


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _dev(name, t, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: the JABD HIP path needs a GPU tensor (got {t.device}); "
                           "there is no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t.contiguous()


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


def _size_query(fn, *args):
    out = c_size(0)
    call(fn, *args, ctypes.byref(out))
    return out.value


# --------------------------------------------------------------------------- decode
def decode(loc, priors, variances):
    """utils/utils_bbox.py:29-34 — loc [A,4] or [B,A,4] -> corner boxes."""
    loc = _dev("decode.loc", loc)
    priors = _dev("decode.priors", priors)
    A = priors.shape[0]
    if loc.shape[-2:] != (A, 4):
        raise ValueError(f"decode: loc {tuple(loc.shape)} vs priors {tuple(priors.shape)}")
    B = loc.numel() // (A * 4) if A else 0
    out = torch.empty_like(loc)
    call("jabd_decode_f32", _p(loc), _p(priors), B, A, float(variances[0]), float(variances[1]),
         _p(out), _stream())
    return out


def decode_landm(pre, priors, variances):
    """utils/utils_bbox.py:39-46 — pre [A,10] or [B,A,10]."""
    pre = _dev("decode_landm.pre", pre)
    priors = _dev("decode_landm.priors", priors)
    A = priors.shape[0]
    if pre.shape[-2:] != (A, 10):
        raise ValueError(f"decode_landm: pre {tuple(pre.shape)} vs priors {tuple(priors.shape)}")
    B = pre.numel() // (A * 10) if A else 0
    out = torch.empty_like(pre)
    call("jabd_decode_landm_f32", _p(pre), _p(priors), B, A, float(variances[0]), _p(out),
         _stream())
    return out


# --------------------------------------------------------------------------- NMS
_NMS_KINDS = {"iou": 0, "greedynms": 0, "diou": 1, "diounms": 1}


def _kind_code(kind, beta1=1.0):
    """The C-ABI kind (0 = IoU, 1 = DIoU) of a rule name: "iou"/"greedynms" or
    "diou"/"diounms" (the reference's nms_kind names, utils/utils_bbox.py:309).
    The DIoU rule needs a positive finite beta1."""
    try:
        k = _NMS_KINDS[kind]
    except (KeyError, TypeError):
        raise ValueError(f"nms kind must be one of {sorted(_NMS_KINDS)}, got {kind!r}") from None
    if k == 1 and not (float(beta1) > 0.0 and math.isfinite(float(beta1))):
        raise ValueError(f"nms: beta1 must be positive and finite, got {beta1!r}")
    return k


def _nms_call(k, beta1, top_k, *args):
    """jabd_batched_nms_f32 for the default rule, its _ex form otherwise."""
    if k == 0 and int(top_k) <= 0:
        call("jabd_batched_nms_f32", *args)
    else:
        call("jabd_batched_nms_ex_f32", *args, k, float(beta1), int(top_k))


def batched_nms(boxes, scores, iou_threshold, score_threshold=-math.inf, n_valid=None,
                kind="iou", beta1=1.0, top_k=0):
    """Independent greedy NMS per image.

    boxes [B,N,4] (or a [B,N,>=5] row tensor whose first 4 columns are boxes),
    scores [B,N].  Returns (keep [B,N] int64, n_keep [B] int64), both on the
    device; keep[b,:n_keep[b]] are row indices in decreasing-score order.
    kind "iou"/"greedynms": suppress when IoU > iou_threshold; "diou"/"diounms":
    when IoU - (d/c)^beta1 > iou_threshold (the reference's diounms).  top_k > 0
    keeps only each image's top_k best-scored candidates before suppression.
    """
    k = _kind_code(kind, beta1)
    if boxes.dim() != 3 or boxes.shape[-1] < 4:
        raise ValueError(f"batched_nms: boxes must be [B,N,>=4], got {tuple(boxes.shape)}")
    boxes = _dev("nms.boxes", boxes)
    scores = _dev("nms.scores", scores)
    B, N = boxes.shape[0], boxes.shape[1]
    if scores.shape != (B, N):
        raise ValueError(f"batched_nms: scores {tuple(scores.shape)} != {(B, N)}")
    dev = boxes.device
    keep = torch.empty((B, N), dtype=torch.int64, device=dev)
    n_keep = torch.zeros((B,), dtype=torch.int64, device=dev)
    if n_valid is not None:
        n_valid = _dev("nms.n_valid", n_valid, torch.int64)
    ws = _ws(_size_query("jabd_nms_workspace_size", B, N), dev)
    C = boxes.shape[-1]
    _nms_call(k, beta1, top_k, _p(boxes), C, N * C, _p(scores), 1, N, _p(n_valid), B, N,
              float(iou_threshold), float(score_threshold), _p(keep), _p(n_keep), _p(ws),
              ws.numel(), _stream())
    return keep, n_keep


def batched_nms_stats(boxes, scores, iou_threshold, score_threshold=-math.inf, n_valid=None,
                      kind="iou", beta1=1.0, top_k=0, return_flags=False):
    """batched_nms (same arguments, same C call) plus per-image measurement
    counters: (keep, n_keep, tested int64[B], dense bool[B]) where `tested` is
    the number of exact fp32 IoU (or DIoU) evaluations the mask producer made
    (grid: its candidate pairs; dense: every pair).  return_flags: the fourth
    result is the producer word itself, int32[B] (0 = grid; the bits are listed
    at jabd_nms_pair_stats in include/jabd.h) instead of `word != 0`.  Raises
    if the pull scan's staging hand-off timed out.  Synchronises (measurement
    only); B <= 254."""
    k = _kind_code(kind, beta1)
    if boxes.dim() != 3 or boxes.shape[-1] < 4:
        raise ValueError(f"batched_nms_stats: boxes must be [B,N,>=4], got {tuple(boxes.shape)}")
    B, N = boxes.shape[0], boxes.shape[1]
    dev = boxes.device
    boxes = _dev("nms.boxes", boxes)
    scores = _dev("nms.scores", scores)
    if scores.shape != (B, N):
        raise ValueError(f"batched_nms_stats: scores {tuple(scores.shape)} != {(B, N)}")
    keep = torch.empty((B, N), dtype=torch.int64, device=dev)
    n_keep = torch.zeros((B,), dtype=torch.int64, device=dev)
    if n_valid is not None:
        n_valid = _dev("nms.n_valid", n_valid, torch.int64)
    ws = _ws(_size_query("jabd_nms_workspace_size", B, N), dev)
    C = boxes.shape[-1]
    _nms_call(k, beta1, top_k, _p(boxes), C, N * C, _p(scores), 1, N, _p(n_valid), B, N,
              float(iou_threshold), float(score_threshold), _p(keep), _p(n_keep), _p(ws),
              ws.numel(), _stream())
    tested = np.zeros(B, np.int64)
    hits = np.zeros(B, np.int32)
    dense = np.zeros(B, np.int32)
    call("jabd_nms_pair_stats", _p(ws), ws.numel(), B, N, tested.ctypes.data, hits.ctypes.data,
         dense.ctypes.data, _stream())
    tested = np.where(dense != 0, N * (N - 1) // 2, tested)
    return keep, n_keep, tested, dense if return_flags else dense != 0


def nms(boxes, scores, iou_threshold):
    """torchvision.ops.nms(boxes[N,4], scores[N], iou_threshold) -> int64[K].

    Returns a device tensor; reading K synchronises the stream once.
    """
    if boxes.dim() != 2 or boxes.shape[-1] != 4:
        raise ValueError(f"nms: boxes must be [N,4], got {tuple(boxes.shape)}")
    keep, n_keep = batched_nms(boxes.unsqueeze(0), scores.unsqueeze(0), iou_threshold)
    return keep[0, : int(n_keep[0].item())]


# --------------------------------------------------------------------------- Soft-NMS
_SOFT_KINDS = ("softnms", "softernms")
SOFT_PRUNE = 0.001   # the reference's literal (utils/utils_bbox.py:104)


def is_soft_kind(kind):
    """True for the Gaussian Soft-NMS names ("softnms", "softernms"): the kind
    of detect / non_max_suppression / detect_image that runs batched_soft_nms.
    batched_nms and batched_nms_stats return index lists only and have no such
    kind (their _kind_code rejects the names)."""
    return isinstance(kind, str) and kind in _SOFT_KINDS


def _soft_args(sigma, offset, prune=SOFT_PRUNE):
    sigma, offset, prune = float(sigma), float(offset), float(prune)
    if not (sigma > 0.0 and math.isfinite(sigma)):
        raise ValueError(f"soft nms: sigma must be positive and finite, got {sigma!r}")
    if not math.isfinite(offset):
        raise ValueError(f"soft nms: offset must be finite, got {offset!r}")
    if not math.isfinite(prune):
        raise ValueError(f"soft nms: prune must be finite, got {prune!r}")
    return sigma, offset


def batched_soft_nms(boxes, scores, sigma=0.5, offset=1.0, score_threshold=-math.inf,
                     prune=SOFT_PRUNE, n_valid=None, top_k=0):
    """Gaussian Soft-NMS per image (the reference's softer_nms, utils/
    utils_bbox.py:65-114; semantics: jabd_batched_soft_nms_f32 in jabd.h).

    boxes [B,N,4] (or a [B,N,>=5] row tensor whose first 4 columns are boxes),
    scores [B,N]; neither is modified.  Returns (keep [B,N] int64, keep_scores
    [B,N] float32, n_keep [B] int64) on the device: keep[b,:n_keep[b]] are the
    original row indices in the reference's result order (its swaps included)
    and keep_scores their decayed scores.  A selected box decays every later
    overlapping score by exp(-IoU^2 / sigma); a decayed score below `prune`
    drops its row.  offset: the reference's +1 of pixel boxes (pass 0 for
    normalised boxes).  Candidates: rows < n_valid[b] with score >=
    score_threshold (NaN scores are dropped); top_k > 0 keeps the top_k best.
    """
    sigma, offset = _soft_args(sigma, offset, prune)
    if boxes.dim() != 3 or boxes.shape[-1] < 4:
        raise ValueError(f"batched_soft_nms: boxes must be [B,N,>=4], got {tuple(boxes.shape)}")
    boxes = _dev("soft_nms.boxes", boxes)
    scores = _dev("soft_nms.scores", scores)
    B, N = boxes.shape[0], boxes.shape[1]
    if scores.shape != (B, N):
        raise ValueError(f"batched_soft_nms: scores {tuple(scores.shape)} != {(B, N)}")
    dev = boxes.device
    keep = torch.empty((B, N), dtype=torch.int64, device=dev)
    keep_scores = torch.empty((B, N), dtype=torch.float32, device=dev)
    n_keep = torch.zeros((B,), dtype=torch.int64, device=dev)
    if n_valid is not None:
        n_valid = _dev("soft_nms.n_valid", n_valid, torch.int64)
    ws = _ws(_size_query("jabd_soft_nms_workspace_size", B, N), dev)
    C = boxes.shape[-1]
    call("jabd_batched_soft_nms_f32", _p(boxes), C, N * C, _p(scores), 1, N, _p(n_valid), B, N,
         sigma, offset, float(prune), float(score_threshold), int(top_k), _p(keep),
         _p(keep_scores), _p(n_keep), _p(ws), ws.numel(), _stream())
    return keep, keep_scores, n_keep


# --------------------------------------------------------------------------- box voting
def _vote_args(vote_threshold, offset, min_votes, cols=5):
    vote_threshold, offset, min_votes = float(vote_threshold), float(offset), int(min_votes)
    if math.isnan(vote_threshold):
        raise ValueError("box_vote: vote_threshold is NaN")
    if not math.isfinite(offset):
        raise ValueError(f"box_vote: offset must be finite, got {offset!r}")
    if min_votes < 1:
        raise ValueError(f"box_vote: min_votes must be at least 1, got {min_votes!r}")
    if cols < 5:
        raise ValueError(f"box_vote: rows need at least 5 columns, got {cols}")
    return vote_threshold, offset, min_votes


def box_vote(rows, vote_threshold=0.4, offset=1.0, score_threshold=-math.inf, min_votes=1,
             max_out=750, n_valid=None, return_owner=False):
    """Box voting per image (semantics: jabd_box_vote_f32 in jabd.h): each
    cluster of boxes whose IoU with the cluster's best-scored box (the seed) is
    >= vote_threshold becomes one row with the score-weighted mean box, the
    seed's score and the seed's other columns.

    rows [B, N, C>=5] device float32 (x1, y1, x2, y2, score, ...), not
    modified.  Returns (out [B,N,C], n_out [B] int64, seed [B,N] int64, votes
    [B,N] int32[, owner [B,N] int32]) on the device: out[b,:n_out[b]] are the
    result rows in seed order (descending score), seed their seeds' input row
    indices, votes their member counts, owner the result row each input row
    joined (-1: none).  Clusters of fewer than min_votes members are dropped;
    at most max_out rows are returned (max_out <= 0: no cap).  offset: 1 for
    pixel boxes, 0 for normalised ones.  Candidates: rows < n_valid[b] with
    score >= score_threshold (NaN scores are dropped).
    """
    if not isinstance(rows, torch.Tensor) or rows.dim() != 3:
        raise ValueError("box_vote: rows must be a [B, N, >=5] tensor")
    vote_threshold, offset, min_votes = _vote_args(vote_threshold, offset, min_votes,
                                                   rows.shape[-1])
    B, N, C = rows.shape
    if N >= 1 << 24:
        raise ValueError(f"box_vote: N={N} exceeds 2^24 rows per image")
    rows = _dev("box_vote.rows", rows)
    dev = rows.device
    out = torch.empty((B, N, C), dtype=torch.float32, device=dev)
    n_out = torch.empty((B,), dtype=torch.int64, device=dev)   # written by every call
    seed = torch.empty((B, N), dtype=torch.int64, device=dev)
    votes = torch.empty((B, N), dtype=torch.int32, device=dev)
    owner = torch.empty((B, N), dtype=torch.int32, device=dev) if return_owner else None
    if n_valid is not None:
        n_valid = _dev("box_vote.n_valid", n_valid, torch.int64)
        if n_valid.numel() != B:
            raise ValueError(f"box_vote: n_valid has {n_valid.numel()} entries for {B} images")
    ws = _ws(_size_query("jabd_box_vote_workspace_size", B, N), dev)
    call("jabd_box_vote_f32", _p(rows), C, N * C, C, _p(n_valid), B, N, vote_threshold, offset,
         float(score_threshold), min_votes, int(max_out), _p(out), _p(n_out), _p(seed),
         _p(votes), _p(owner), _p(ws), ws.numel(), _stream())
    return (out, n_out, seed, votes, owner) if return_owner else (out, n_out, seed, votes)


def tta_collect(rows, n_keep, merged, offsets, pass_index, input_shape, image_shape,
                letterbox=True, flip=False):
    """One pass of a multi-scale / flip detection joins `merged` on the device
    (jabd_tta_collect_f32): the first n_keep[0] of the pass's detect rows
    [n_max, 15], un-mirrored if `flip` (the pass ran on the mirrored canvas),
    corrected to image pixels as correct_boxes(..., letterbox, to_pixels=True),
    are written from merged[offsets[pass_index]] on, and offsets[pass_index+1]
    = min(offsets[pass_index] + n_keep[0], len(merged)).  Rows beyond the
    capacity of merged [cap, 15] are dropped.  offsets: device int64 of at
    least pass_index + 2 entries, offsets[0] set by the caller.  input_shape =
    (H, W) of the network input, image_shape = (im_height, im_width).  No
    host synchronisation.  Returns merged."""
    rows = _dev("tta_collect.rows", rows)
    n_keep = _dev("tta_collect.n_keep", n_keep, torch.int64)
    if rows.dim() != 2 or rows.shape[1] != 15:
        raise ValueError(f"tta_collect: rows must be [n, 15], got {tuple(rows.shape)}")
    for name, t, dt in (("merged", merged, torch.float32), ("offsets", offsets, torch.int64)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt
                and t.is_contiguous()):
            raise ValueError(f"tta_collect: {name} must be a contiguous device {dt} tensor")
    if merged.dim() != 2 or merged.shape[1] != 15:
        raise ValueError(f"tta_collect: merged must be [cap, 15], got {tuple(merged.shape)}")
    p = int(pass_index)
    if p < 0 or offsets.dim() != 1 or offsets.numel() < p + 2 or n_keep.numel() < 1:
        raise ValueError("tta_collect: offsets needs pass_index + 2 entries, n_keep one")
    call("jabd_tta_collect_f32", _p(rows), _p(n_keep), rows.shape[0], _p(merged),
         merged.shape[0], _p(offsets), p, int(input_shape[0]), int(input_shape[1]),
         int(image_shape[0]), int(image_shape[1]), 1 if letterbox else 0, 1 if flip else 0,
         _stream())
    return merged


# --------------------------------------------------------------------------- tiled detection
def _tile_origins(name, origins):
    origins = _dev(name + ".origins", origins, torch.int32)
    if origins.dim() != 2 or origins.shape[1] != 2:
        raise ValueError(f"{name}: origins must be int32 [n_tiles, 2], got "
                         f"{tuple(origins.shape)}")
    return origins


def tile_gather(image, origins, tile, fill=84.0, mean=(104.0, 117.0, 123.0)):
    """The tile batch of an image (jabd_tile_gather_f32): image device HWC
    [ih, iw, 3], float32 or uint8; origins device int32 [T, 2] = (y0, x0), which
    may be negative or reach past the image; tile = (tile_h, tile_w).  Returns
    float32 [T, 3, tile_h, tile_w] with out[t, c, y, x] = P - mean[c], P the
    image's pixel (y0 + y, x0 + x) or `fill` outside the image."""
    if not isinstance(image, torch.Tensor) or image.dtype not in (torch.float32, torch.uint8):
        raise TypeError("tile_gather: image must be a float32 or uint8 tensor")
    image = _dev("tile_gather.image", image, image.dtype)
    if image.dim() != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError(f"tile_gather: image must be [ih, iw, 3], got {tuple(image.shape)}")
    origins = _tile_origins("tile_gather", origins)
    th, tw = int(tile[0]), int(tile[1])
    if th < 1 or tw < 1:
        raise ValueError(f"tile_gather: bad tile {tile!r}")
    T = origins.shape[0]
    out = torch.empty((T, 3, th, tw), dtype=torch.float32, device=image.device)
    m =(ctypes.c_float * 3)(*[float(v) for v in mean])
    call("jabd_tile_gather_f32", _p(image), 1 if image.dtype == torch.uint8 else 0,
         image.shape[0], image.shape[1], _p(origins), T, th, tw, float(fill),
         ctypes.cast(m, ctypes.c_void_p), _p(out), _stream())
    return out


def tile_collect(rows, n_keep, origins, merged, offsets, pass_index, tile, image_shape,
                 border=1.0):
    """A batch of tiles' detect rows joins `merged` on the device
    (jabd_tile_collect_f32).  rows [n_slots, A, 15] and n_keep [n_slots] are
    ops.detect's outputs for a tile batch, origins device int32 [T, 2] (T <=
    n_slots: only the first T slots are read), tile = (tile_h, tile_w),
    image_shape = (im_height, im_width).  A row whose box comes within `border`
    tile pixels of a tile side that lies inside the image is dropped (the tile
    cut the face: a neighbouring tile sees it whole); the others are brought to
    image pixels and written, in tile and row order, from
    merged[offsets[pass_index]] on; offsets[pass_index + 1] = min(offsets[
    pass_index] + survivors, len(merged)).  border=-inf keeps every row.
    offsets as ops.tta_collect takes it: both can extend one chain.  No host
    synchronisation.  Returns merged."""
    rows = _dev("tile_collect.rows", rows)
    n_keep = _dev("tile_collect.n_keep", n_keep, torch.int64)
    origins = _tile_origins("tile_collect", origins)
    if rows.dim() != 3 or rows.shape[2] != 15:
        raise ValueError(f"tile_collect: rows must be [n_slots, A, 15], got {tuple(rows.shape)}")
    S, A = rows.shape[0], rows.shape[1]
    T = origins.shape[0]
    if T > S or n_keep.numel() < T:
        raise ValueError(f"tile_collect: {T} origins for {S} slots and {n_keep.numel()} counts")
    for name, t, dt in (("merged", merged, torch.float32), ("offsets", offsets, torch.int64)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt
                and t.is_contiguous()):
            raise ValueError(f"tile_collect: {name} must be a contiguous device {dt} tensor")
    if merged.dim() != 2 or merged.shape[1] != 15:
        raise ValueError(f"tile_collect: merged must be [cap, 15], got {tuple(merged.shape)}")
    p = int(pass_index)
    if p < 0 or offsets.dim() != 1 or offsets.numel() < p + 2:
        raise ValueError("tile_collect: offsets needs pass_index + 2 entries")
    border = float(border)
    if math.isnan(border):
        raise ValueError("tile_collect: border is NaN")
    ws = _ws(_size_query("jabd_tile_collect_workspace_size", T, A), rows.device)
    call("jabd_tile_collect_f32", _p(rows), _p(n_keep), T, A, _p(origins), int(tile[0]),
         int(tile[1]), int(image_shape[0]), int(image_shape[1]), border, _p(merged),
         merged.shape[0], _p(offsets), p, _p(ws), ws.numel(), _stream())
    return merged


# --------------------------------------------------------------------------- batched detection
def _image_u8(name, index, image):
    """image as a C-contiguous uint8 [H, W, 3] array."""
    arr = np.asarray(image)
    if arr.dtype != np.uint8:
        raise TypeError(f"{name}: image {index} must be uint8, got {arr.dtype}")
    if arr.ndim != 3 or arr.shape[2] != 3 or arr.shape[0] < 1 or arr.shape[1] < 1:
        raise ValueError(f"{name}: image {index} must be [H, W, 3], got {arr.shape}")
    return np.ascontiguousarray(arr)


def _letterbox_sides(ih, iw, size):
    """(nw, nh) of utils/utils.py:10-13 for size = (w, h), as jabd_letterbox_f32
    derives them (float64)."""
    w, h = int(size[0]), int(size[1])
    scale = min(w / iw, h / ih)
    return int(iw * scale), int(ih * scale)


def _pack_arrays(name, images, size, first=0):
    """The checked uint8 arrays of `images` and their int64 [n, 3] slot table
    (offsets from 0); `first` is the index of images[0] in the caller's count."""
    arrs = [_image_u8(name, first + i, im) for i, im in enumerate(images)]
    desc = np.zeros((len(arrs), 3), np.int64)
    off = 0
    for i, a in enumerate(arrs):
        ih, iw = a.shape[0], a.shape[1]
        if size is not None:
            nw, nh = _letterbox_sides(ih, iw, size)
            if nw == 0 or nh == 0:
                raise ValueError(f"{name}: image {first + i} ({ih} x {iw}) collapses to "
                                 f"{nh} x {nw} on a {int(size[1])} x {int(size[0])} canvas")
        desc[i] = (off, ih, iw)
        off += a.size
    return arrs, desc, off


def pack_images(images, size=None):
    """Host only: the pool and slot table ops.letterbox_batch takes.  images:
    uint8 [H, W, 3] RGB arrays (or anything np.asarray turns into one) of any
    sizes; another dtype raises TypeError, another shape ValueError.  Returns
    (pool, desc): pool uint8 1-D, the images' bytes back to back, and desc
    int64 [n, 3] = (byte offset into pool, ih, iw), both pinned where a device
    is present (plain host tensors otherwise).  With size = (w, h) an image
    whose letterbox to that canvas collapses (nw or nh 0) raises ValueError
    naming its index, before any device work."""
    arrs, desc, total = _pack_arrays("pack_images", list(images), size)
    pin = torch.cuda.is_available()
    pool = torch.empty(total, dtype=torch.uint8, pin_memory=pin)
    view = pool.numpy()
    for a, (off, _, _) in zip(arrs, desc):
        view[off:off + a.size] = a.reshape(-1)
    table = torch.empty((len(arrs), 3), dtype=torch.int64, pin_memory=pin)
    table.numpy()[...] = desc
    return pool, table


def _batch_desc(name, desc):
    desc = _dev(name + ".desc", desc, torch.int64)
    if desc.dim() != 2 or desc.shape[1] != 3:
        raise ValueError(f"{name}: desc must be int64 [n, 3], got {tuple(desc.shape)}")
    return desc


def letterbox_batch(pool, desc, size, fill=84.0, mean=(104.0, 117.0, 123.0), pool_bytes=None):
    """Images of different sizes letterboxed into one network input batch
    (jabd_letterbox_batch_u8).  pool device uint8 1-D and desc device int64
    [n, 3] as ops.pack_images lays them out; size = (w, h) as ops.letterbox
    takes it.  Returns float32 [n, 3, h, w]: slot i holds the bytes of
    ops.letterbox(image_i.float(), size, fill, mean).  An empty slot (ih or iw
    <= 0, a letterbox that collapses, or bytes not inside the pool) is
    fill - mean everywhere and reads nothing.  pool_bytes (default: all of
    pool) is the size the range check uses; it may not exceed len(pool)."""
    pool = _dev("letterbox_batch.pool", pool, torch.uint8)
    if pool.dim() != 1:
        raise ValueError(f"letterbox_batch: pool must be 1-D, got {tuple(pool.shape)}")
    desc = _batch_desc("letterbox_batch", desc)
    w, h = int(size[0]), int(size[1])
    if w < 1 or h < 1:
        raise ValueError(f"letterbox_batch: bad size {size!r}")
    nbytes = pool.numel() if pool_bytes is None else int(pool_bytes)
    if not 0 <= nbytes <= pool.numel():
        raise ValueError(f"letterbox_batch: pool_bytes {nbytes} outside [0, {pool.numel()}]")
    n = desc.shape[0]
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=pool.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    call("jabd_letterbox_batch_u8", _p(pool), nbytes, _p(desc), n, _p(out), h, w, float(fill),
         ctypes.cast(m, ctypes.c_void_p), _stream())
    return out


def batch_collect(rows, n_keep, desc, input_shape, max_det=0, out=None, offsets=None):
    """A batch's detect rows brought to each image's own pixels and packed
    (jabd_batch_collect_f32).  rows [n_slots, A, 15] and n_keep [n_slots] are
    ops.detect's outputs for a letterboxed batch, desc device int64 [n, 3]
    the batch's slot table (n <= n_slots: only the first n slots are read),
    input_shape = (H, W) of the network input.  Slot i contributes its first
    count_i = clamp(n_keep[i], 0, A) rows, at most max_det of them when
    max_det > 0 and none when the slot is empty; they are corrected as
    correct_boxes(..., (ih_i, iw_i), letterbox=True, to_pixels=True) and
    written from out[offsets[i]] on, with offsets[0] = 0 and offsets[i + 1] =
    min(offsets[i] + count_i, len(out)).  out: device float32 [cap, 15]
    (default: a new [n * A, 15] tensor; rows beyond the capacity are dropped,
    rows no survivor lands on are left as they are), offsets: device int64
    [n + 1] (default: new).  No host synchronisation.  Returns (out, offsets)."""
    rows = _dev("batch_collect.rows", rows)
    n_keep = _dev("batch_collect.n_keep", n_keep, torch.int64)
    desc = _batch_desc("batch_collect", desc)
    if rows.dim() != 3 or rows.shape[2] != 15:
        raise ValueError(f"batch_collect: rows must be [n_slots, A, 15], got {tuple(rows.shape)}")
    S, A = rows.shape[0], rows.shape[1]
    n = desc.shape[0]
    if n > S or n_keep.numel() < n:
        raise ValueError(f"batch_collect: {n} table rows for {S} slots and {n_keep.numel()} "
                         "counts")
    H, W = int(input_shape[0]), int(input_shape[1])
    if H < 1 or W < 1:
        raise ValueError(f"batch_collect: bad input shape {input_shape!r}")
    if out is None:
        out = torch.empty((n * A, 15), dtype=torch.float32, device=rows.device)
    if offsets is None:
        offsets = torch.empty(n + 1, dtype=torch.int64, device=rows.device)
    for name, t, dt in (("out", out, torch.float32), ("offsets", offsets, torch.int64)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt
                and t.is_contiguous()):
            raise ValueError(f"batch_collect: {name} must be a contiguous device {dt} tensor")
    if out.dim() != 2 or out.shape[1] != 15:
        raise ValueError(f"batch_collect: out must be [cap, 15], got {tuple(out.shape)}")
    if offsets.dim() != 1 or offsets.numel() < n + 1:
        raise ValueError(f"batch_collect: offsets needs {n + 1} entries")
    call("jabd_batch_collect_f32", _p(rows), _p(n_keep), n, A, _p(desc), H, W, int(max_det),
         _p(out), out.shape[0], _p(offsets), _stream())
    return out, offsets


# the widely used ArcFace five-point template of a 112 x 112 crop: left eye,
# right eye, nose, left and right mouth corner (a row's columns 5..14)
ARCFACE_112 = ((38.2946, 51.6963), (73.5318, 51.5014), (56.0252, 71.7366),
               (41.5493, 92.3655), (70.7299, 92.2041))


def align_template(size=112):
    """Host only: the default template of ops.align_faces for a size x size
    crop, float32 [5, 2]: ARCFACE_112 * (size / 112), formed in double."""
    return (np.array(ARCFACE_112, np.float64) * (float(size) / 112.0)).astype(np.float32)


def _align_args(name, size, template, out, mean, std):
    """Checked host arguments of align_faces: (size, template float32 [10],
    out_kind, mean float32 [3], std float32 [3])."""
    if int(size) != size or not 1 <= int(size) <= 1024:
        raise ValueError(f"{name}: size must be an int in [1, 1024], got {size!r}")
    size = int(size)
    if template is None:
        q = align_template(size)
    else:
        q = np.asarray(template, np.float32)
        if q.shape != (5, 2) or not np.isfinite(q).all():
            raise ValueError(f"{name}: template must be five finite (x, y) points")
    if out not in ("u8", "f32"):
        raise ValueError(f"{name}: out must be 'u8' or 'f32', got {out!r}")
    m = np.ascontiguousarray(np.broadcast_to(np.asarray(mean, np.float32), (3,)))
    s = np.ascontiguousarray(np.broadcast_to(np.asarray(std, np.float32), (3,)))
    if not (np.isfinite(m).all() and np.isfinite(s).all() and (s != 0).all()):
        raise ValueError(f"{name}: mean must be finite and std finite and non-zero")
    return size, np.ascontiguousarray(q.reshape(10)), 0 if out == "u8" else 1, m, s


def align_faces(pool, desc, rows, offsets, size=112, template=None, antialias=True, out="u8",
                mean=127.5, std=127.5, bgr=False, crops=None, matrices=None, pool_bytes=None):
    """Aligned face crops from detect rows, on the device
    (jabd_align_faces_u8).  pool device uint8 1-D and desc device int64 [n, 3]
    as ops.pack_images lays them out; rows device float32 [cap, 15] in image
    pixels and offsets device int64 [n + 1] as ops.batch_collect returns them:
    the first min(offsets[n], cap) rows are faces, face r belonging to image i
    with offsets[i] <= r < offsets[i + 1].  Each face's landmarks are fitted
    to `template` (float32 [5, 2] crop coordinates; default align_template(size))
    by a least-squares similarity, and the image is warped into a size x size
    crop, bilinear, with up to 4 x 4 sub-samples per pixel where the face is
    scaled down (antialias=False: always one).  out "u8": crops uint8 [cap,
    size, size, 3] RGB; "f32": float32 [cap, 3, size, size], plane k = (value -
    mean[k]) / std[k] of channel k, or of channel 2 - k with bgr (mean, std: a
    number or three).  An invalid face (a non-finite landmark, coinciding
    landmarks, an empty slot) gives a crop of zeros ("f32": of (0 - mean) / std)
    and a zero matrix.  Returns (crops, matrices): matrices float32 [cap, 6] =
    the 2 x 3 forward matrix (a, -b, tx, b, a, ty) per face; matrices=False
    skips them (None is returned in their place).  crops / matrices may be
    given (contiguous device tensors of those shapes); entries of faces beyond
    the count are not written.  No workspace and no host synchronisation.
    pool_bytes as in letterbox_batch."""
    pool = _dev("align_faces.pool", pool, torch.uint8)
    if pool.dim() != 1:
        raise ValueError(f"align_faces: pool must be 1-D, got {tuple(pool.shape)}")
    desc = _batch_desc("align_faces", desc)
    rows = _dev("align_faces.rows", rows)
    offsets = _dev("align_faces.offsets", offsets, torch.int64)
    if rows.dim() != 2 or rows.shape[1] != 15:
        raise ValueError(f"align_faces: rows must be [cap, 15], got {tuple(rows.shape)}")
    n, cap = desc.shape[0], rows.shape[0]
    if offsets.dim() != 1 or offsets.numel() < n + 1:
        raise ValueError(f"align_faces: offsets needs {n + 1} entries")
    size, q, kind, m, s = _align_args("align_faces", size, template, out, mean, std)
    nbytes = pool.numel() if pool_bytes is None else int(pool_bytes)
    if not 0 <= nbytes <= pool.numel():
        raise ValueError(f"align_faces: pool_bytes {nbytes} outside [0, {pool.numel()}]")
    shape = (cap, size, size, 3) if kind == 0 else (cap, 3, size, size)
    dtype = torch.uint8 if kind == 0 else torch.float32
    if crops is None:
        crops = torch.empty(shape, dtype=dtype, device=rows.device)
    if matrices is None:
        matrices = torch.empty((cap, 6), dtype=torch.float32, device=rows.device)
    elif matrices is False:
        matrices = None
    for name, t, dt, shp in (("crops", crops, dtype, shape),
                             ("matrices", matrices, torch.float32, (cap, 6))):
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt
                                  and t.is_contiguous() and tuple(t.shape) == shp):
            raise ValueError(f"align_faces: {name} must be a contiguous device {dt} tensor of "
                             f"shape {shp}")
    call("jabd_align_faces_u8", _p(pool), nbytes, _p(desc), n, _p(rows), _p(offsets), cap,
         ctypes.c_void_p(q.ctypes.data), size, 1 if antialias else 0, kind,
         ctypes.c_void_p(m.ctypes.data), ctypes.c_void_p(s.ctypes.data), 1 if bgr else 0,
         _p(crops), _p(matrices), _stream())
    return crops, matrices


def detect(loc, conf, landm, priors, variances, conf_threshold=0.5, nms_threshold=0.3,
           nms_kind="greedynms", beta1=1.0, top_k=0, sigma=0.5, soft_offset=0.0):
    """predict.py:162-181 on device for a batch: decode + filter + NMS.

    loc [B,A,4], conf [B,A,2] (eval softmax), landm [B,A,10].
    Returns (rows [B,A,15], n_keep [B]); rows[b,:n_keep[b]] are the kept
    detections (x1,y1,x2,y2,score,landmarks) in NMS order.
    nms_kind, beta1, top_k: the suppression rule, as batched_nms.
    nms_kind "softnms" (or "softernms"): Gaussian Soft-NMS (batched_soft_nms)
    with `sigma` and `soft_offset`; nms_threshold and beta1 are ignored, the
    rows are in the Soft-NMS's result order and column 4 holds the decayed
    score.  soft_offset defaults to 0, not the reference's pixel +1: the
    decoded boxes are normalised, and with +1 every pair would overlap.
    """
    soft = is_soft_kind(nms_kind)
    if soft:
        sigma, soft_offset = _soft_args(sigma, soft_offset)
    else:
        k = _kind_code(nms_kind, beta1)
    loc = _dev("detect.loc", loc)
    conf = _dev("detect.conf", conf)
    landm = _dev("detect.landm", landm)
    priors = _dev("detect.priors", priors)
    B, A = loc.shape[0], loc.shape[1]
    if priors.shape != (A, 4) or conf.shape != (B, A, 2) or landm.shape != (B, A, 10):
        raise ValueError("detect: shape mismatch")
    dev = loc.device
    out = torch.empty((B, A, 15), dtype=torch.float32, device=dev)
    n_keep = torch.empty((B,), dtype=torch.int64, device=dev)   # written by every call
    if soft:
        ws = _ws(_size_query("jabd_detect_soft_workspace_size", B, A), dev)
        call("jabd_detect_soft_f32", _p(loc), _p(conf), _p(landm), _p(priors), B, A,
             float(variances[0]), float(variances[1]), float(conf_threshold), sigma, soft_offset,
             SOFT_PRUNE, int(top_k), _p(out), _p(n_keep), _p(ws), ws.numel(), _stream())
        return out, n_keep
    ws = _ws(_size_query("jabd_detect_workspace_size", B, A), dev)
    args = (_p(loc), _p(conf), _p(landm), _p(priors), B, A,
            float(variances[0]), float(variances[1]), float(conf_threshold), float(nms_threshold),
            _p(out), _p(n_keep), _p(ws), ws.numel(), _stream())
    if k == 0 and int(top_k) <= 0:
        call("jabd_detect_f32", *args)
    else:
        call("jabd_detect_ex_f32", *args, k, float(beta1), int(top_k))
    return out, n_keep


# --------------------------------------------------------------------------- match
def match_encode(targets, priors, threshold, variances, raw_loc=False):
    """Batched match()+encode() — nets/retinaface_training.py:93-162.

    targets: list of B device tensors [n_i,15]; priors [A,4].
    Returns loc_t [B,A,4], conf_t [B,A] int64, landm_t [B,A,10].
    raw_loc=True is match_iou() (nets/retinaface_training_DIOU.py:176-246):
    loc_t holds the matched truth corners instead of the encoded offsets.
    """
    priors = _dev("match.priors", priors)
    dev = priors.device
    B, A = len(targets), priors.shape[0]
    counts = [int(t.shape[0]) for t in targets]
    if any(c == 0 for c in counts):
        raise ValueError("match: an image has no targets (the reference's match() fails too)")
    for t in targets:
        _dev("match.targets", t)
    if len(targets) == 1:
        flat = targets[0].reshape(-1, 15).contiguous()
    else:  # the images' rows back to back, one launch
        flat = torch.empty((sum(counts), 15), dtype=torch.float32, device=dev)
        items, o = [], 0
        for t, c in zip(targets, counts):
            items.append((t.reshape(-1, 15).contiguous(), flat[o:o + c], 0.0))
            o += c
        from .functional import window_copies
        window_copies(items)
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + c)
    offsets = torch.tensor(offs, dtype=torch.int64).to(dev, non_blocking=True)
    loc_t = torch.empty((B, A, 4), dtype=torch.float32, device=dev)
    conf_t = torch.empty((B, A), dtype=torch.int64, device=dev)
    landm_t = torch.empty((B, A, 10), dtype=torch.float32, device=dev)
    ws = _ws(_size_query("jabd_match_workspace_size", B, A), dev)
    call("jabd_match_iou_f32" if raw_loc else "jabd_match_encode_f32", _p(flat), _p(offsets), B, max(counts) if counts else 0,
         _p(priors), A, float(threshold), float(variances[0]), float(variances[1]), _p(loc_t),
         _p(conf_t), _p(landm_t), _p(ws), ws.numel(), _stream())
    return loc_t, conf_t, landm_t


# --------------------------------------------------------------------------- loss
IOU_KINDS = {"Iou": 0, "Giou": 1, "Diou": 2, "Ciou": 3}


def iou_kind(kind):
    """The C-ABI kind (0..3) of an IouLoss losstype: one of the exact names
    'Iou', 'Giou', 'Diou', 'Ciou' (nets/retinaface_training_DIOU.py:507-516), or
    that integer.  The reference treats every other string as CIoU; here it
    is an error."""
    if isinstance(kind, str):
        if kind not in IOU_KINDS:
            raise ValueError(f"losstype must be one of {', '.join(IOU_KINDS)}; got {kind!r}")
        return IOU_KINDS[kind]
    if isinstance(kind, bool) or not isinstance(kind, int) or not 0 <= kind <= 3:
        raise ValueError(f"losstype must be one of {', '.join(IOU_KINDS)} (or 0..3); "
                         f"got {kind!r}")
    return kind


def multibox_sums(loc, conf, landm, loc_t, conf_t, landm_t, neg_pos, diou=None):
    """Un-normalised MultiBoxLoss sums [3], counts [2] and the selection mask.

    diou=(priors [A,4], variances) or (priors, variances, kind): the box term is
    the IouLoss of nets/retinaface_training_DIOU.py:491-522 (loc_t from
    match_encode(raw_loc=True)); kind is a losstype name or 0..3 (iou_kind),
    'Diou' when left out.
    """
    loc, conf, landm = (_dev("loss.loc", loc), _dev("loss.conf", conf),
                        _dev("loss.landm", landm))
    loc_t, landm_t = _dev("loss.loc_t", loc_t), _dev("loss.landm_t", landm_t)
    conf_t = _dev("loss.conf_t", conf_t, torch.int64)
    B, A = loc.shape[0], loc.shape[1]
    dev = loc.device
    if diou is not None:
        pri, var, kind = _iou_priors(diou, A)
    sums = torch.empty(3, dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    sel = torch.empty((B, A), dtype=torch.uint8, device=dev)
    ws = _ws(_size_query("jabd_multibox_workspace_size", B, A), dev)
    if diou is None:
        call("jabd_multibox_loss_fwd_f32", _p(loc), _p(conf), _p(landm), _p(loc_t), _p(conf_t),
             _p(landm_t), B, A, int(neg_pos), _p(sums), _p(counts), _p(sel), _p(ws),
             ws.numel(), _stream())
    else:
        call("jabd_multibox_iou_loss_fwd_f32", _p(loc), _p(conf), _p(landm), _p(loc_t),
             _p(conf_t), _p(landm_t), _p(pri), float(var[0]), float(var[1]), B, A,
             int(neg_pos), _p(sums), _p(counts), _p(sel), _p(ws), ws.numel(), kind, _stream())
    return sums, counts, sel


def _iou_priors(diou, A):
    pri, var = diou[0], diou[1]
    kind = iou_kind(diou[2]) if len(diou) > 2 else IOU_KINDS["Diou"]
    pri = _dev("loss.priors", pri)
    if tuple(pri.shape) != (A, 4):
        raise ValueError(f"IoU loss: priors {tuple(pri.shape)} != ({A}, 4)")
    return pri, var, kind


def multibox_normalize(sums, counts):
    loss = torch.empty(3, dtype=torch.float32, device=sums.device)
    call("jabd_multibox_loss_finalize_f32", _p(sums), _p(counts), _p(loss), _stream())
    return loss


def multibox_backward(loc, conf, landm, loc_t, conf_t, landm_t, sel, gout, counts, diou=None):
    """The three gradients; diou as multibox_sums takes it."""
    B, A = loc.shape[0], loc.shape[1]
    if diou is not None:
        pri, var, kind = _iou_priors(diou, A)
    gl = torch.empty_like(loc)
    gc = torch.empty_like(conf)
    glm = torch.empty_like(landm)
    gout = _dev("loss.gout", gout)
    if diou is None:
        call("jabd_multibox_loss_bwd_f32", _p(loc), _p(conf), _p(landm), _p(loc_t), _p(conf_t),
             _p(landm_t), _p(sel), B, A, _p(gout), _p(counts), _p(gl), _p(gc), _p(glm),
             _stream())
    else:
        call("jabd_multibox_iou_loss_bwd_f32", _p(loc), _p(conf), _p(landm), _p(loc_t),
             _p(conf_t), _p(landm_t), _p(pri), float(var[0]), float(var[1]), _p(sel), B, A,
             _p(gout), _p(counts), _p(gl), _p(gc), _p(glm), kind, _stream())
    return gl, gc, glm


def _iou_rows_args(pred, priors, truth, kind):
    pred, truth = _dev("iou_rows.pred", pred), _dev("iou_rows.truth", truth)
    if pred.dim() != 2 or pred.shape[1] != 4 or truth.dim() != 2 or truth.shape[1] != 4:
        raise ValueError(f"iou_rows: [P,4] boxes, got {tuple(pred.shape)} and "
                         f"{tuple(truth.shape)}")
    if pred.shape[0] != truth.shape[0]:
        raise ValueError(f"iou_rows: paired rows only ({pred.shape[0]} predictions vs "
                         f"{truth.shape[0]} truths; the reference's row swap and broadcast "
                         "are not reproduced)")
    if priors is not None:
        priors = _dev("iou_rows.priors", priors)
        if priors.shape != pred.shape:
            raise ValueError(f"iou_rows: priors {tuple(priors.shape)} != {tuple(pred.shape)}")
    return pred, priors, truth, iou_kind(kind)


def iou_rows(pred, truth, kind, priors=None, variances=(0.1, 0.2)):
    """bbox_overlaps_<kind> for paired rows (nets/retinaface_training_DIOU.py:
    339-490): the clamped overlaps [P] of pred [P,4] against truth [P,4].
    priors=None: pred holds corner boxes; otherwise loc offsets decoded in the
    kernel against priors [P,4] with `variances` (IouLoss pred_mode 'Center').
    P == 0 launches nothing."""
    pred, priors, truth, k = _iou_rows_args(pred, priors, truth, kind)
    val = torch.empty(pred.shape[0], dtype=torch.float32, device=pred.device)
    call("jabd_iou_rows_fwd_f32", _p(pred), _p(priors), _p(truth), pred.shape[0],
         float(variances[0]), float(variances[1]), k, _p(val), _stream())
    return val


def iou_rows_backward(pred, truth, kind, gval, priors=None, variances=(0.1, 0.2)):
    """dL/dpred [P,4] of iou_rows given dL/dval [P]."""
    pred, priors, truth, k = _iou_rows_args(pred, priors, truth, kind)
    gval = _dev("iou_rows.gval", gval)
    if gval.shape != pred.shape[:1]:
        raise ValueError(f"iou_rows: gval {tuple(gval.shape)} != ({pred.shape[0]},)")
    gpred = torch.empty_like(pred)
    call("jabd_iou_rows_bwd_f32", _p(pred), _p(priors), _p(truth), pred.shape[0],
         float(variances[0]), float(variances[1]), k, _p(gval), _p(gpred), _stream())
    return gpred


def fixed_sum(x):
    """Σ x of a device float32 vector as a [1] tensor, in a fixed order
    (jabd_colsum_f32): two runs agree bit for bit.  Empty -> 0."""
    x = _dev("fixed_sum.x", x).reshape(-1)
    if x.numel() == 0:
        return torch.zeros(1, dtype=torch.float32, device=x.device)
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    call("jabd_colsum_f32", _p(x), x.numel(), 1, _p(out), _stream())
    return out


# --------------------------------------------------------------------------- letterbox
def letterbox(image, size, fill=84.0, mean=None):
    """utils/utils.py:8-19 letterbox_image (+ :27-29 preprocess_input when `mean`
    is given) on the device — see jabd_letterbox_f32.

    image: device float32 [ih, iw, 3] or [B, ih, iw, 3]; size = (w, h) as the
    reference passes it.  mean=None -> [.., h, w, 3] canvas; mean=(m0, m1, m2)
    -> [B, 3, h, w] network input (canvas - mean, NCHW).
    """
    image = _dev("letterbox.image", image)
    squeeze = image.dim() == 3
    if squeeze:
        image = image.unsqueeze(0)
    if image.dim() != 4 or image.shape[-1] != 3:
        raise ValueError(f"letterbox: expected [B, H, W, 3], got {tuple(image.shape)}")
    B, ih, iw = image.shape[0], image.shape[1], image.shape[2]
    w, h = int(size[0]), int(size[1])
    if mean is None:
        out = torch.empty((B, h, w, 3), dtype=torch.float32, device=image.device)
        m = None
    else:
        out = torch.empty((B, 3, h, w), dtype=torch.float32, device=image.device)
        m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    call("jabd_letterbox_f32", _p(image), B, ih, iw, _p(out), h, w, float(fill),
         ctypes.cast(m, ctypes.c_void_p) if m is not None else ctypes.c_void_p(0),
         0 if mean is None else 1, _stream())
    return out[0] if (squeeze and mean is None) else out


def correct_boxes(rows, input_shape, image_shape, letterbox=True, to_pixels=True):
    """In place on device rows [n, 15]: retinaface_correct_boxes
    (utils/utils_bbox.py:9-24, if letterbox) then predict.py:195-196's scale to
    image pixels.  input_shape = (H, W) of the network input, image_shape =
    (im_height, im_width)."""
    rows = _dev("correct_boxes.rows", rows)
    if rows.dim() != 2 or rows.shape[1] != 15:
        raise ValueError(f"correct_boxes: expected [n, 15], got {tuple(rows.shape)}")
    call("jabd_correct_boxes_f32", _p(rows), rows.shape[0], int(input_shape[0]),
         int(input_shape[1]), int(image_shape[0]), int(image_shape[1]), 1 if letterbox else 0,
         1 if to_pixels else 0, _stream())
    return rows


# --------------------------------------------------------------------------- augment
def augment(image_u8, input_shape, nw, nh, dx, dy, flip, hue, sat, val):
    """utils/dataloader.py:71-115 + :62-64 image part on the device, given the
    random draws (see utils.dataloader.draw_params).  image_u8: device uint8
    RGB [ih, iw, 3]; input_shape = (h, w).  Returns float32 [3, h, w]."""
    img = _dev("augment.image", image_u8, torch.uint8)
    if img.dim() != 3 or img.shape[2] != 3:
        raise ValueError(f"augment: expected [H, W, 3] uint8, got {tuple(img.shape)}")
    ih, iw = int(img.shape[0]), int(img.shape[1])
    h, w = int(input_shape[0]), int(input_shape[1])
    out = torch.empty((3, h, w), dtype=torch.float32, device=img.device)
    ws = _ws(_size_query("jabd_augment_workspace_size", ih, int(nw)), img.device)
    call("jabd_augment_u8", _p(img), ih, iw, int(nw), int(nh), h, w, int(dx), int(dy),
         1 if flip else 0, float(hue), float(sat), float(val), _p(out), _p(ws), ws.numel(),
         _stream())
    return out


# --------------------------------------------------------------------------- WIDER eval
def wider_pr_curve(preds, gts, ignores, iou_thresh=0.5, thresh_num=1000, device="cuda"):
    """Σ over images of img_pr_info(image_eval(...)) — utils/evaluation.py:255-305,
    347-375 — on the device.  preds: list of [n_i, 5] (x, y, w, h, score) arrays,
    gts: list of [m_i, 4] (x, y, w, h), ignores: list of [m_i] (1 = kept).
    Returns the float64 pr_curve [thresh_num, 2] (device tensor)."""
    def cat(xs, k, dt):
        a = [np.asarray(x, dt).reshape(-1, k) if k else np.asarray(x, dt).reshape(-1) for x in xs]
        offs = np.zeros(len(a) + 1, np.int64)
        offs[1:] = np.cumsum([len(x) for x in a])
        flat = np.concatenate(a) if a else np.zeros((0,) + ((k,) if k else ()), dt)
        return (torch.from_numpy(np.ascontiguousarray(flat)).to(device),
                torch.from_numpy(offs).to(device), int(offs[-1]))
    if not (len(preds) == len(gts) == len(ignores)):
        raise ValueError("wider_pr_curve: preds, gts and ignores differ in length")
    p, poff, npred = cat(preds, 5, np.float64)
    g, goff, ngt = cat(gts, 4, np.float64)
    ig, _, _ = cat(ignores, 0, np.uint8)
    pr = torch.zeros((thresh_num, 2), dtype=torch.float64, device=device)
    ws = _ws(_size_query("jabd_wider_eval_workspace_size", npred, ngt), device)
    call("jabd_wider_eval_f64", _p(p), _p(poff), _p(g), _p(ig), _p(goff), len(preds), npred, ngt,
         float(iou_thresh), int(thresh_num), _p(pr), _p(ws), ws.numel(), _stream())
    return pr


# --------------------------------------------------------------------------- bicubic
def _bicubic_call(fn, src, size_in, size_out):
    B, H, W, C = size_in
    OH, OW = size_out
    dst = torch.empty((B, OH, OW, C) if fn.endswith("ac_f32") else (B, H, W, C),
                      dtype=torch.float32, device=src.device)
    call(fn, _p(src), B, H, W, C, _p(dst), OH, OW, _stream())
    return dst


class UpsampleBicubicFn(torch.autograd.Function):
    """F.interpolate(x, size, mode="bicubic", align_corners=True) on NHWC
    (train_mobilenetV3_ecagai.py:270,279), HIP forward and backward."""

    @staticmethod
    def forward(ctx, x, oh, ow):
        x = _dev("bicubic.x", x)
        if x.dim() != 4:
            raise ValueError(f"bicubic: expected NHWC, got {tuple(x.shape)}")
        ctx.shape = tuple(x.shape)
        return _bicubic_call("jabd_upsample_bicubic_ac_f32", x, ctx.shape, (oh, ow))

    @staticmethod
    def backward(ctx, gy):
        B, H, W, C = ctx.shape
        gy = gy.contiguous()
        gx = _bicubic_call("jabd_upsample_bicubic_ac_bwd_f32", gy, ctx.shape,
                           (gy.shape[1], gy.shape[2]))
        return gx, None, None


def upsample_bicubic(x_nhwc, size):
    """NHWC bicubic align_corners resize to size = (OH, OW)."""
    return UpsampleBicubicFn.apply(x_nhwc, int(size[0]), int(size[1]))


# --------------------------------------------------------------------------- BECA
def beca_part(B, pixels, C, device):
    """Reduction workspace of jabd_beca_fwd_f32 / _bwd_f32."""
    n = int(lib().jabd_beca_ws_floats(B, pixels, C))
    return torch.empty(max(n, 1), dtype=torch.float32, device=device)


class BecaFn(torch.autograd.Function):
    """eca_block of the bicubic variant (train_mobilenetV3_ecagai.py:286-316) on
    NHWC x [B, H, W, C] with the conv1d weight w [k]: x * Hardsigmoid(conv1d(std))."""

    @staticmethod
    def forward(ctx, x, w):
        x = _dev("beca.x", x)
        w = _dev("beca.w", w.reshape(-1))
        B, H, W, C = x.shape
        y = torch.empty_like(x)
        stats = torch.empty((4, B * C), dtype=torch.float32, device=x.device)
        part = beca_part(B, H * W, C, x.device)
        call("jabd_beca_fwd_f32", _p(x), B, H * W, C, _p(w), w.numel(), _p(y), _p(stats),
             _p(part), part.numel(), _stream())
        from .functional import tap
        tap("beca", stats[2].view(B, C))
        ctx.save_for_backward(x, w, stats)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, stats = ctx.saved_tensors
        B, H, W, C = x.shape
        gy = gy.contiguous()
        gx = torch.empty_like(x)
        gw = torch.empty_like(w)
        ws = torch.empty((2, B * C), dtype=torch.float32, device=x.device)
        part = beca_part(B, H * W, C, x.device)
        call("jabd_beca_bwd_f32", _p(x), _p(gy), B, H * W, C, _p(w), w.numel(), _p(stats),
             _p(gx), _p(gw), _p(ws), _p(part), part.numel(), _stream())
        return gx, gw


def beca(x_nhwc, weight):
    """weight: the block's Conv1d(1, 1, k) weight (any shape with k elements)."""
    return BecaFn.apply(x_nhwc, weight.reshape(-1))


def version():
    return lib().jabd_version().decode()
