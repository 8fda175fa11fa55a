"""CPU (numpy) restatement of tiled detection's device steps, for
tests/test_tile_plan.py, test_tile_gather.py, test_tile_collect.py and
test_predict_tiled.py: the plan (predict.tile_plan), the image -> tile-batch
gather (jabd_tile_gather_f32), the tile -> image collect with its edge filter
(jabd_tile_collect_f32) and the merge of the collected rows.  The arithmetic
is the one include/jabd.h states, every step rounded as it says."""
import math

import numpy as np

X_COLS = [0, 2, 5, 7, 9, 11, 13]
Y_COLS = [1, 3, 6, 8, 10, 12, 14]


def axis_origins(L, t, o):
    """One axis of the plan: stride t - o, n = 1 if L <= t else
    ceil((L - t) / stride) + 1, origin k = min(k stride, L - t)."""
    if L <= t:
        return [0]
    stride = t - o
    n = math.ceil((L - t) / stride) + 1
    return [min(k * stride, L - t) for k in range(n)]


def plan(ih, iw, tile, overlap):
    ys = axis_origins(ih, tile[0], overlap[0])
    xs = axis_origins(iw, tile[1], overlap[1])
    return np.array([(y, x) for y in ys for x in xs], np.int32).reshape(-1, 2)


def gather(image, origins, tile, fill=84.0, mean=(104.0, 117.0, 123.0)):
    """float32 [T, 3, th, tw]: pixel (or fill) minus the channel mean, one fp32
    subtraction; image HWC uint8 or float32."""
    img = np.asarray(image)
    ih, iw = img.shape[:2]
    th, tw = tile
    out = np.empty((len(origins), 3, th, tw), np.float32)
    m = np.asarray(mean, np.float32)
    for t, (y0, x0) in enumerate(np.asarray(origins).tolist()):
        canvas = np.full((th, tw, 3), np.float32(fill), np.float32)
        ys = [y for y in range(th) if 0 <= y0 + y < ih]
        xs = [x for x in range(tw) if 0 <= x0 + x < iw]
        if ys and xs:
            canvas[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = img[
                y0 + ys[0]:y0 + ys[-1] + 1, x0 + xs[0]:x0 + xs[-1] + 1].astype(np.float32)
        out[t] = (canvas - m).transpose(2, 0, 1)
    return out


def keep_mask(rows, origin, tile, image_shape, border):
    """The edge filter for one tile's rows [n, 15] -> bool [n] (True: kept)."""
    r = np.asarray(rows, np.float32).astype(np.float64)
    (y0, x0), (th, tw), (ih, iw) = origin, tile, image_shape
    b = float(np.float32(border))
    bx1, by1, bx2, by2 = r[:, 0] * tw, r[:, 1] * th, r[:, 2] * tw, r[:, 3] * th
    drop = np.zeros(len(r), bool)
    with np.errstate(invalid="ignore"):          # a NaN compares false: kept
        if x0 > 0:
            drop |= bx1 < b
        if x0 + tw < iw:
            drop |= bx2 > tw - b
        if y0 > 0:
            drop |= by1 < b
        if y0 + th < ih:
            drop |= by2 > th - b
    return ~drop


def to_image(rows, origin, tile):
    """Rows in normalised tile coordinates -> image pixels: (float)((double)v *
    tile + origin) per coordinate column; the score is copied."""
    r = np.array(rows, np.float32, copy=True)
    (y0, x0), (th, tw) = origin, tile
    with np.errstate(invalid="ignore", over="ignore"):
        r[:, X_COLS] = (r[:, X_COLS].astype(np.float64) * tw + x0).astype(np.float32)
        r[:, Y_COLS] = (r[:, Y_COLS].astype(np.float64) * th + y0).astype(np.float32)
    return r


def collect(rows, n_keep, origins, tile, image_shape, border, merged, offsets, pass_index):
    """jabd_tile_collect_f32 in place on numpy merged [cap, 15] / offsets:
    rows [n_slots, A, 15], n_keep [n_slots], origins [T, 2] (T <= n_slots).
    Returns the list of per-tile keep masks (over the clamped row counts)."""
    A = rows.shape[1]
    cap = merged.shape[0]
    pos = max(0, min(int(offsets[pass_index]), cap))
    masks = []
    for t, origin in enumerate(np.asarray(origins).tolist()):
        nk = max(0, min(int(n_keep[t]), A))
        mask = keep_mask(rows[t, :nk], origin, tile, image_shape, border)
        masks.append(mask)
        live = to_image(rows[t, :nk][mask], origin, tile)
        room = max(0, cap - pos)
        merged[pos:pos + min(room, len(live))] = live[:room]
        pos += len(live)
    offsets[pass_index + 1] = min(pos, cap)
    return masks


def iou_pixels(boxes):
    """fp32 IoU matrix of pixel boxes, the greedy NMS's form (no +1)."""
    b = np.asarray(boxes, np.float32)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.maximum(np.float32(0), np.minimum(b[:, None, 2], b[None, :, 2])
                   - np.maximum(b[:, None, 0], b[None, :, 0]))
    h = np.maximum(np.float32(0), np.minimum(b[:, None, 3], b[None, :, 3])
                   - np.maximum(b[:, None, 1], b[None, :, 1]))
    inter = w * h
    with np.errstate(all="ignore"):
        return inter / ((area[:, None] + area[None, :]) - inter)


def merge_nms(merged_rows, nms_iou, max_out=750):
    """The second stage with merge="nms": greedy NMS (oracle/box_ref.nms) on
    the collected pixel rows; the kept rows in descending score."""
    from oracle import box_ref
    keep = box_ref.nms(merged_rows[:, :4], merged_rows[:, 4], nms_iou)
    if max_out > 0:
        keep = keep[:max_out]
    return merged_rows[keep], keep
