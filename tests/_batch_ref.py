"""Numpy restatement of the batched-detection kernels (test infrastructure
only), built on oracle/prep_ref.py: jabd_letterbox_batch_u8 is prep_ref's
letterbox_image + preprocess_input per image, jabd_batch_collect_f32 is
prep_ref.correct_rows per slot plus the packing."""
import numpy as np

from oracle import prep_ref

MEAN = (104.0, 117.0, 123.0)


def sides(ih, iw, h, w):
    """(nw, nh) of utils/utils.py:10-13 on an h x w canvas."""
    scale = min(w / iw, h / ih)
    return int(iw * scale), int(ih * scale)


def is_empty(ih, iw, h, w):
    if ih <= 0 or iw <= 0:
        return True
    nw, nh = sides(ih, iw, h, w)
    return nw == 0 or nh == 0


def letterbox_batch(images, shape, fill=84.0, mean=MEAN):
    """float32 [n, 3, h, w]; images: uint8 [ih, iw, 3] arrays, None or an empty
    array for an empty slot.  shape = (h, w)."""
    h, w = shape
    m = np.array(mean, np.float32)
    out = np.empty((len(images), 3, h, w), np.float32)
    for i, im in enumerate(images):
        if im is None or im.size == 0 or is_empty(im.shape[0], im.shape[1], h, w):
            out[i] = (np.float32(fill) - m)[:, None, None]
            continue
        lb = prep_ref.letterbox_image(np.asarray(im, np.float32), (w, h), fill=np.float32(fill))
        out[i] = (lb - m).transpose(2, 0, 1)
    return out


def collect(rows, n_keep, sizes, input_shape, max_det, cap):
    """(out [offsets[-1], 15], offsets [n + 1]) for the first len(sizes) slots
    of rows [n_slots, A, 15]; sizes: (ih, iw) per slot."""
    A = rows.shape[1]
    h, w = input_shape
    offsets = np.zeros(len(sizes) + 1, np.int64)
    parts = []
    for i, (ih, iw) in enumerate(sizes):
        cnt = 0 if is_empty(ih, iw, h, w) else int(min(max(int(n_keep[i]), 0), A))
        if max_det > 0:
            cnt = min(cnt, max_det)
        cnt_in = max(min(cnt, cap - int(offsets[i])), 0)
        offsets[i + 1] = min(offsets[i] + cnt, cap)
        if cnt_in:
            r = rows[i, :cnt_in]
            fixed = prep_ref.correct_rows(r, (h, w), (ih, iw), letterbox=True, to_pixels=True)
            # the score column keeps its bits, whatever a float assignment would do to a NaN
            fixed.view(np.uint32)[:, 4] = np.ascontiguousarray(r).view(np.uint32)[:, 4]
            parts.append(fixed)
    out = np.concatenate(parts) if parts else np.zeros((0, 15), np.float32)
    return out, offsets
