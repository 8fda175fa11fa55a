"""numpy restatement of jabd_align_faces_u8 (include/jabd.h): the float64
similarity fit in closed form, the float32 bilinear blend and the sub-sample
mean, operation by operation in the kernel's order, so the device output can be
compared by bytes.  Python floats are IEEE doubles and numpy rounds after every
operation, which is what the kernel does with contraction off.

Two independent pieces pin the restatement itself (tests/test_align_ref.py):
umeyama_svd, the textbook SVD estimate with its reflection guard, and warp_f64,
a plain single-sample float64 bilinear warp."""
import math

import numpy as np

ARCFACE_112 = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366],
                        [41.5493, 92.3655], [70.7299, 92.2041]], np.float64)


def default_template(size):
    """The ArcFace five-point template for a size x size crop, float32 [5, 2]."""
    return (ARCFACE_112 * (float(size) / 112.0)).astype(np.float32)


class Fit:
    """ia, ib, tx, ty: Python floats; s: sub-samples per axis, 0 = invalid;
    m: float32 [6] = (a, -b, tx, b, a, ty)."""

    def __init__(self):
        self.ia = self.ib = self.tx = self.ty = 0.0
        self.s = 0
        self.m = np.zeros(6, np.float32)


def fit(lm, template, antialias=True):
    """The fit of one face: lm float32 [10] (a row's columns 5..14), template
    float32 [5, 2] or [10]."""
    lm = np.asarray(lm, np.float32).reshape(10)
    q = np.asarray(template, np.float32).reshape(10)
    f = Fit()
    if not np.isfinite(lm).all():
        return f
    p = [float(v) for v in lm]
    q = [float(v) for v in q]
    mpx = mpy = mqx = mqy = 0.0
    for i in range(5):
        mpx = mpx + p[2 * i]
        mpy = mpy + p[2 * i + 1]
        mqx = mqx + q[2 * i]
        mqy = mqy + q[2 * i + 1]
    mpx, mpy, mqx, mqy = mpx / 5.0, mpy / 5.0, mqx / 5.0, mqy / 5.0
    S = A = B = 0.0
    for i in range(5):
        px, py = p[2 * i] - mpx, p[2 * i + 1] - mpy
        qx, qy = q[2 * i] - mqx, q[2 * i + 1] - mqy
        S = S + (px * px + py * py)
        A = A + (px * qx + py * qy)
        B = B + (px * qy - py * qx)
    if not S > 0.0:
        return f
    a, b = A / S, B / S
    det = a * a + b * b
    if (a == 0.0 and b == 0.0) or not det > 0.0 or not math.isfinite(det):
        return f
    f.tx = mqx - (a * mpx - b * mpy)
    f.ty = mqy - (b * mpx + a * mpy)
    f.ia, f.ib = a / det, b / det
    s = 1
    if antialias:
        s = 4
        for k in (1, 2, 3):
            if float(k * k) * det >= 1.0:
                s = k
                break
    f.s = s
    with np.errstate(over="ignore"):
        f.m = np.array([a, -b, f.tx, b, a, f.ty], np.float64).astype(np.float32)
    return f


def sample(image, f, size):
    """The unrounded crop of a valid face: float32 [size, size, 3] from the
    uint8 image [ih, iw, 3]."""
    ih, iw = image.shape[:2]
    img = image.astype(np.float32)
    s = f.s
    idx = np.arange(size, dtype=np.float64)
    zero, one = np.float32(0), np.float32(1)
    acc = np.zeros((size, size, 3), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for jy in range(s):
            dv = (((idx + (float(jy) + 0.5) / float(s)) - 0.5) - f.ty)[:, None]
            for jx in range(s):
                du = (((idx + (float(jx) + 0.5) / float(s)) - 0.5) - f.tx)[None, :]
                sx = f.ia * du + f.ib * dv
                sy = f.ia * dv - f.ib * du
                fx, fy = np.floor(sx), np.floor(sy)
                ok = (fx >= -1.0) & (fx <= float(iw - 1)) & (fy >= -1.0) & (fy <= float(ih - 1))
                wx = np.where(ok, sx - fx, 0.0).astype(np.float32)[..., None]
                wy = np.where(ok, sy - fy, 0.0).astype(np.float32)[..., None]
                ax, ay = one - wx, one - wy
                x0 = np.where(ok, fx, 0.0).astype(np.int64)
                y0 = np.where(ok, fy, 0.0).astype(np.int64)

                def tap(yy, xx):
                    inside = ok & (yy >= 0) & (yy < ih) & (xx >= 0) & (xx < iw)
                    v = img[np.clip(yy, 0, ih - 1), np.clip(xx, 0, iw - 1)]
                    return np.where(inside[..., None], v, zero)
                p00, p01 = tap(y0, x0), tap(y0, x0 + 1)
                p10, p11 = tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
                top = p00 * ax + p01 * wx
                bot = p10 * ax + p11 * wx
                t = top * ay + bot * wy
                acc = acc + np.where(ok[..., None], t, zero)
    assert acc.dtype == np.float32
    return acc / np.float32(s * s)


def slot_image(pool, desc, i):
    """Image i of the pool as uint8 [ih, iw, 3], or None for an empty slot
    (the slot rules of jabd_letterbox_batch_u8)."""
    off, ih, iw = (int(v) for v in desc[i])
    nbytes = int(pool.size)
    if ih <= 0 or iw <= 0 or ih > 0x7fffffff or iw > 0x7fffffff:
        return None
    if off < 0 or off > nbytes or ih * iw > (nbytes - off) // 3:
        return None
    return pool[off:off + 3 * ih * iw].reshape(ih, iw, 3)


def owner(offsets, r):
    """The image of face r: offsets[i] <= r < offsets[i + 1]."""
    n = len(offsets) - 1
    for i in range(n):
        if offsets[i] <= r < offsets[i + 1]:
            return i
    raise ValueError(f"face {r} has no image in {list(offsets)}")


def finish(v, out="u8", mean=127.5, std=127.5, bgr=False):
    """The output form of an unrounded crop [size, size, 3]."""
    if out == "u8":
        return np.rint(v).astype(np.uint8)
    mean = np.broadcast_to(np.asarray(mean, np.float32), (3,))
    std = np.broadcast_to(np.asarray(std, np.float32), (3,))
    planes = v.transpose(2, 0, 1)
    if bgr:
        planes = planes[::-1]
    res = (planes - mean[:, None, None]) / std[:, None, None]
    assert res.dtype == np.float32
    return np.ascontiguousarray(res)


def align_faces(pool, desc, rows, offsets, size, template=None, antialias=True, out="u8",
                mean=127.5, std=127.5, bgr=False, crops=None, matrices=None):
    """The whole call on host arrays.  crops / matrices: the buffers' contents
    before the call (what the call does not write must survive); default zeros.
    Returns (crops, matrices, s_per_face)."""
    pool = np.asarray(pool, np.uint8).reshape(-1)
    desc = np.asarray(desc, np.int64).reshape(-1, 3)
    rows = np.asarray(rows, np.float32).reshape(-1, 15)
    offsets = [int(v) for v in offsets]
    cap = rows.shape[0]
    q = default_template(size) if template is None else np.asarray(template, np.float32)
    shape = (cap, size, size, 3) if out == "u8" else (cap, 3, size, size)
    dtype = np.uint8 if out == "u8" else np.float32
    crops = np.zeros(shape, dtype) if crops is None else np.array(crops, dtype).reshape(shape)
    matrices = (np.zeros((cap, 6), np.float32) if matrices is None
                else np.array(matrices, np.float32).reshape(cap, 6))
    count = min(offsets[len(desc)], cap) if len(desc) else 0
    ss = []
    for r in range(count):
        image = slot_image(pool, desc, owner(offsets, r))
        f = fit(rows[r, 5:15], q, antialias)
        if image is None:
            f = Fit()
        v = sample(image, f, size) if f.s else np.zeros((size, size, 3), np.float32)
        crops[r] = finish(v, out, mean, std, bgr)
        matrices[r] = f.m
        ss.append(f.s)
    return crops, matrices, ss


# ------------------------------------------------------------------ test inputs
def similar(q, scale, theta, shift, rng=None, noise=0.0, about=(0.0, 0.0)):
    """Landmarks float32 [5, 2] whose best fit onto the template q has scale
    ~`scale` and rotation -theta; the template point `about` lands on `shift`."""
    c, s = np.cos(theta), np.sin(theta)
    src = np.asarray(q, np.float64) - np.asarray(about)
    if rng is not None:
        src = src + rng.normal(0.0, noise, src.shape)
    return ((src @ np.array([[c, s], [-s, c]])) / scale + np.asarray(shift)).astype(np.float32)


# ------------------------------------------------------------------ independent checks
def umeyama_svd(p, q):
    """Umeyama's least-squares similarity p -> q by SVD with the reflection
    guard; p, q float64 [5, 2].  Returns the 2 x 3 matrix."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    n = p.shape[0]
    mp, mq = p.mean(0), q.mean(0)
    dp, dq = p - mp, q - mq
    cov = dq.T @ dp / n
    U, d, Vt = np.linalg.svd(cov)
    D = np.ones(2)
    if np.linalg.det(cov) < 0:
        D[1] = -1.0
    R = U @ np.diag(D) @ Vt
    scale = (d * D).sum() / ((dp ** 2).sum() / n)
    M = np.zeros((2, 3))
    M[:, :2] = scale * R
    M[:, 2] = mq - scale * R @ mp
    return M


def warp_f64(image, M, size):
    """crop[y, x] = bilinear(image, M^-1 (x, y)) in float64, one sample per
    pixel, constant border 0; float64 [size, size, 3]."""
    ih, iw = image.shape[:2]
    inv = np.linalg.inv(np.vstack([M, [0.0, 0.0, 1.0]]))
    ys, xs = np.mgrid[0:size, 0:size].astype(np.float64)
    sx = inv[0, 0] * xs + inv[0, 1] * ys + inv[0, 2]
    sy = inv[1, 0] * xs + inv[1, 1] * ys + inv[1, 2]
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    wx, wy = (sx - x0)[..., None], (sy - y0)[..., None]
    pad = np.zeros((ih + 2, iw + 2, 3))
    pad[1:-1, 1:-1] = image

    def tap(yy, xx):
        return pad[np.clip(yy + 1, 0, ih + 1), np.clip(xx + 1, 0, iw + 1)]
    top = tap(y0, x0) * (1 - wx) + tap(y0, x0 + 1) * wx
    bot = tap(y0 + 1, x0) * (1 - wx) + tap(y0 + 1, x0 + 1) * wx
    return top * (1 - wy) + bot * wy
