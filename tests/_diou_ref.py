"""CPU restatement of the reference's diounms (utils/box_utils.py:450-526) in
numpy fp32, for tests/test_diou_nms.py.

Every operation is one fp32 numpy ufunc in the reference's order (no fused
multiply-add), so with beta1 == 1 the values are the reference's bit for bit.
Where the project departs from the reference, this follows the project:

* order: descending score, stable (ties by lower row index), NaN scores first,
  -0.0 == 0.0 -- the order of oracle/box_ref.nms_py;
* a pair whose value is NaN (a NaN coordinate, or two boxes that are the same
  point: d / c = 0 / 0) is not suppressed; the reference's IoU.le(overlap)
  would drop the later box;
* the decision is (double)value > thr, as the IoU kind's;
* beta1 != 1: u = (float)pow((double)(d / c), beta1);
* top_k <= 0 means no cut.

kind="iou" runs the same loop on inter / union alone, with torchvision's union
order (area_i + area_j) - inter: the project's IoU kind (finite boxes only:
torchvision's std::max / std::min treat a NaN operand differently).

diounms_c is the same loop in C (tests/_diou_ref.c, built with the host
compiler at first use) for the 24 000-row cases, which take 4-7 s per run in
numpy; tests/test_diou_nms.py checks that the two agree.
"""
import ctypes
import hashlib
import os
import subprocess
import tempfile
import threading

import numpy as np


def order_desc(scores):
    s = np.asarray(scores, np.float32).reshape(-1)
    nan = np.isnan(s)
    return np.lexsort((np.arange(len(s)), np.where(nan, np.float32(0), -s), ~nan))


_twin_lock = threading.Lock()
_twin_fn = None


def _twin():
    """tests/_diou_ref.c built with the host compiler at first use, into the
    temporary directory (nothing is written to the repository).  The first
    callers may be several threads (diounms_c runs in a pool) or several test
    processes: threads build under a lock, and every build goes to a file name
    of its own (mkstemp) that is renamed over the target once it is complete,
    so a reader only ever sees a whole library."""
    global _twin_fn
    with _twin_lock:
        if _twin_fn is not None:
            return _twin_fn
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_diou_ref.c")
        tag = hashlib.sha1(open(src, "rb").read()).hexdigest()[:12]
        tmpdir = tempfile.gettempdir()
        out = os.path.join(tmpdir, f"jabd_diou_ref_{os.getuid()}_{tag}.so")
        if not os.path.exists(out):
            fd, tmp = tempfile.mkstemp(prefix="jabd_diou_ref_", suffix=".so.part", dir=tmpdir)
            os.close(fd)
            try:
                subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-fPIC", "-shared",
                                       "-ffp-contract=off", "-fno-fast-math", "-o", tmp, src,
                                       "-lm"])
                os.replace(tmp, out)
            finally:
                if os.path.exists(tmp):
                    os.unlink(tmp)
        fn = ctypes.CDLL(out).diou_ref_nms
        fn.restype = ctypes.c_int64
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_double,
                       ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
        _twin_fn = fn
        return fn


def diounms_c(boxes, scores, overlap=0.5, top_k=0, beta1=1.0, kind="diou"):
    """diounms() through the C twin (tests/_diou_ref.c): same result, for the
    24k-row cases.  The call drops the GIL, so several run in threads."""
    assert kind in ("diou", "iou")
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    order = order_desc(scores)
    if top_k > 0:
        order = order[:top_k]
    ranked = np.ascontiguousarray(b[order])
    keep = np.empty(max(len(order), 1), np.int64)
    margin = ctypes.c_double(0.0)
    k = _twin()(ranked.ctypes.data, len(order), float(overlap), float(beta1),
                0 if kind == "iou" else 1, keep.ctypes.data, ctypes.byref(margin))
    assert k >= 0
    return order[keep[:k]].astype(np.int64), float(margin.value)


def diounms(boxes, scores, overlap=0.5, top_k=0, beta1=1.0, kind="diou"):
    """-> (keep int64 [K]: kept row indices in decreasing-score order,
           margin: the smallest |value - overlap| over every decision made;
           inf when no finite value was compared)."""
    assert kind in ("diou", "iou")
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    order = order_desc(scores)
    if top_k > 0:
        order = order[:top_k]
    x1, y1, x2, y2 = (np.ascontiguousarray(b[order, k]) for k in range(4))
    area = (x2 - x1) * (y2 - y1)
    two = np.float32(2)
    zero = np.float32(0)
    thr = float(overlap)
    idx = np.arange(len(order))
    keep = []
    margin = np.inf
    with np.errstate(all="ignore"):
        while idx.size:
            i = idx[0]
            keep.append(order[i])
            idx = idx[1:]
            if not idx.size:
                break
            xx1, yy1, xx2, yy2 = x1[idx], y1[idx], x2[idx], y2[idx]
            w = np.maximum(np.minimum(xx2, x2[i]) - np.maximum(xx1, x1[i]), zero)
            h = np.maximum(np.minimum(yy2, y2[i]) - np.maximum(yy1, y1[i]), zero)
            inter = w * h
            if kind == "iou":
                val = inter / ((area[i] + area[idx]) - inter)
            else:
                union = (area[idx] - inter) + area[i]
                dx = (x1[i] + x2[i]) / two - (xx1 + xx2) / two
                dy = (y1[i] + y2[i]) / two - (yy1 + yy2) / two
                d = dx * dx + dy * dy
                ex = np.maximum(xx2, x2[i]) - np.minimum(xx1, x1[i])
                ey = np.maximum(yy2, y2[i]) - np.minimum(yy1, y1[i])
                c = ex * ex + ey * ey
                u = d / c
                if beta1 != 1.0:
                    u = np.power(u.astype(np.float64), float(beta1)).astype(np.float32)
                val = inter / union - u
            assert val.dtype == np.float32
            v64 = val.astype(np.float64)
            fin = np.abs(v64[np.isfinite(v64)] - thr)
            if fin.size:
                margin = min(margin, float(fin.min()))
            idx = idx[~(v64 > thr)]          # NaN: not suppressed
    return np.asarray(keep, np.int64), margin
