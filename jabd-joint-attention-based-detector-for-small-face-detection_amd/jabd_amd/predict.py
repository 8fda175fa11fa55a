"""predict.py's detect_image (predict.py:115-196) as one device pipeline:
letterbox + preprocess_input (jabd_letterbox_f32) -> RetinaFace eval forward ->
decode + score filter + NMS (jabd_detect_f32) -> retinaface_correct_boxes +
pixel rescale (jabd_correct_boxes_f32).  Only the kept rows leave the device.
"""
import collections
import os

import numpy as np
import torch

from jabd_amd import functional as F
from jabd_amd import hipmodule, ops

# JABD_PREDICT_GRAPH=0: launch the forward + detect kernels one by one (A/B).
# The library initialises its workspaces with its own fill kernel (fill.hip),
# not hipMemsetAsync: with captured memset nodes, a replay that followed an
# eager detect launched after the capture read a wrong fill pattern and
# faulted the device (ROCm 7, tools/graph_check.py --between det); with kernel
# nodes only, interleaved eager calls and replays agree bit for bit.
PREDICT_GRAPH = os.environ.get("JABD_PREDICT_GRAPH", "1") != "0"
# graphs kept per module (least recently used dropped first): each holds a
# private memory pool with the whole activation set of its shape
GRAPH_CACHE = int(os.environ.get("JABD_PREDICT_GRAPHS", "4"))


class GraphedDetect:
    """The eval forward + decode / filter / NMS of one input shape, captured
    once as a HIP graph (torch.cuda.CUDAGraph) and replayed per image: a bs1
    predict step is ~170 launches (R50) whose host-side dispatch (ctypes +
    Python per launch) exceeded their GPU time (predict.py get_FPS,
    predict.py:253-333).  The input is copied into the graph's static input;
    the outputs are the graph's static (rows, n_keep) buffers, valid until
    the next replay.  The forward runs with split-K on (functional.split_k),
    as the eager bs1 predict path.  Invalid once the model's packs may have
    changed (hipmodule generation)."""

    def __init__(self, net, shape, priors, variances, conf_thres, nms_thres, device,
                 nms_kind="greedynms", beta1=1.0, top_k=0, sigma=0.5, soft_offset=0.0):
        self.net, self.gen = net, hipmodule.generation()
        self.x = torch.zeros(shape, dtype=torch.float32, device=device)
        self.pri = priors
        self.args = (variances, conf_thres, nms_thres)
        self.rule = (nms_kind, float(beta1), int(top_k))
        self.soft = (float(sigma), float(soft_offset))   # read by the "softnms" kind only
        cur = torch.cuda.current_stream(device)
        side = torch.cuda.Stream(device=device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):   # packs, workspaces and lazy state first
            for _ in range(2):
                self._body()
        cur.wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self._body()

    def _body(self):
        with torch.no_grad(), F.split_k():
            loc, conf, landm = self.net(self.x)
            v, ct, nt = self.args
            kind, beta1, top_k = self.rule
            sigma, soft_offset = self.soft
            return ops.detect(loc, conf, landm, self.pri, v, ct, nt, nms_kind=kind, beta1=beta1,
                              top_k=top_k, sigma=sigma, soft_offset=soft_offset)

    def __call__(self, x):
        self.x.copy_(x)
        self.graph.replay()
        return self.out


def graphed_detect(net, x, priors, variances, conf_thres=0.5, nms_thres=0.3,
                   nms_kind="greedynms", beta1=1.0, top_k=0, sigma=0.5, soft_offset=0.0):
    """ops.detect(*net(x), ...) for a batch of the shape of x, through a HIP
    graph cached on the module per (shape, device, thresholds, priors,
    suppression rule); rebuilt when the module's eval packs may have changed.
    The rule (kind, beta1, top_k; for "softnms": sigma, soft_offset, top_k) is
    baked into the captured launches, so it is part of the key: a graph
    captured for one rule never serves another."""
    soft = ops.is_soft_kind(nms_kind)
    if soft:
        # the Soft-NMS ignores nms_thres and beta1: one graph whatever came with them
        sigma, soft_offset = ops._soft_args(sigma, soft_offset)
        rule = ("soft", sigma, soft_offset, max(int(top_k), 0))
        nms_thres = 0.0
    else:
        code = ops._kind_code(nms_kind, beta1)
        # the IoU kind ignores beta1: one graph whatever value came with it
        rule = (code, float(beta1) if code else 1.0, max(int(top_k), 0))
    key = (tuple(x.shape), str(x.device), float(variances[0]), float(variances[1]),
           float(conf_thres), float(nms_thres), priors.data_ptr()) + rule
    cache = net.__dict__.setdefault("_jabd_graphs", collections.OrderedDict())
    g = cache.get(key)
    if g is None or g.gen != hipmodule.generation() or g.pri is not priors:
        cache.pop(key, None)
        while len(cache) >= max(1, GRAPH_CACHE):
            cache.popitem(last=False)
        if soft:
            g = GraphedDetect(net, tuple(x.shape), priors, variances, conf_thres, nms_thres,
                              x.device, nms_kind, beta1, top_k, sigma=sigma,
                              soft_offset=soft_offset)
        else:   # exactly the arguments of the hard kinds
            g = GraphedDetect(net, tuple(x.shape), priors, variances, conf_thres, nms_thres,
                              x.device, nms_kind, beta1, top_k)
        cache[key] = g
    cache.move_to_end(key)
    return g(x)


def _use_graph(net, shape, fixed_shape):
    """Graph only a shape that will recur: letterboxed inputs (one fixed
    shape), or an image size this module has already run once.  A folder of
    mixed-size images (letterbox_image=False) stays on the eager path instead
    of paying two warm-up forwards, a capture and a private pool per size."""
    if not PREDICT_GRAPH or net.training:
        return False
    if fixed_shape:
        return True
    seen = net.__dict__.setdefault("_jabd_seen_shapes", collections.OrderedDict())
    hit = shape in seen
    seen[shape] = True
    seen.move_to_end(shape)
    while len(seen) > 64:
        seen.popitem(last=False)
    return hit


def detect_image(net, image, input_shape, cfg, confidence=0.5, nms_iou=0.3,
                 letterbox_image=True, device="cuda", nms_kind="greedynms", beta1=1.0, top_k=0,
                 sigma=0.5, soft_offset=0.0):
    """image: RGB HWC array (uint8 or float32), as predict.py's np.array(image,
    np.float32).  input_shape = (H, W) of the network input (used only when
    letterbox_image; otherwise the image's own size, as the reference).
    Returns numpy float32 [K, 15] (x1, y1, x2, y2, score, 5 landmark xy) in image
    pixels, NMS order; [] when nothing survives (the reference returns early).
    nms_kind "greedynms" (IoU) or "diounms" with its beta1; top_k > 0 keeps
    only the top_k best-scored candidates before suppression (ops.detect).
    nms_kind "softnms" (alias "softernms"): Gaussian Soft-NMS with `sigma` and
    `soft_offset`; nms_iou and beta1 are ignored and the rows carry their
    decayed scores, in the Soft-NMS's result order.  soft_offset defaults to
    0, not softer_nms's pixel +1: suppression runs on the normalised decode
    output, where +1 would make every pair overlap."""
    from utils.anchors import Anchors
    img = torch.from_numpy(np.ascontiguousarray(np.asarray(image, np.float32))).to(device)
    ih, iw = int(img.shape[0]), int(img.shape[1])
    H, W = (int(input_shape[0]), int(input_shape[1])) if letterbox_image else (ih, iw)
    x = ops.letterbox(img, (W, H), mean=(104.0, 117.0, 123.0))   # [1, 3, H, W]
    priors = Anchors(cfg, image_size=(H, W)).get_anchors().to(device).float().contiguous()
    with torch.no_grad():
        if _use_graph(net, (H, W, str(device)), letterbox_image):
            priors = _cached_priors(net, cfg, H, W, device, priors)
            rows, n_keep = graphed_detect(net, x, priors, cfg["variance"], confidence, nms_iou,
                                          nms_kind, beta1, top_k, sigma, soft_offset)
        else:
            with F.split_k():
                loc, conf, landm = net(x)
            rows, n_keep = ops.detect(loc, conf, landm, priors, cfg["variance"], confidence,
                                      nms_iou, nms_kind=nms_kind, beta1=beta1, top_k=top_k,
                                      sigma=sigma, soft_offset=soft_offset)
        k = int(n_keep[0].item())
        if k == 0:
            return []
        det = rows[0, :k].contiguous()
        ops.correct_boxes(det, (H, W), (ih, iw), letterbox=letterbox_image, to_pixels=True)
    return det.cpu().numpy()


def _pinned(stash, slot, nbytes):
    """Pinned uint8 buffer `slot` of a call's staging set, grown when too small."""
    buf = stash.get(slot)
    if buf is None or buf.numel() < nbytes:
        buf = stash[slot] = torch.empty(max(nbytes, 1), dtype=torch.uint8, pin_memory=True)
    return buf


def detect_images(net, images, input_shape, cfg, batch=8, max_det=750, confidence=0.5,
                  nms_iou=0.3, device="cuda", nms_kind="greedynms", beta1=1.0, top_k=0,
                  sigma=0.5, soft_offset=0.0):
    """detect_image(..., letterbox_image=True) for many images of any sizes at
    batch throughput: predict.py's dir_predict, video and get_map_txt loops.
    images: an iterable of RGB HWC uint8 arrays (anything np.asarray turns into
    one; another dtype raises TypeError, another shape or an image whose
    letterbox collapses ValueError, before that chunk's device work).  It is
    consumed `batch` images at a time, so a generator over a folder never holds
    the folder.  Returns a list with one numpy float32 [K_i, 15] per image, in
    order: the rows detect_image returns for that image (image pixels, NMS
    order), cut to the first max_det (max_det <= 0: all).  An image without a
    detection gives an array of shape (0, 15), not detect_image's [].

    Per chunk: the slot table and the images' bytes go to the device in one
    non-blocking copy from pinned memory, ops.letterbox_batch fills `batch`
    slots (the last chunk is padded with empty slots, so one HIP graph of the
    shape (batch, 3, H, W) serves every chunk and every later call), the
    forward + ops.detect run as in detect_image, ops.batch_collect brings each
    slot's rows to its image's pixels, and the offsets with the first
    min(batch * max_det, batch * A) rows come back in one non-blocking copy
    followed by an event.  Chunks are pipelined two deep (two staging and two
    result buffers): chunk c + 1 is packed and enqueued before chunk c's event
    is waited on, and that wait is the chunk's only host synchronisation
    (max_det <= 0: one more, for the rows)."""
    return _detect_chunks("detect_images", None, net, images, input_shape, cfg, batch, max_det,
                          confidence, nms_iou, device, nms_kind, beta1, top_k, sigma, soft_offset)


def _detect_chunks(name, extra, net, images, input_shape, cfg, batch, max_det, confidence,
                   nms_iou, device, nms_kind, beta1, top_k, sigma, soft_offset):
    """The chunk pipeline of detect_images (its docstring).  extra: None, or
    the private hook of extract_faces, an object with
      enqueue(pool, table, out, offsets) -> device uint8 1-D tensor
        called behind the chunk's ops.batch_collect with the chunk's device
        byte pool and slot table and the collected rows [cap, 15] and offsets
        [batch + 1]; what it returns is downloaded into a pinned buffer of its
        own by one more non-blocking copy in front of the chunk's event, so the
        chunk still has one host synchronisation;
      finish(host, rows, offs, n) -> list of n per-image results
        called behind that wait with the downloaded bytes (numpy uint8), the
        chunk's host rows and offsets and its number of images; its results
        replace the per-image rows."""
    import itertools
    batch = int(batch)
    if batch < 1:
        raise ValueError(f"{name}: batch must be at least 1, got {batch}")
    H, W = _pair("input_shape", input_shape)
    if H < 1 or W < 1:
        raise ValueError(f"{name}: bad input shape {input_shape!r}")
    if ops.is_soft_kind(nms_kind):
        ops._soft_args(sigma, soft_offset)
    else:
        ops._kind_code(nms_kind, beta1)
    max_det = max(int(max_det), 0)
    it = iter(images)
    head = batch * 24                      # the slot table leads the staging buffer
    stage, result, side = {}, {}, {}
    state = {}

    def setup():
        priors = _priors_for(net, cfg, H, W, device)
        A = priors.shape[0]
        state.update(priors=priors, A=A, cap=batch * (min(max_det, A) if max_det else A),
                     graph=_use_graph(net, (H, W, str(device)), True))

    def enqueue(chunk, first, slot):
        arrs, desc, total = ops._pack_arrays(name, chunk, (W, H), first)
        buf = _pinned(stage, slot, head + total)
        host = buf.numpy()
        table = host[:head].view(np.int64).reshape(batch, 3)
        table[...] = 0                     # the padding: empty slots
        table[:len(arrs)] = desc
        for a, (off, _, _) in zip(arrs, desc):
            host[head + off:head + off + a.size] = a.reshape(-1)
        if not state:
            setup()
        A, cap = state["A"], state["cap"]
        dev = buf[:head + total].to(device, non_blocking=True)
        table = dev[:head].view(torch.int64).view(batch, 3)
        x = ops.letterbox_batch(dev[head:], table, (W, H), fill=84.0,
                                mean=(104.0, 117.0, 123.0))
        if state["graph"]:
            rows, n_keep = graphed_detect(net, x, state["priors"], cfg["variance"], confidence,
                                          nms_iou, nms_kind, beta1, top_k, sigma, soft_offset)
        else:
            with F.split_k():
                loc, conf, landm = net(x)
            rows, n_keep = ops.detect(loc, conf, landm, state["priors"], cfg["variance"],
                                      confidence, nms_iou, nms_kind=nms_kind, beta1=beta1,
                                      top_k=top_k, sigma=sigma, soft_offset=soft_offset)
        # offsets and rows share one buffer: one copy brings both back
        tail = (batch + 1) * 8
        res = torch.empty(tail + cap * 60, dtype=torch.uint8, device=dev.device)
        offsets = res[:tail].view(torch.int64)
        out = res[tail:].view(torch.float32).view(cap, 15)
        ops.batch_collect(rows, n_keep, table, (H, W), max_det=max_det, out=out, offsets=offsets)
        back = res if max_det else res[:tail]
        hres = _pinned(result, slot, back.numel())[:back.numel()]
        hres.copy_(back, non_blocking=True)
        hside = None
        if extra is not None:
            more = extra.enqueue(dev[head:], table, out, offsets)
            hside = _pinned(side, slot, more.numel())[:more.numel()]
            hside.copy_(more, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        return len(arrs), hres, out, done, hside

    def finish(job):
        n, hres, out, done, hside = job
        done.synchronize()
        host = hres.numpy()
        tail = (batch + 1) * 8
        offs = host[:tail].view(np.int64)
        if max_det:
            rows = host[tail:].view(np.float32).reshape(-1, 15)
        else:                              # no cap: the rows that exist, one more wait
            rows = out[:int(offs[n])].cpu().numpy()
        if extra is not None:
            return extra.finish(hside.numpy(), rows, offs, n)
        return [rows[offs[i]:offs[i + 1]].copy() for i in range(n)]

    results, pending, first = [], None, 0
    with torch.no_grad():
        for c in itertools.count():
            chunk = list(itertools.islice(it, batch))
            if not chunk:
                break
            job = enqueue(chunk, first, c & 1)
            first += len(chunk)
            if pending is not None:
                results += finish(pending)
            pending = job
        if pending is not None:
            results += finish(pending)
    return results


def _crop_layout(size, kind):
    """(shape, numpy dtype, bytes) of one crop."""
    if kind == 0:
        return (size, size, 3), np.uint8, size * size * 3
    return (3, size, size), np.float32, size * size * 12


def align_faces(image, dets, size=112, template=None, antialias=True, out="u8", mean=127.5,
                std=127.5, bgr=False, device="cuda"):
    """Aligned crops of one image's detections (ops.align_faces).  image: RGB
    HWC uint8 array; dets: the [K, 15] rows any of the detect functions
    returned for it (image pixels), or [].  Returns numpy (crops, matrices):
    crops uint8 [K, size, size, 3], or float32 [K, 3, size, size] with
    out="f32"; matrices float32 [K, 6].  [] or K == 0 gives arrays of length 0
    without device work.  The other arguments are ops.align_faces'."""
    size, _, kind, _, _ = ops._align_args("align_faces", size, template, out, mean, std)
    shape, dtype, _ = _crop_layout(size, kind)
    arr = ops._image_u8("align_faces", 0, image)
    rows = np.asarray(dets, np.float32)
    if rows.size == 0:
        return np.zeros((0,) + shape, dtype), np.zeros((0, 6), np.float32)
    if rows.ndim != 2 or rows.shape[1] != 15:
        raise ValueError(f"align_faces: dets must be [K, 15], got {rows.shape}")
    K = rows.shape[0]
    pool = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)).to(device)
    desc = torch.tensor([[0, arr.shape[0], arr.shape[1]]], dtype=torch.int64, device=device)
    offsets = torch.tensor([0, K], dtype=torch.int64, device=device)
    crops, matrices = ops.align_faces(pool, desc, torch.from_numpy(np.ascontiguousarray(rows))
                                      .to(device), offsets, size=size, template=template,
                                      antialias=antialias, out=out, mean=mean, std=std, bgr=bgr)
    return crops.cpu().numpy(), matrices.cpu().numpy()


class _AlignHook:
    """extract_faces' side of _detect_chunks: ops.align_faces on the chunk's
    own device pool and collected rows, crops and matrices packed into one
    device buffer (the matrices lead, so both stay aligned)."""

    def __init__(self, size, template, antialias, out, mean, std, bgr):
        self.size, _, self.kind, _, _ = ops._align_args("extract_faces", size, template, out,
                                                        mean, std)
        self.kw = dict(size=self.size, template=template, antialias=antialias, out=out,
                       mean=mean, std=std, bgr=bgr)

    def enqueue(self, pool, table, out, offsets):
        cap = self.cap = out.shape[0]             # the same for every chunk of a call
        shape, _, nbytes = _crop_layout(self.size, self.kind)
        lead = -(-cap * 24 // 16) * 16            # the crops start on a 16-byte boundary
        buf = torch.empty(lead + cap * nbytes, dtype=torch.uint8, device=out.device)
        matrices = buf[:cap * 24].view(torch.float32).view(cap, 6)
        crops = buf[lead:]
        crops = (crops if self.kind == 0 else crops.view(torch.float32)).view((cap,) + shape)
        ops.align_faces(pool, table, out, offsets, crops=crops, matrices=matrices, **self.kw)
        return buf

    def finish(self, host, rows, offs, n):
        cap = self.cap
        shape, dtype, _ = _crop_layout(self.size, self.kind)
        matrices = host[:cap * 24].view(np.float32).reshape(cap, 6)
        crops = host[-(-cap * 24 // 16) * 16:].view(dtype).reshape((cap,) + shape)
        return [(rows[offs[i]:offs[i + 1]].copy(), crops[offs[i]:offs[i + 1]].copy(),
                 matrices[offs[i]:offs[i + 1]].copy()) for i in range(n)]


def extract_faces(net, images, input_shape, cfg, size=112, batch=8, max_det=750, confidence=0.5,
                  nms_iou=0.3, device="cuda", nms_kind="greedynms", beta1=1.0, top_k=0,
                  sigma=0.5, soft_offset=0.0, template=None, antialias=True, out="u8",
                  mean=127.5, std=127.5, bgr=False):
    """detect_images plus the aligned crop of every detection, made on the
    device from the chunk's own byte pool and collected rows before the pool
    is released (ops.align_faces; size, template, antialias, out, mean, std,
    bgr are its arguments, the others detect_images').  Returns one (rows,
    crops, matrices) per image, in order: rows exactly detect_images' [K_i, 15],
    crops uint8 [K_i, size, size, 3] (out="f32": float32 [K_i, 3, size, size]),
    matrices float32 [K_i, 6].  The chunk pipeline is detect_images' own: the
    crops and matrices of a chunk come back in a second pinned buffer by a
    second non-blocking copy in front of the chunk's one event, so the chunk
    still synchronises once.  That buffer holds batch * max_det crops whatever
    the number of faces, size * size * 3 bytes each (out="f32": four times
    that), twice on the host and up to twice on the device; max_det <= 0 would
    size it by the number of anchors and raises ValueError."""
    if int(max_det) <= 0:
        raise ValueError(f"extract_faces: max_det must be positive, got {max_det!r} (the crop "
                         "buffer holds batch * max_det crops)")
    hook = _AlignHook(size, template, antialias, out, mean, std, bgr)
    return _detect_chunks("extract_faces", hook, net, images, input_shape, cfg, batch, max_det,
                          confidence, nms_iou, device, nms_kind, beta1, top_k, sigma, soft_offset)


def _tta_passes(net, img, cfg, scales, flip, confidence, nms_iou, device, nms_kind, beta1, top_k):
    """The passes of detect_image_tta: (rows [A, 15], n_keep [1], (H, W),
    mirrored) one after the other, each valid until the next is asked for (a
    graphed pass hands out its graph's static buffers)."""
    from utils.anchors import Anchors
    ih, iw = int(img.shape[0]), int(img.shape[1])
    plan = []
    for s in scales:
        H = 32 * max(1, round(ih * float(s) / 32))
        W = 32 * max(1, round(iw * float(s) / 32))
        priors = Anchors(cfg, image_size=(H, W)).get_anchors().to(device).float().contiguous()
        graph = _use_graph(net, (H, W, str(device)), False)
        if graph:
            priors = _cached_priors(net, cfg, H, W, device, priors)
        plan.append((H, W, priors, graph))
    total = sum(p[2].shape[0] for p in plan) * (2 if flip else 1)

    def run():
        for H, W, priors, graph in plan:
            x = ops.letterbox(img, (W, H), mean=(104.0, 117.0, 123.0))   # [1, 3, H, W]
            for mirrored in ((False, True) if flip else (False,)):
                # the canvas is mirrored, not the image: 1 - x un-mirrors it exactly
                xin = x.flip(-1).contiguous() if mirrored else x
                if graph:
                    rows, n_keep = graphed_detect(net, xin, priors, cfg["variance"], confidence,
                                                  nms_iou, nms_kind, beta1, top_k)
                else:
                    with F.split_k():
                        loc, conf, landm = net(xin)
                    rows, n_keep = ops.detect(loc, conf, landm, priors, cfg["variance"],
                                              confidence, nms_iou, nms_kind=nms_kind, beta1=beta1,
                                              top_k=top_k)
                yield rows[0], n_keep, (H, W), mirrored
    return total, run()


def detect_image_tta(net, image, cfg, scales=(0.5, 1.0, 1.5, 2.0), flip=True, confidence=0.5,
                     nms_iou=0.3, vote_thres=0.4, min_votes=1, max_out=750, device="cuda",
                     nms_kind="greedynms", beta1=1.0, top_k=0, _merged_hook=None):
    """Multi-scale / flip test-time detection with box voting, on the device.
    image: RGB HWC array as detect_image takes it.  For every scale s the image
    is letterboxed to a network input of H = 32 max(1, round(ih s / 32)), W
    likewise, and detected (detect_image's forward + decode + filter + NMS with
    `confidence`, `nms_iou`, `nms_kind`, `beta1`, `top_k`), plain and, with
    `flip`, on the mirrored canvas.  Each pass's rows are un-mirrored, brought
    to image pixels and appended to one merged list on the device
    (ops.tta_collect); ops.box_vote (IoU >= vote_thres with the pixel +1,
    min_votes, max_out) then replaces each cluster of overlapping rows by one
    row: the score-weighted mean box with the best member's score and
    landmarks.  Returns numpy float32 [K, 15] in image pixels, descending
    score; [] when nothing survives.  The call synchronises with the device
    once, reading the number of result rows (max_out <= 0: once more for the
    rows).  A shape recurs in a HIP graph as in detect_image without
    letterbox_image: from the second call with the same image size on.
    _merged_hook(merged, offsets), if given, sees the device buffers the
    passes were collected into just before the vote (offsets[-1] rows are
    valid); the tests read the voting step's input through it."""
    img = torch.from_numpy(np.ascontiguousarray(np.asarray(image, np.float32))).to(device)
    ih, iw = int(img.shape[0]), int(img.shape[1])
    scales = tuple(scales)
    if not scales:
        raise ValueError("detect_image_tta: no scales")
    ops._vote_args(vote_thres, 1.0, min_votes)
    with torch.no_grad():
        cap, passes = _tta_passes(net, img, cfg, scales, flip, confidence, nms_iou, device,
                                  nms_kind, beta1, top_k)
        n_pass = len(scales) * (2 if flip else 1)
        merged = torch.empty((cap, 15), dtype=torch.float32, device=img.device)
        offsets = torch.zeros(n_pass + 1, dtype=torch.int64, device=img.device)
        for p, (rows, n_keep, shape, mirrored) in enumerate(passes):
            ops.tta_collect(rows, n_keep, merged, offsets, p, shape, (ih, iw), letterbox=True,
                            flip=mirrored)
        if _merged_hook is not None:
            _merged_hook(merged, offsets)
        out, n_out, _, _ = ops.box_vote(merged.unsqueeze(0), vote_threshold=vote_thres,
                                        offset=1.0, min_votes=min_votes, max_out=max_out,
                                        n_valid=offsets[n_pass:])
        if max_out > 0:
            # the rows that can be asked for travel with the count: one synchronisation
            bound = min(int(max_out), cap)
            host = torch.empty((bound, 15), dtype=torch.float32, pin_memory=True)
            host.copy_(out[0, :bound], non_blocking=True)
            k = int(n_out[0].item())
            return host[:k].numpy().copy() if k else []
        k = int(n_out[0].item())
        if k == 0:
            return []
        return out[0, :k].cpu().numpy()


def _pair(name, v):
    """(a, b) from an int or a pair of ints."""
    try:
        a, b = (v, v) if isinstance(v, (int, np.integer)) else v
        if int(a) != a or int(b) != b:
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be an int or a pair of ints, got {v!r}") from None
    return int(a), int(b)


def tile_plan(ih, iw, tile=(1024, 1024), overlap=(128, 128)):
    """The tile origins of sliced detection: int32 [T, 2] = (y0, x0),
    row-major (y outer).  Per axis of length L with tile t and overlap o:
    stride = t - o, n = 1 if L <= t else ceil((L - t) / stride) + 1, origin k =
    min(k * stride, L - t) (0 when L <= t): the tiles cover the axis, the last
    is flush with its end, and neighbours share at least o pixels.  tile sides
    must be positive multiples of 32 (the network's stride) and 0 <= o < t;
    anything else raises ValueError."""
    th, tw = _pair("tile", tile)
    oy, ox = _pair("overlap", overlap)
    if int(ih) != ih or int(iw) != iw or ih < 1 or iw < 1:
        raise ValueError(f"tile_plan: bad image size {ih!r} x {iw!r}")
    axes = []
    for L, t, o in ((int(ih), th, oy), (int(iw), tw, ox)):
        if t < 32 or t % 32:
            raise ValueError(f"tile_plan: tile side {t} is no positive multiple of 32")
        if not 0 <= o < t:
            raise ValueError(f"tile_plan: overlap {o} outside [0, {t})")
        stride = t - o
        n = 1 if L <= t else -(-(L - t) // stride) + 1
        axes.append([min(k * stride, max(L - t, 0)) for k in range(n)])
    return np.array([(y, x) for y in axes[0] for x in axes[1]], np.int32).reshape(-1, 2)


# rows the merged list of detect_image_tiled keeps at most (60 bytes each, and
# the merge step's workspace grows with it); later rows are dropped
TILE_MERGE_ROWS = 1 << 17


def detect_image_tiled(net, image, cfg, tile=(1024, 1024), overlap=128, batch=8, border=1.0,
                       full_pass=True, merge="nms", confidence=0.5, nms_iou=0.3,
                       vote_thres=0.4, min_votes=1, max_out=750, device="cuda",
                       nms_kind="greedynms", beta1=1.0, top_k=0, _merged_hook=None):
    """Sliced detection of a large image, on the device.  image: RGB HWC array,
    uint8 (uploaded as uint8) or float32.  The image is cut into overlapping
    tiles (tile_plan(ih, iw, tile, overlap)); the tiles go through the network
    in chunks of `batch` (ops.tile_gather -> forward -> ops.detect with
    `confidence`, `nms_iou`, `nms_kind`, `beta1`, `top_k`), the last chunk
    padded to `batch` slots, so one HIP graph of the shape (batch, 3, th, tw)
    serves every chunk and every later image whatever its size.  Each chunk's
    rows join one merged list in image pixels (ops.tile_collect): a box within
    `border` tile pixels of a tile side inside the image is dropped there (the
    tile cut the face; the overlap lets a neighbour see it whole).  With
    `full_pass`, the whole image letterboxed to one tile joins the list as the
    last pass (ops.tta_collect): it finds the faces larger than the overlap,
    which every tile cut.  The list is then merged across tiles: merge="nms"
    runs ops.batched_nms with `nms_iou` and the rule of `nms_kind` / `beta1` on
    the pixel rows, merge="vote" ops.box_vote (`vote_thres`, pixel +1,
    `min_votes`); at most max_out rows are returned.  nms_kind "softnms" raises
    ValueError: decayed scores from different tiles do not compose.  The merged
    list keeps at most TILE_MERGE_ROWS rows.  Returns numpy float32 [K, 15] in
    image pixels, descending score; [] when nothing survives.  The call
    synchronises with the device once, reading the number of result rows
    (max_out <= 0: once more for the rows).  _merged_hook(merged, offsets), if
    given, sees the device buffers just before the merge (offsets[-1] rows are
    valid; offsets[c + 1] closes chunk c, the last entry the full pass)."""
    if ops.is_soft_kind(nms_kind):
        raise ValueError("detect_image_tiled: nms_kind 'softnms' is not supported: decayed "
                         "scores from different tiles do not compose")
    kind = ops._kind_code(nms_kind, beta1)
    if merge not in ("nms", "vote"):
        raise ValueError(f"detect_image_tiled: merge must be 'nms' or 'vote', got {merge!r}")
    if merge == "vote":
        ops._vote_args(vote_thres, 1.0, min_votes)
    batch = int(batch)
    if batch < 1:
        raise ValueError(f"detect_image_tiled: batch must be at least 1, got {batch}")
    th, tw = _pair("tile", tile)
    arr = np.asarray(image)
    if arr.dtype != np.uint8:
        arr = np.asarray(arr, np.float32)
    if arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError(f"detect_image_tiled: image must be [H, W, 3], got {arr.shape}")
    ih, iw = int(arr.shape[0]), int(arr.shape[1])
    plan = tile_plan(ih, iw, (th, tw), overlap)
    T = plan.shape[0]
    n_chunks = -(-T // batch)
    # every chunk gathers `batch` tiles: the padding repeats the last origin
    padded = np.concatenate([plan, np.repeat(plan[-1:], n_chunks * batch - T, 0)])
    img = torch.from_numpy(np.ascontiguousarray(arr)).to(device)
    origins = torch.from_numpy(padded).to(device)
    mean = (104.0, 117.0, 123.0)
    priors = _priors_for(net, cfg, th, tw, device)
    A = priors.shape[0]
    n_pass = n_chunks + (1 if full_pass else 0)
    cap = max(1, min((T + (1 if full_pass else 0)) * A, TILE_MERGE_ROWS))
    graph = _use_graph(net, (th, tw, str(device)), True)

    def run(x):
        if graph:
            return graphed_detect(net, x, priors, cfg["variance"], confidence, nms_iou,
                                  nms_kind, beta1, top_k)
        with F.split_k():
            loc, conf, landm = net(x)
        return ops.detect(loc, conf, landm, priors, cfg["variance"], confidence, nms_iou,
                          nms_kind=nms_kind, beta1=beta1, top_k=top_k)
    with torch.no_grad():
        merged = torch.empty((cap, 15), dtype=torch.float32, device=img.device)
        offsets = torch.zeros(n_pass + 1, dtype=torch.int64, device=img.device)
        for c in range(n_chunks):
            org = origins[c * batch:(c + 1) * batch]
            rows, n_keep = run(ops.tile_gather(img, org, (th, tw), fill=84.0, mean=mean))
            ops.tile_collect(rows, n_keep, org[:min(batch, T - c * batch)], merged, offsets, c,
                             (th, tw), (ih, iw), border=border)
        if full_pass:
            rows, n_keep = run(ops.letterbox(img.float(), (tw, th), mean=mean))
            ops.tta_collect(rows[0], n_keep, merged, offsets, n_chunks, (th, tw), (ih, iw),
                            letterbox=True, flip=False)
        if _merged_hook is not None:
            _merged_hook(merged, offsets)
        bound = min(int(max_out), cap) if max_out > 0 else cap
        if merge == "vote":
            out, n_out, _, _ = ops.box_vote(merged.unsqueeze(0), vote_threshold=vote_thres,
                                            offset=1.0, min_votes=min_votes, max_out=max_out,
                                            n_valid=offsets[n_pass:])
            out = out[0, :bound]
        else:
            keep, n_out = ops.batched_nms(merged.unsqueeze(0),
                                          merged[:, 4].contiguous().unsqueeze(0), nms_iou,
                                          n_valid=offsets[n_pass:], kind=nms_kind,
                                          beta1=beta1 if kind else 1.0)
            # entries of keep beyond n_out are not written: any valid row stands in
            out = merged.index_select(0, keep[0, :bound].clamp_(0, cap - 1))
        if max_out > 0:
            # the rows that can be asked for travel with the count: one synchronisation
            host = torch.empty((bound, 15), dtype=torch.float32, pin_memory=True)
            host.copy_(out, non_blocking=True)
            k = min(int(n_out[0].item()), bound)
            return host[:k].numpy().copy() if k else []
        k = int(n_out[0].item())
        if k == 0:
            return []
        return out[:k].cpu().numpy()


def _priors_key(cfg, H, W, device):
    return (H, W, str(device), repr(cfg.get("min_sizes")), repr(cfg.get("steps")),
            bool(cfg.get("clip", False)))


def _cached_priors(net, cfg, H, W, device, priors):
    """One priors tensor per (input size, device, anchor cfg) on the module
    (the graph keys on its storage).  The priors are a function of exactly
    these keys (utils/anchors.py:8-42), so another cfg on the same net gets
    its own tensor (and graph) instead of stale priors."""
    cache = net.__dict__.setdefault("_jabd_priors", {})
    key = _priors_key(cfg, H, W, device)
    p = cache.get(key)
    if p is None or p.shape != priors.shape:
        p = cache[key] = priors
    return p


def _priors_for(net, cfg, H, W, device):
    """_cached_priors for a shape that recurs by construction (the tile): the
    anchors are generated once per key, not per call."""
    p = net.__dict__.setdefault("_jabd_priors", {}).get(_priors_key(cfg, H, W, device))
    if p is None:
        from utils.anchors import Anchors
        p = Anchors(cfg, image_size=(H, W)).get_anchors().to(device).float().contiguous()
        p = _cached_priors(net, cfg, H, W, device, p)
    return p
