"""Time predict.detect_images against a plain loop of predict.detect_image
over the same images, and its two kernels on their own.

    python tools/detect_images_time.py [--input 1280] [--images 64] [--rounds 3]
                                       [--batches 1,8,32] [--confs 0.6,0.5]

Model: JABD-MNv3 (cfg_mnet) with weights_init.  Images: --images seeded uint8
images, 1024 wide, heights drawn from 600..1500.  Confidence 0.6 is the
forward-bound end (random weights score just above 0.5: no rows), 0.5 the
worst-case row count.  Per confidence the loop and every batch size alternate
in the same run, --rounds times after one untimed pass of each (graphs warm);
the clock is the host's around work that ends in a device synchronise.  The
kernels are timed with HIP events around --reps back-to-back calls, at batch
8, and set beside their algorithmic bytes and the 8 TB/s floor.  One JSON line
per figure."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "jabd-joint-attention-based-detector-for-small-face-detection_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM = 8.0e12   # bytes/s, the floor the byte counts are set beside


def make_images(n, seed=0):
    rng = np.random.default_rng(seed)
    heights = rng.integers(600, 1501, n)
    return [rng.integers(0, 256, (int(h), 1024, 3), dtype=np.uint8) for h in heights]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def events(fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", type=int, default=1280)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--confs", default="0.6,0.5")
    args = ap.parse_args()
    if args.rounds < 1 or args.images < 1 or args.reps < 1:
        ap.error("--rounds, --images and --reps must be at least 1")
    from jabd_amd import ops
    from jabd_amd.predict import detect_image, detect_images
    from nets.retinaface_r import RetinaFace
    from nets.retinaface_training import weights_init
    from utils.config import cfg_mnet
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    net = RetinaFace(cfg=cfg_mnet, mode="eval")
    weights_init(net)
    net = net.eval().to(dev)
    shape = (args.input, args.input)
    images = make_images(args.images)
    batches = [int(b) for b in args.batches.split(",")]
    src_bytes = sum(im.size for im in images)

    for conf in (float(c) for c in args.confs.split(",")):
        def loop():
            return [detect_image(net, im, shape, cfg_mnet, confidence=conf, device=dev)
                    for im in images]
        runs = {"loop": loop}
        for b in batches:
            runs[f"batch{b}"] = (lambda b=b: detect_images(net, images, shape, cfg_mnet, batch=b,
                                                           confidence=conf, device=dev))
        rows = {}
        for name, fn in runs.items():                            # untimed: captures, pools
            out = fn()
            rows[name] = int(sum(len(o) for o in out))
        secs = {name: [] for name in runs}
        for _ in range(args.rounds):
            for name, fn in runs.items():
                secs[name].append(timed(fn)[0])
        for name in runs:
            s = np.asarray(secs[name])
            print(json.dumps({
                "what": "images_per_s", "path": name, "input": args.input, "confidence": conf,
                "images": len(images), "source_bytes": src_bytes, "rounds": args.rounds,
                "result_rows": rows[name], "img_s_median": len(images) / float(np.median(s)),
                "img_s_min": len(images) / float(s.max()),
                "img_s_max": len(images) / float(s.min())}), flush=True)

    # the two kernels on their own, batch 8
    B, (H, W) = 8, shape
    pool, desc = ops.pack_images(images[:B], size=(W, H))
    pool, desc = pool.to(dev), desc.to(dev)
    inside = 0
    for _, ih, iw in desc.cpu().numpy():
        nw, nh = ops._letterbox_sides(int(ih), int(iw), (W, H))
        inside += nw * nh
    t = events(lambda: ops.letterbox_batch(pool, desc, (W, H)), args.reps)
    written, read = B * H * W * 12, int(pool.numel())
    print(json.dumps({
        "what": "letterbox_batch", "input": args.input, "slots": B, "seconds": t,
        "bytes_written": written, "bytes_source": read, "tap_bytes_at_most": inside * 12,
        "bytes_per_s": (written + read) / t, "floor_seconds_at_8TBs": (written + read) / HBM,
        "working_set_bytes": written + read,
        "fits_infinity_cache_256MiB": written + read <= 256 << 20}), flush=True)
    from jabd_amd.predict import _priors_for
    A = _priors_for(net, cfg_mnet, H, W, dev).shape[0]
    g = torch.Generator().manual_seed(3)
    rows = torch.rand((B, A, 15), generator=g).to(dev)
    for label, kept, max_det in (("every row kept", A, 0), ("750 per slot", A, 750),
                                 ("300 rows kept", 300, 750)):
        n_keep = torch.full((B,), kept, dtype=torch.int64, device=dev)
        cap = B * (min(max_det, A) if max_det else A)
        out = torch.empty((cap, 15), dtype=torch.float32, device=dev)
        offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
        t = events(lambda: ops.batch_collect(rows, n_keep, desc, (H, W), max_det=max_det,
                                             out=out, offsets=offsets), args.reps)
        moved = int(offsets[-1].item()) * 120
        print(json.dumps({
            "what": "batch_collect", "case": label, "input": args.input, "slots": B, "A": A,
            "seconds": t, "rows_out": int(offsets[-1].item()), "bytes_read_plus_written": moved,
            "bytes_per_s": moved / t, "floor_seconds_at_8TBs": moved / HBM}), flush=True)


if __name__ == "__main__":
    main()
