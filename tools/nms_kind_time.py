"""Time both suppression rules of the batched NMS on the C5 input (bench.py's
nms leg: 8 images x 100k clustered boxes, seed 99, threshold 0.3).

    python tools/nms_kind_time.py [--warmup 10] [--reps 50] [--thr 0.3]

Per kind: the median and the spread of --reps timed calls after --warmup
untimed ones (HIP events around each call), the kept counts, and the pair
counters of jabd_nms_pair_stats.  One JSON line per kind.  The DIoU time has
no target: it is recorded next to the IoU time so that
the next change to nms.hip has a baseline.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "jabd-joint-attention-based-detector-for-small-face-detection_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--thr", type=float, default=0.3)
    ap.add_argument("--kinds", default="iou,diou")
    args = ap.parse_args()
    if args.reps < 1 or args.warmup < 0:
        ap.error("--reps must be at least 1 and --warmup at least 0")
    from jabd_amd import ops, synth
    dev = torch.device("cuda:0")
    B, n = 8, 100_000
    bx, sc = synth.nms_boxes(B, n, seed=99)
    b, s = torch.from_numpy(bx).to(dev), torch.from_numpy(sc).to(dev)
    for kind in args.kinds.split(","):
        for _ in range(args.warmup):
            ops.batched_nms(b, s, args.thr, kind=kind)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.batched_nms(b, s, args.thr, kind=kind)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        _, nk, tested, dense = ops.batched_nms_stats(b, s, args.thr, kind=kind)
        ms = np.sort(np.asarray(ms))
        print(json.dumps({
            "kind": kind, "config": f"C5: {B} x {n} clustered boxes, seed 99, thr {args.thr}",
            "warmup": args.warmup, "reps": args.reps,
            "ms_median": float(np.median(ms)), "ms_min": float(ms[0]), "ms_max": float(ms[-1]),
            "ms_p10": float(ms[len(ms) // 10]), "ms_p90": float(ms[(9 * len(ms)) // 10]),
            "kept": [int(v) for v in nk.cpu()],
            "pairs_tested": [int(v) for v in tested],
            "dense_fallback_images": int(dense.sum())}), flush=True)


if __name__ == "__main__":
    main()
