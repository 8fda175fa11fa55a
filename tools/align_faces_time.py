"""Time ops.align_faces (jabd_align_faces_u8) with HIP events.

    python tools/align_faces_time.py [--faces 750] [--size 112] [--reps 20]

750 faces of one 3840 x 2160 image, and the same number spread over eight such
images, at three face sizes: the detector's own small faces (11-22 px between
the crop's borders, scaled up, one sample per pixel), ~150 px faces (2 x 2
sub-samples) and ~400 px faces (4 x 4).  Per case: warm-up, then the median of
--reps calls each between two events, and the mean of --reps calls back to
back; uint8 and float output; cap equal to the face count and cap 6000 (what
extract_faces launches at batch 8, max_det 750: the workgroups beyond the count
exit).  Set beside the time: the bytes written plus every face's source
footprint read once, over 8 TB/s.  One JSON line per case."""
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

HBM = 8.0e12   # bytes/s, the floor the byte counts are set beside
IH, IW = 2160, 3840


def make_rows(n, size, lo, hi, rng):
    """n rows whose landmarks are the template scaled by 1 / U(lo, hi) (log
    uniform), turned by up to 20 degrees, jittered, anywhere in the image; and
    the bytes of their source footprints."""
    from jabd_amd import ops
    q = ops.align_template(size).astype(np.float64) - size / 2.0
    rows = np.zeros((n, 15), np.float32)
    src = 0.0
    for r in range(n):
        sc = float(np.exp(rng.uniform(np.log(lo), np.log(hi))))
        th = rng.uniform(-0.35, 0.35)
        rot = np.array([[np.cos(th), np.sin(th)], [-np.sin(th), np.cos(th)]])
        centre = (rng.uniform(100, IW - 100), rng.uniform(100, IH - 100))
        lm = ((q + rng.normal(0, 1.0, q.shape)) @ rot) / sc + centre
        rows[r, 5:] = lm.astype(np.float32).reshape(10)
        src += (size / sc) ** 2 * 3
    return rows, src


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    each = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        each.append(a.elapsed_time(b) * 1e3)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return float(np.median(each)), a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=750)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("align_faces_time: no HIP device (there is no CPU path to time)")
    from jabd_amd import ops
    dev = torch.device("cuda:0")
    K, size = args.faces, args.size
    for n_img in (1, 8):
        pool = torch.randint(0, 256, (n_img * IH * IW * 3,), dtype=torch.uint8, device=dev)
        desc = torch.tensor([[i * IH * IW * 3, IH, IW] for i in range(n_img)],
                            dtype=torch.int64, device=dev)
        per = [K // n_img + (1 if i < K % n_img else 0) for i in range(n_img)]
        offsets = torch.tensor(np.concatenate([[0], np.cumsum(per)]), dtype=torch.int64,
                               device=dev)
        for label, lo, hi in (("11-22 px faces, s=1", 5.0, 10.0), ("~150 px faces, s=2", 0.6, 0.9),
                              ("~400 px faces, s=4", 0.2, 0.33)):
            host, src = make_rows(K, size, lo, hi, np.random.default_rng(0))
            for cap in (K, 6000):
                rows = torch.full((max(cap, K), 15), float("nan"), device=dev)
                rows[:K] = torch.from_numpy(host).to(dev)
                for kind in ("u8", "f32"):
                    if kind == "f32" and cap != K:
                        continue
                    crops, mats = ops.align_faces(pool, desc, rows, offsets, size=size, out=kind)

                    def fn():
                        ops.align_faces(pool, desc, rows, offsets, size=size, out=kind,
                                        crops=crops, matrices=mats)
                    med, b2b = timed(fn, args.reps)
                    nbytes = K * size * size * (3 if kind == "u8" else 12) + K * 24 + src
                    print(json.dumps({"images": n_img, "faces": K, "size": size, "case": label,
                                      "cap": int(rows.shape[0]), "out": kind,
                                      "median_us": round(med, 2),
                                      "back_to_back_us": round(b2b, 2),
                                      "bytes": int(nbytes),
                                      "floor_us": round(nbytes / HBM * 1e6, 2),
                                      "fraction_of_floor": round(nbytes / HBM * 1e6 / med, 4)}),
                          flush=True)
        del pool


if __name__ == "__main__":
    main()
