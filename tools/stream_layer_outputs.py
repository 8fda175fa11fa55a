"""Outputs of the conv1x1_stream-served layers of one C2 forward (bs32 1024^2
JABD-MNv3 eval), one .npy per layer, for a bytewise comparison of two builds.

  JABD_LIB=<parent libjabd.so> python3 tools/stream_layer_outputs.py --out DIR_A
  python3 tools/stream_layer_outputs.py --out DIR_B
  python3 tools/stream_layer_outputs.py --compare DIR_A DIR_B
"""
import argparse
import filecmp
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jabd-joint-attention-based-detector-for-small-face-detection_amd")]


def dump(out_dir, batch, size):
    import numpy as np
    import torch
    import bench
    from jabd_amd import _lib, functional as F, synth
    dev = torch.device("cuda")
    m = bench.build_model(dev)
    x = synth.images(batch, size, device=dev)
    os.makedirs(out_dir, exist_ok=True)
    real = F.conv
    n = [0]

    def conv(xx, pk, *a, **kw):
        _lib.launch_log_reset()
        y = real(xx, pk, *a, **kw)
        log = _lib.launch_log()
        if log and log[0][0] == "conv1x1_stream":
            M = y.shape[0] * y.shape[1] * y.shape[2]
            name = "%02d_M%d_K%d_N%d_tag%d.npy" % (n[0], M, pk.Cin + pk.Cin2, pk.Cout, log[0][1])
            np.save(os.path.join(out_dir, name), y.cpu().numpy())
            n[0] += 1
        return y

    F.conv = conv
    with torch.no_grad():
        m(x)
    torch.cuda.synchronize()
    print("%d stream-served layers written to %s" % (n[0], out_dir))


def compare(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    if fa != fb:
        print("different layer lists:", fa, fb)
        return 1
    bad = 0
    for f in fa:
        same = filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False)
        h = hashlib.sha256(open(os.path.join(a, f), "rb").read()).hexdigest()[:16]
        print("%-40s %s  sha256 %s" % (f, "bytes equal" if same else "DIFFERENT", h))
        bad += not same
    print("%d layers, %d different" % (len(fa), bad))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    dump(args.out, args.batch, args.size)


if __name__ == "__main__":
    main()
