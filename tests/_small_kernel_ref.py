"""Input recipes, fp64 references and error metrics shared by the edge tests of
the three small kernels: tests/test_beca_edges.py, tests/test_wider_eval_edges.py
and tests/test_bicubic_edges.py.  Test infrastructure only; nothing here runs
on the device."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

# ============================================================================ BECA
# x is the kernels' layout, [B, P, C] (NHWC with the H*W pixels flattened).


def beca_block(x, w):
    """The reference block (train_mobilenetV3_ecagai.py:276-284, :301-308) in
    x's dtype: two-pass population std over the pixels, conv1d over channels
    (zero pad (k-1)/2, no bias), Hardsigmoid, x * gate.  Returns the four
    [B, C] stats rows the kernel keeps (mean, std, v, gate) and y."""
    P = x.shape[1]
    mean = x.sum(1, keepdim=True) / P
    std = ((x - mean).pow(2).sum(1, keepdim=True) / P).pow(0.5)      # [B, 1, C]
    k = w.numel()
    v = F.conv1d(std, w.view(1, 1, k), padding=(k - 1) // 2)
    gate = (v + 3).clamp(0, 6) / 6                                    # Hardsigmoid
    return {"mean": mean[:, 0], "std": std[:, 0], "v": v[:, 0], "gate": gate[:, 0],
            "y": x * gate}


def beca_ref(x, w, gy, dtype=torch.float64):
    """beca_block plus autograd's dx, dw for the cotangent gy, all in `dtype`."""
    xr = x.to(dtype).clone().requires_grad_(True)
    wr = w.to(dtype).clone().requires_grad_(True)
    out = beca_block(xr, wr)
    out["y"].backward(gy.to(dtype))
    out = {n: t.detach() for n, t in out.items()}
    out["dx"], out["dw"] = xr.grad, wr.grad
    return out


def beca_x(B, C, P, seed):
    """Per (b, c): scale exp(U(log 0.05, log 4)), offset U(-3, 3), x = randn * s + m,
    so the stds the conv1d sees span 80x instead of sitting at one value."""
    g = torch.Generator().manual_seed(seed)
    s = torch.exp(torch.empty(B, 1, C).uniform_(math.log(0.05), math.log(4.0), generator=g))
    m = torch.empty(B, 1, C).uniform_(-3.0, 3.0, generator=g)
    return torch.randn(B, P, C, generator=g) * s + m


def beca_taps(x, k, seed):
    """w = a * u: u = randn(k) minus its mean (k > 1) so v takes both signs, a
    such that 3 is the geometric middle of the widest (ratio) gap between
    adjacent sorted |conv1d(std, u)| in the 40%-60% quantile range: about a
    quarter of the gates saturate low, a quarter high, half stay linear, and
    no |v| sits on the Hardsigmoid's kinks."""
    g = torch.Generator().manual_seed(seed + 7919)
    u = torch.randn(k, generator=g, dtype=torch.float64)
    if k > 1:
        u = u - u.mean()
    xd = x.double()
    std = (xd - xd.mean(1, keepdim=True)).pow(2).mean(1, keepdim=True).sqrt()
    s = F.conv1d(std, u.view(1, 1, k), padding=(k - 1) // 2).abs().flatten().sort().values
    n = s.numel()
    lo, hi = int(math.floor(0.4 * n)), min(n - 1, int(math.ceil(0.6 * n)))
    lo = min(lo, hi - 1)
    cand = s[lo:hi + 1]
    j = int((cand[1:] / cand[:-1]).argmax())
    a = 3.0 / math.sqrt(float(cand[j]) * float(cand[j + 1]))
    return (a * u).float()


def beca_regimes(v):
    """(fraction v <= -3, fraction |v| < 3, fraction v >= 3, min ||v| - 3|)."""
    v = v.double().flatten()
    n = v.numel()
    return (int((v <= -3).sum()) / n, int((v.abs() < 3).sum()) / n, int((v >= 3).sum()) / n,
            float((v.abs() - 3).abs().min()))


KINK_MARGIN = 1e-3   # 100x the fp32 error of v; the recipe clears it by another 10x
REGIME_MIN = 0.10    # of the gates, in each regime, once B * C >= 24

# (B, C, pixels, k): the branch each one reaches is in test_beca_edges.py's docstring
BECA_CASES = ((2, 40, 2051, 3), (3, 64, 1155, 3), (2, 256, 100, 5), (1, 100, 63, 5),
              (2, 1024, 64, 5), (2, 1028, 2050, 5), (1, 4, 65613, 5), (3, 70, 129, 3),
              (2, 6, 300, 3), (2, 66, 2049, 9))
BECA_ABI_CASES = ((2, 40, 2051, 3), (2, 1028, 2050, 5))
BECA_LARGE_MEAN = (2, 40, 2400, 3)


def beca_id(case):
    return "B%d-C%d-P%d-k%d" % case


@functools.lru_cache(maxsize=None)
def beca_case(case, kind="recipe"):
    """(x, w, gy, fp64 reference) of one case, computed once and shared; treat
    every tensor as read-only.  kind "large_mean": x = 64 + 0.05 * randn, which
    separates the two-pass std from a one-pass E[x^2] - E[x]^2 (64^2 * 2^-24 =
    2.4e-4 against a variance of 2.5e-3)."""
    B, C, P, k = case
    seed = C * 31 + P
    if kind == "large_mean":
        x = 64.0 + 0.05 * torch.randn(B, P, C, generator=torch.Generator().manual_seed(seed))
    else:
        x = beca_x(B, C, P, seed)
    w = beca_taps(x, k, seed)
    gy = torch.randn(B, P, C, generator=torch.Generator().manual_seed(seed + 1))
    return x, w, gy, beca_ref(x, w, gy)


def _slice_max(t):
    """max |t| over the pixels of each (b, c) slice of a [B, P, C] tensor."""
    return t.double().abs().amax(1, keepdim=True)


def beca_errors(got, ref, x, gy):
    """Per-(b, c)-slice errors, the worst slice reported.  Slice scales span 80x
    and a near-closed gate makes max |y| tiny, so y is normalised by the slice's
    max(|ref|, |x|) and dx by its max(|ref|, |grad_y|); dw by max |ref|."""
    y_den = torch.maximum(_slice_max(ref["y"]), _slice_max(x))
    dx_den = torch.maximum(_slice_max(ref["dx"]), _slice_max(gy))
    return {
        "y": float(((got["y"].double().cpu() - ref["y"]).abs() / y_den).max()),
        "dx": float(((got["dx"].double().cpu() - ref["dx"]).abs() / dx_den).max()),
        "dw": float((got["dw"].double().cpu() - ref["dw"]).abs().max() / ref["dw"].abs().max()),
    }


def beca_stats_errors(stats, ref, w):
    """The four kept rows on their own: mean relative to the slice's RMS
    sqrt(mean^2 + std^2) (a mean may sit at 0), std relative to itself, v
    relative to conv1d(std, |w|) (the size of the terms it sums), the gate
    absolutely."""
    B, C = ref["mean"].shape
    s = stats.double().cpu().view(4, B, C)
    k = w.numel()
    vden = F.conv1d(ref["std"][:, None], w.double().abs().view(1, 1, k), padding=(k - 1) // 2)[:, 0]
    return {
        "mean": float(((s[0] - ref["mean"]).abs()
                       / (ref["mean"] ** 2 + ref["std"] ** 2).sqrt()).max()),
        "std": float(((s[1] - ref["std"]).abs() / ref["std"]).max()),
        "v": float(((s[2] - ref["v"]).abs() / vden).max()),
        "gate": float((s[3] - ref["gate"]).abs().max()),
    }


# ====================================================================== WIDER eval
def _a(rows, k):
    return np.asarray(rows, np.float64).reshape(-1, k)


def _score_at(t, T):
    """Threshold t of T exactly as the evaluation computes it."""
    return 1 - (t + 1) / T


# name -> (preds, gts, ignores, iou_thresh, thresh_num, expected [T, 2] rows of
# [proposals, recalled]).  Derivations, from utils/evaluation.py:255-305, are in
# tests/test_wider_eval_edges.py::test_oracle_hand_case.
_UNIT = [0, 0, 10, 10]
WIDER_HAND = {
    "argmax-tie-first-ignored": ([_a([_UNIT + [0.9]], 5)], [_a([_UNIT, _UNIT], 4)], [[0, 1]],
                                 0.5, 4, [[0, 0]] * 4),
    "argmax-tie-first-kept": ([_a([_UNIT + [0.9]], 5)], [_a([_UNIT, _UNIT], 4)], [[1, 0]],
                              0.5, 4, [[1, 1]] * 4),
    "iou-equals-thresh": ([_a([[0, 0, 10, 5, 0.9]], 5)], [_a([_UNIT], 4)], [[1]],
                          0.5, 4, [[1, 1]] * 4),
    "iou-one-ulp-under-thresh": ([_a([[0, 0, 10, 5, 0.9]], 5)], [_a([_UNIT], 4)], [[1]],
                                 float(np.nextafter(0.5, 1)), 4, [[1, 0]] * 4),
    "score-equals-threshold": ([_a([[50, 50, 5, 5, _score_at(2, 7)]], 5)], [_a([_UNIT], 4)], [[1]],
                               0.5, 7, [[0, 0], [0, 0]] + [[1, 0]] * 5),
    "score-one-ulp-under-threshold": ([_a([[50, 50, 5, 5, float(np.nextafter(_score_at(2, 7), 0))]],
                                          5)], [_a([_UNIT], 4)], [[1]],
                                      0.5, 7, [[0, 0]] * 3 + [[1, 0]] * 4),
    "nan-coordinate": ([_a([[float("nan"), 0, 10, 10, 0.9], _UNIT + [0.8]], 5)], [_a([_UNIT], 4)],
                       [[1]], 0.5, 4, [[2, 1]] * 4),
    "zero-over-zero": ([_a([[5, 5, 0, 0, 0.9], [20, 20, 10, 10, 0.8]], 5)],
                       [_a([[5, 5, 0, 0], [20, 20, 10, 10]], 4)], [[1, 1]], 0.5, 4, [[2, 1]] * 4),
    "unsorted-scores": ([_a([_UNIT + [0.2], [50, 50, 5, 5, 0.9], _UNIT + [0.6]], 5)],
                        [_a([_UNIT], 4)], [[1]], 0.5, 5, [[2, 1]] + [[3, 1]] * 4),
}


def wider_image(n_pred, n_gt, g, ignore=None, sort=False):
    """One synthetic image: gts scattered over a 200 x 200 field, three quarters
    of the preds jittered copies of a gt (so IoUs land on both sides of the
    threshold), a quarter moved anywhere; scores unsorted unless asked."""
    gt = np.c_[g.uniform(0, 200, (n_gt, 2)), g.uniform(4, 40, (n_gt, 2))]
    src = gt[g.integers(0, n_gt, n_pred)] if n_gt else np.zeros((n_pred, 4))
    pr = src + g.normal(0, 3, (n_pred, 4))
    pr[: n_pred // 4, :2] = g.uniform(0, 200, (n_pred // 4, 2))
    scores = g.uniform(0, 1, n_pred)
    if sort:
        scores = np.sort(scores)[::-1]
    if ignore is None:
        ig = (g.uniform(0, 1, n_gt) < 0.7).astype(np.uint8)
    else:
        ig = np.full(n_gt, ignore, np.uint8)
    return np.c_[pr, scores], gt, ig


def wider_set(sizes, seed, ignore=None):
    """(preds, gts, ignores) for a list of (n_pred, n_gt) image sizes."""
    g = np.random.default_rng(seed)
    imgs = [wider_image(n, m, g, ignore) for n, m in sizes]
    return [i[0] for i in imgs], [i[1] for i in imgs], [i[2] for i in imgs]


# (n_pred, n_gt) per image.  The kernel's workgroup is 256 wide: 700 / 300 and
# 257 take a second (and third) trip of its `+= blockDim.x` loops.
WIDER_SETS = {
    "700x300-unsorted": [(700, 300)],
    "257x1-and-1x257": [(257, 1), (1, 257)],
    "empties-first-middle-last": [(0, 5), (9, 4), (7, 0), (0, 0), (12, 6), (5, 0), (0, 3)],
    "all-empty": [(0, 4), (6, 0), (0, 0)],
    "300-tiny-images": [(1 + i % 3, 1 + i % 2) for i in range(300)],
}

# ========================================================================= bicubic


def bicubic_ref(x_nchw, size, wts):
    """F.interpolate(mode="bicubic", align_corners=True) in float64 on the CPU,
    and the gradient of sum(out * wts)."""
    xr = x_nchw.double().clone().requires_grad_(True)
    out = F.interpolate(xr, size=list(size), mode="bicubic", align_corners=True)
    out.backward(wts.double())
    return out.detach(), xr.grad
