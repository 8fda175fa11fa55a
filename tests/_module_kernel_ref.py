"""Float64 restatements, float32 same-order restatements and error bounds for
the module-level kernels (csrc/modules.hip, the gate-scale backward of
csrc/train.hip, the nearest up-sample pair of csrc/nlm_train.hip), shared by
tests/test_module_kernel_edges.py.  Test infrastructure only; nothing here runs
on the device.  Tensors are the kernels' layouts: NHWC maps [B, H, W, C],
pooled rows [B, S, C].

Activation derivatives follow the project's table (oracle/model_ref.py,
_KinkFn): relu / leaky z > 0; hardswish z < -3 -> 0, z <= 3 -> z/3 + 1/2,
else 1; hardsigmoid 1/6 on the open interval (-3, 3).  torch's CPU
Hardswish backward is NOT the reference at exactly +-3: it returns 0 at -3
and g at +3 where the table gives -g/2 and 3g/2 (everywhere else the two
agree, which test_act_table_matches_torch_off_the_kinks pins).  A NaN fails
every comparison of the table, so relu' = 0, leaky' = slope, hardswish' = 1
and hardsigmoid' = 0 there.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of float32 (round to nearest)
TINY = 2.0 ** -150      # absolute rounding error of a subnormal float32 result
ACT = {"none": 0, "relu": 1, "leaky": 2, "hswish": 3, "hsigmoid": 4, "sigmoid": 5}
KINDS = ("relu", "leaky", "hswish", "hsigmoid", "sigmoid")
SLOPE = 0.1


# ============================================================ adaptive average pool
def bins(n, z):
    """AdaptiveAvgPool2d's bins of an axis of n into z: [floor(b n / z), ceil((b+1) n / z))."""
    return [((b * n) // z, ((b + 1) * n + z - 1) // z) for b in range(z)]


def pool_fwd(x, sizes):
    """cat over sizes of adaptive_avg_pool2d(x, (z, z)) -> [B, S, C], in x's dtype
    (sum of the bin's pixels, then one division by the count)."""
    out = []
    for z in sizes:
        for r0, r1 in bins(x.shape[1], z):
            for c0, c1 in bins(x.shape[2], z):
                out.append(x[:, r0:r1, c0:c1].sum((1, 2)) / ((r1 - r0) * (c1 - c0)))
    return torch.stack(out, 1)


def pool_counts(H, W, sizes):
    """Pixels per bin, [S]."""
    return torch.tensor([(r1 - r0) * (c1 - c0) for z in sizes for r0, r1 in bins(H, z)
                         for c0, c1 in bins(W, z)], dtype=torch.float64)


def pool_bwd(dy, H, W, sizes):
    """dx[b, i, j, c] = sum over every bin holding (i, j) of dy[b, s, c] / |bin s|:
    each bin scatters to its pixels, so no bin can be missed.  Levels, then bin
    rows, then bin columns ascending, which is also each pixel's order of
    accumulation in the kernel: in float32 this is the same-order restatement."""
    B, _, C = dy.shape
    dx = torch.zeros((B, H, W, C), dtype=dy.dtype)
    s = 0
    for z in sizes:
        for r0, r1 in bins(H, z):
            for c0, c1 in bins(W, z):
                cnt = torch.tensor((r1 - r0) * (c1 - c0), dtype=dy.dtype)
                dx[:, r0:r1, c0:c1] += (dy[:, s] / cnt)[:, None, None, :]
                s += 1
    return dx


def bins_per_pixel(H, W, sizes):
    """How many bins hold each pixel, [H, W]."""
    n = torch.zeros((H, W), dtype=torch.float64)
    for z in sizes:
        for r0, r1 in bins(H, z):
            for c0, c1 in bins(W, z):
                n[r0:r1, c0:c1] += 1
    return n


def pool_bwd_window(dy, H, W, sizes, window):
    """The gather form, per pixel, scanning bin rows / columns lo(i) .. hi(i):
    window "pm1" is floor(i z / n) -/+ 1, the search adaptive_pool_bwd_kernel
    used before it was widened; "exact" is floor(i z / n) .. ceil((i+1) z / n) - 1."""
    def rng(i, n, z):
        if window == "pm1":
            return max(0, i * z // n - 1), min(z - 1, i * z // n + 1)
        return i * z // n, min(z - 1, ((i + 1) * z - 1) // n)

    B, _, C = dy.shape
    dx = torch.zeros((B, H, W, C), dtype=dy.dtype)
    for i in range(H):
        for j in range(W):
            base = 0
            for z in sizes:
                rb, cb = bins(H, z), bins(W, z)
                bi0, bi1 = rng(i, H, z)
                bj0, bj1 = rng(j, W, z)
                for bi in range(bi0, bi1 + 1):
                    r0, r1 = rb[bi]
                    if not r0 <= i < r1:
                        continue
                    for bj in range(bj0, bj1 + 1):
                        c0, c1 = cb[bj]
                        if not c0 <= j < c1:
                            continue
                        dx[:, i, j] += dy[:, base + bi * z + bj] / ((r1 - r0) * (c1 - c0))
                base += z * z
    return dx


def torch_pool(x, sizes):
    """The plain PyTorch op: F.adaptive_avg_pool2d per size, concatenated, and the
    gradient of sum(out * w) by autograd (x NHWC float64; w [B, S, C])."""
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    out = torch.cat([F.adaptive_avg_pool2d(xr, (z, z)).flatten(2) for z in sizes], 2)
    out = out.permute(0, 2, 1)
    return out.detach(), lambda w: torch.autograd.grad(out, xr, w)[0].permute(0, 2, 3, 1)


# ==================================================================== activations
def act_fwd(z, kind, slope=SLOPE):
    """The five activations in z's dtype (float64 for the reference)."""
    if kind == "relu":
        return torch.where(z > 0, z, torch.where(z != z, z, torch.zeros_like(z)))
    if kind == "leaky":
        return torch.where(z > 0, z, z * slope)
    if kind == "hsigmoid":
        return torch.where(z != z, z, (z / 6 + 0.5).clamp(0, 1))
    if kind == "hswish":
        return z * (z / 6 + 0.5).clamp(0, 1)
    if kind == "sigmoid":
        return 1 / (1 + torch.exp(-z))
    raise KeyError(kind)


def act_deriv(z, kind, slope=SLOPE):
    """d act / dz by the convention table of the module docstring, literally."""
    one, zero = torch.ones_like(z), torch.zeros_like(z)
    if kind == "relu":
        return torch.where(z > 0, one, zero)
    if kind == "leaky":
        return torch.where(z > 0, one, zero + slope)
    if kind == "hswish":
        return torch.where(z < -3, zero, torch.where(z <= 3, z / 3 + 0.5, one))
    if kind == "hsigmoid":
        return torch.where((z > -3) & (z < 3), one / 6, zero)
    if kind == "sigmoid":
        s = 1 / (1 + torch.exp(-z))
        return s * (1 - s)
    raise KeyError(kind)


def act_fwd_f32(x, kind, slope=SLOPE):
    """Float32 restatement of the single-rounding forwards (relu, leaky)."""
    assert kind in ("relu", "leaky") and x.dtype == torch.float32
    return act_fwd(x, kind, torch.tensor(slope, dtype=torch.float32))


def act_bwd_f32(x, dy, kind, slope=SLOPE):
    """Float32 restatement of the single-rounding backwards: dy times a float32
    constant (1, 0, the slope, float32(1/6))."""
    assert kind in ("relu", "leaky", "hsigmoid") and x.dtype == dy.dtype == torch.float32
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    if kind == "hsigmoid":
        d = torch.where((x > -3) & (x < 3), one / 6, zero)     # float32(1) / float32(6)
    else:
        d = torch.where(x > 0, one, zero + (slope if kind == "leaky" else 0.0))
    return dy * d


def act_fwd_bound(z, kind, measured=0.0):
    """Per-element bound on |kernel - float64| of the forward at float64 input z
    (exactly representable in float32).  relu / leaky are compared bit for bit
    instead.  hardsigmoid = med3(fma(z, float32(1/6), 1/2), 0, 1): two roundings
    (the constant, the fma), each relative to |z/6| or |z/6 + 1/2|.  hardswish
    multiplies that by z: the two errors scale with |z| and the product adds a
    third, so 3 u max(|z|, |z z/6|, |z (z/6 + 1/2)|, |y|).  sigmoid: 4x the
    measured error of torch's own float32 CPU sigmoid (its expf cannot be
    derived).  Each rounding of a subnormal result errs by up to 2^-150
    instead of relatively, which the TINY terms add."""
    t, a = z / 6, z / 6 + 0.5
    if kind == "hsigmoid":
        return 2 * U * torch.maximum(t.abs(), a.abs()) + 2 * TINY
    if kind == "hswish":
        m = torch.stack([z.abs(), (z * t).abs(), (z * a).abs(), act_fwd(z, kind).abs()]).amax(0)
        return 3 * U * m + 3 * TINY
    if kind == "sigmoid":
        return torch.full_like(z, 4 * measured)
    raise KeyError(kind)


def act_bwd_bound(z, dy, kind, measured=0.0):
    """Backward bounds.  hardswish: dx = dy * (z / 3 + 1/2) is a division, an add
    and a product, 3 u max(|dy z/3|, |dy (z/3 + 1/2)|, |dy|) (0 and 1 outside
    [-3, 3] are exact, and covered).  sigmoid: 4x the measured error of torch's
    float32 CPU dy * s * (1 - s)."""
    if kind == "hswish":
        m = torch.stack([(dy * z / 3).abs(), (dy * (z / 3 + 0.5)).abs(), dy.abs()]).amax(0)
        return 3 * U * m + 3 * TINY
    if kind == "sigmoid":
        return torch.full_like(z, 4 * measured)
    raise KeyError(kind)


ACT_LIPSCHITZ = {"none": 1.0, "relu": 1.0, "leaky": 1.0, "hswish": 1.5, "hsigmoid": 1 / 6,
                 "sigmoid": 0.25}


def sigmoid_measured(x32, dy32=None):
    """Worst |float32 CPU torch - float64| of sigmoid(x) (and of dy * s * (1 - s))
    on these inputs."""
    s32, s64 = torch.sigmoid(x32), torch.sigmoid(x32.double())
    fwd = float((s32.double() - s64).abs().max()) if x32.numel() else 0.0
    if dy32 is None:
        return fwd
    d32, d64 = dy32 * (s32 * (1 - s32)), dy32.double() * (s64 * (1 - s64))
    return fwd, (float((d32.double() - d64).abs().max()) if x32.numel() else 0.0)


def kink_inputs():
    """Finite inputs on and beside every kink: +-3, +-0, their float32
    neighbours, a subnormal of each sign."""
    f = np.float32
    v = [f(-3), f(3), f(0), f(-0.0)]
    for k in (f(-3), f(3), f(0)):
        v += [np.nextafter(k, f(np.inf), dtype=f), np.nextafter(k, f(-np.inf), dtype=f)]
    v += [f(1e-40), f(-1e-40)]
    return torch.from_numpy(np.asarray(v, dtype=f))


# ===================================================================== eval BN + act
def bn_eval(x, rm, rv, eps, g, b):
    """z = (x - mean) / sqrt(var + eps) * gamma + beta over rows [M, C] in float64,
    and M = the largest magnitude among its intermediates (x - mean, that times
    invstd, that times gamma, z).  The kernel's float32 expression rounds at
    most 7 times (var + eps, sqrt, 1 / sqrt, the subtraction, two products, the
    add), every one relative to one of those intermediates: |kernel - z| <=
    7 u M.  Neither |x| nor |mean| enters: the subtraction of two float32
    values errs relative to its result, so a mean far above x's spread does not
    widen the bound (a folded x * scale + shift form would break it)."""
    d = x - rm
    t = d / torch.sqrt(rv + eps)
    tg = t * g
    z = tg + b
    return z, torch.stack([d.abs(), t.abs(), tg.abs(), z.abs()]).amax(0)


# ============================================================ channel scale, backward
def scale_bwd(da, x, s):
    """dx = da * s[b][c]; ds[b][c] = sum_hw da * x, and sum_hw |da * x| (da, x
    [B, HW, C], s [B, C])."""
    return da * s[:, None, :], (da * x).sum(1), (da * x).abs().sum(1)


def eca_fwd(x, w, gate):
    """x * gate(conv1d(mean_hw(x))) on NCHW x, plain torch ops (autograd-able);
    also returns the conv1d output z."""
    k = w.numel()
    z = F.conv1d(x.mean((2, 3)).unsqueeze(1), w.view(1, 1, k), padding=(k - 1) // 2).squeeze(1)
    s = torch.sigmoid(z) if gate == "sigmoid" else F.hardsigmoid(z)
    return x * s[:, :, None, None], z


# ================================================================= nearest up-sample
def nearest_index(n_in, n_out):
    """ATen's nearest source index of every destination index: min(floorf(dst *
    float32(in / out)), in - 1), computed in float32 for every tensor dtype."""
    scale = np.float32(n_in) / np.float32(n_out)
    idx = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return torch.from_numpy(np.minimum(idx, n_in - 1))


def nearest_fwd(src, h, w):
    ii, jj = nearest_index(src.shape[1], h), nearest_index(src.shape[2], w)
    return src[:, ii][:, :, jj]


def nearest_bwd(dup, hs, ws):
    """Scatter-add of dup [B, h, w, C] onto its sources -> [B, hs, ws, C]."""
    B, h, w, C = dup.shape
    ii, jj = nearest_index(hs, h), nearest_index(ws, w)
    rows = torch.zeros((B, hs, w, C), dtype=dup.dtype).index_add_(1, ii, dup)
    return torch.zeros((B, hs, ws, C), dtype=dup.dtype).index_add_(2, jj, rows)


# ======================================================================== max-pool
def torch_maxpool(x, dy=None):
    """F.max_pool2d(3, 2, 1) of NHWC x on the CPU in x's dtype, and autograd's dx."""
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(dy is not None)
    y = F.max_pool2d(xr, 3, 2, 1)
    if dy is None:
        return y.permute(0, 2, 3, 1).contiguous()
    (dx,) = torch.autograd.grad(y, xr, dy.permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1).contiguous(), dx.permute(0, 2, 3, 1).contiguous()


def distinct(shape, seed):
    """Float32 values that are all different (a shuffled grid of step 1/8), so a
    max-pool window has one maximum."""
    n = int(np.prod(shape))
    p = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    return ((p.float() - n // 2) / 8).view(shape)


def randn(shape, seed, scale=1.0, dtype=torch.float32):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed),
                        dtype=torch.float64) * scale).to(dtype)
