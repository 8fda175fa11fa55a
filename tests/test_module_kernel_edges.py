"""Edge parity of the kernels behind the stand-alone nn.Module surface, each
called through its C entry point (jabd_amd._lib.call) so that strides,
alignment, nblk and the workspace are the test's to choose.  References and
bounds: tests/_module_kernel_ref.py.

  adaptive pool   backward at maps smaller than the output size (z > 2H puts
                  more than three bins on a row: the old floor(i z / H) -/+ 1
                  search dropped the rest), forward two-pass, one-pass (no
                  workspace: unreachable from Python) and with a workspace one
                  float short; C past the 256 threads; a batch stride wider
                  than the image; bad size lists
  activations     five kinds, n = 0 .. 1027, every pointer misaligned in turn,
                  guards, the float4 grid-stride loop past its 8192-workgroup
                  cap, the kinks and their float32 neighbours, NaN and +-inf
  eval BN + act   C = 1 .. 257, M = 0 .. 7, the grid-stride wrap, var 0 and
                  1e4, a mean far above x's spread
  channel scale   bit for bit, the image index after the stride wraps
  scale backward  empty and short pixel blocks (ScaleFn passes nblk =
                  clamp(HW // 256, 1, 64), so Python cannot make an empty one
                  today), ECA backward through EcaScaleFn with both gates
  nearest         forward, + add (non-zero lateral), backward with and without
                  accumulation, ratios 1, 2, above 2 and a 1 x 1 source
  max-pool 3/2/1  maps of 1 x 1 .. 2 x 9, C4 not a power of two and above 64

Bars.  A single-rounding op equals its float32 restatement bit for bit (a
signed zero aside: -0 == +0).  A short float32 expression: (roundings) x 2^-24
x (largest float64 intermediate of the element).  A sequential sum of n terms:
(n + 1) 2^-24 sum|terms|.  Sigmoid: 4x the error of torch's own float32 CPU
sigmoid against float64, taken over all the inputs of a test together; on the
2 000 N(0, 4^2) inputs of test_act_sizes_and_alignment that is 8.4e-8 forward
and 1.6e-7 for dy * s * (1 - s) (|dy| up to 3.5), so the bars there are 3.3e-7
and 6.2e-7; on the 12 kink inputs 1.8e-8 and 2.7e-8.

Not marked gpu: the helpers against torch.nn.functional in float64, and a
known-answer test of the old bin window, which differs from the reference at
(H, W, z) = (2, 2, 6) and agrees at (3, 3, 6), (4, 4, 8), (13, 17, 8).
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import _module_kernel_ref as R
from _module_kernel_ref import ACT, KINDS, SLOPE, U

gpu = pytest.mark.gpu

PSP = (1, 3, 6, 8)
EIGHT = (1, 2, 3, 4, 5, 6, 7, 8)
POOL_MAPS = ((2, 2), (1, 5), (5, 1), (2, 7), (3, 2), (1, 1), (4, 4), (13, 17))
POOL_CASES = [(hw, sz) for hw in POOL_MAPS for sz in (PSP, (6,), EIGHT)] + [((3, 5), (16,))]


def _pid(case):
    (H, W), sz = case
    return f"{H}x{W}-" + "_".join(map(str, sz))


def _same(a, b):
    """Equal element for element, NaN matching NaN (a signed zero aside)."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _within(got, ref, bound):
    """max (|got - ref| - bound) <= 0 elementwise; returns the worst err / bound
    for the message."""
    err = (got.double() - ref).abs()
    if err.numel() == 0:
        return True, 0.0
    return bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())


# ============================================================== CPU: the helpers
@pytest.mark.parametrize("hw", [(2, 2), (1, 5), (2, 7), (3, 2), (13, 17), (7, 1)])
def test_pool_helpers_match_torch(hw):
    """pool_fwd, pool_bwd (scatter) and the exact-range gather against
    F.adaptive_avg_pool2d and its autograd in float64, sizes (1, 3, 6, 8)
    concatenated; bar 64 x 2^-53 x the largest magnitude (float64 rounding of
    sums of at most 221 terms in another order)."""
    H, W = hw
    x = R.randn((2, H, W, 5), 3, dtype=torch.float64)
    w = R.randn((2, sum(z * z for z in PSP), 5), 4, dtype=torch.float64)
    out, grad = R.torch_pool(x, PSP)
    eps = 64 * 2.0 ** -53
    assert (R.pool_fwd(x, PSP) - out).abs().max() <= eps * x.abs().max()
    want = grad(w)
    for got in (R.pool_bwd(w, H, W, PSP), R.pool_bwd_window(w, H, W, PSP, "exact")):
        assert (got - want).abs().max() <= eps * want.abs().max()
    assert float(R.pool_counts(H, W, PSP).sum()) == float(R.bins_per_pixel(H, W, PSP).sum())


def test_old_bin_window_drops_bins():
    """Known answer for what the widened search closes: the floor(i z / H) -/+ 1
    window against the full scan.  At (2, 2, 6) row 0 lies in bins 0..2 and row
    1 in bins 3..5, but the window of row 1 is 2..4 (bin 5 lost) and likewise
    for the columns, so dx differs by whole dy terms; at (3, 3, 6), (4, 4, 8)
    and (13, 17, 8) the window holds every bin and the two are identical."""
    for H, W, z, differs in ((2, 2, 6, True), (1, 5, 3, True), (2, 7, 6, True), (2, 3, 8, True),
                             (3, 2, 8, True), (3, 3, 6, False), (4, 4, 8, False),
                             (13, 17, 8, False)):
        dy = R.randn((1, z * z, 2), 5, dtype=torch.float64)
        full = R.pool_bwd(dy, H, W, (z,))
        old = R.pool_bwd_window(dy, H, W, (z,), "pm1")
        err = float((old - full).abs().max())
        if differs:
            assert err > 0.5, (H, W, z, err)
        else:
            assert torch.equal(old, R.pool_bwd_window(dy, H, W, (z,), "exact")), (H, W, z)
            assert err <= 64 * 2.0 ** -53 * float(full.abs().max()), (H, W, z, err)
    # the lost mass at (2, 2, 6) is exactly the bins outside the window
    ones = torch.ones((1, 36, 1), dtype=torch.float64)
    assert float(R.pool_bwd(ones, 2, 2, (6,)).sum()) == pytest.approx(36.0)
    assert float(R.pool_bwd_window(ones, 2, 2, (6,), "pm1").sum()) < 36.0 - 1.0


@pytest.mark.parametrize("hw", [(13, 17), (27, 27)])
def test_old_and_new_window_same_order_where_old_was_complete(hw):
    """At the existing 13 x 17 test map and the 27 x 27 pyramid map, sizes
    (1, 3, 6, 8): the float32 gather in the kernel's order gives the same bits
    with the old window, the exact range and the scatter restatement."""
    H, W = hw
    dy = R.randn((1, 110, 3), 6)
    want = R.pool_bwd(dy, H, W, PSP)
    assert torch.equal(R.pool_bwd_window(dy, H, W, PSP, "pm1"), want)
    assert torch.equal(R.pool_bwd_window(dy, H, W, PSP, "exact"), want)


NEAREST = (((1, 1), (7, 5)), ((3, 3), (3, 3)), ((4, 6), (8, 12)), ((5, 7), (17, 13)),
           ((1, 9), (1, 9)))


@pytest.mark.parametrize("src,dst", NEAREST)
def test_nearest_helper_matches_interpolate(src, dst):
    (hs, ws), (h, w) = src, dst
    x = R.randn((2, hs, ws, 3), 7, dtype=torch.float64).requires_grad_(True)
    ref = F.interpolate(x.permute(0, 3, 1, 2), size=(h, w), mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(R.nearest_fwd(x.detach(), h, w), ref.detach())
    g = R.randn((2, h, w, 3), 8, dtype=torch.float64)
    (dx,) = torch.autograd.grad(ref, x, g)
    got = R.nearest_bwd(g, hs, ws)
    assert (got - dx).abs().max() <= 64 * 2.0 ** -53 * dx.abs().max()


def test_act_table_matches_torch_off_the_kinks():
    """The float64 forwards equal torch's; the derivative table equals torch's
    CPU autograd away from +-3 and 0, and states -g/2 and 3g/2 for hardswish at
    -3 and +3."""
    z = R.randn((4001,), 9, 4.0, torch.float64)
    z = z[((z.abs() - 3).abs() > 1e-9) & (z != 0)]
    fns = {"relu": F.relu, "leaky": lambda t: F.leaky_relu(t, SLOPE), "hswish": F.hardswish,
           "hsigmoid": F.hardsigmoid, "sigmoid": torch.sigmoid}
    for kind, fn in fns.items():
        zr = z.clone().requires_grad_(True)
        y = fn(zr)
        (d,) = torch.autograd.grad(y.sum(), zr)
        assert (R.act_fwd(z, kind) - y.detach()).abs().max() <= 8 * 2.0 ** -53 * 16, kind
        # (torch's Hardsigmoid backward multiplies by float32(1/6) in every dtype)
        tol = U / 6 if kind == "hsigmoid" else 8 * 2.0 ** -53
        assert (R.act_deriv(z, kind) - d).abs().max() <= tol, kind
    k = torch.tensor([-3.0, 3.0], dtype=torch.float64)
    assert R.act_deriv(k, "hswish").tolist() == [-0.5, 1.5]
    assert R.act_deriv(k, "hsigmoid").tolist() == [0.0, 0.0]
    nan = torch.tensor([float("nan")], dtype=torch.float64)
    assert [float(R.act_deriv(nan, kd)) for kd in KINDS[:4]] == [0.0, SLOPE, 1.0, 0.0]


def test_float32_restatements_sit_within_the_bounds():
    """The bars hold for honest float32 arithmetic: the same-order float32 pool
    backward and the float32 activations against float64."""
    dy = R.randn((2, 110, 4), 10)
    n = R.bins_per_pixel(2, 7, PSP)[None, :, :, None]
    bound = (n + 1) * U * R.pool_bwd(dy.double().abs(), 2, 7, PSP)
    assert _within(R.pool_bwd(dy, 2, 7, PSP), R.pool_bwd(dy.double(), 2, 7, PSP), bound)[0]
    x = R.randn((4099,), 11, 4.0)
    for kind in ("hswish", "hsigmoid"):
        got = getattr(F, {"hswish": "hardswish", "hsigmoid": "hardsigmoid"}[kind])(x)
        assert _within(got, R.act_fwd(x.double(), kind), R.act_fwd_bound(x.double(), kind))[0]


# ================================================================== GPU plumbing
def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _args(args):
    """Device tensors and Guarded buffers become their addresses here, so that
    every operand stays referenced until the launch has been queued."""
    return [a.data_ptr() if isinstance(a, torch.Tensor) else a.ptr() if isinstance(a, Guarded)
            else a for a in args]


def _call(name, *args):
    from jabd_amd._lib import call
    call(name, *_args(args), _st())


def _i32(v):
    return (ctypes.c_int32 * max(len(v), 1))(*v)


def _refused(name, *args):
    """The entry point must return its error code and launch nothing."""
    from jabd_amd import _lib
    _lib.launch_log_reset()
    with pytest.raises(RuntimeError, match=name):
        _lib.call(name, *_args(args), _st())
    assert _lib.launch_log() == []


SENTINEL = -777.25
GUARD = 8  # floats on each side; a multiple of 4 keeps the 16-byte phase


class Guarded:
    """A float32 device buffer of n elements starting `off` floats past a
    16-byte boundary, NaN-filled, with sentinel guards on both sides."""

    def __init__(self, cuda, n, off=0):
        self.buf = torch.full((n + 2 * GUARD + off,), SENTINEL, device=cuda)
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.n = GUARD + off, n
        self.view = self.buf[self.lo:self.lo + n]
        self.view.fill_(float("nan"))
        assert n == 0 or self.view.data_ptr() % 16 == 4 * (off % 4)

    def ptr(self):
        return self.view.data_ptr()

    def result(self):
        b = self.buf.cpu()
        assert bool((b[:self.lo] == SENTINEL).all()) and \
            bool((b[self.lo + self.n:] == SENTINEL).all()), "wrote outside its range"
        return b[self.lo:self.lo + self.n].clone()


def _at(cuda, t, off=0):
    """t copied to the device `off` floats past a 16-byte boundary."""
    flat = t.reshape(-1)
    buf = torch.zeros(flat.numel() + 4 + off, device=cuda)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + flat.numel()]
    v.copy_(flat)
    return v


# ========================================================== 1. adaptive pool backward
def _pool_bwd_gpu(cuda, dy, H, W, sizes):
    B, _, C = dy.shape
    out = Guarded(cuda, B * H * W * C)
    _call("jabd_adaptive_pool_bwd_f32", _at(cuda, dy), B, H, W, C, _i32(sizes),
          len(sizes), out)
    return out.result().view(B, H, W, C)


@gpu
@pytest.mark.parametrize("case", POOL_CASES, ids=_pid)
def test_adaptive_pool_bwd(cuda, case):
    """jabd_adaptive_pool_bwd_f32 against the float64 full scan, B = 2, C = 4
    and 10.  Each pixel sums n terms dy / |bin| (one division each, n - 1
    adds): bar (n + 1) 2^-24 sum|terms|, n the number of bins holding the
    pixel.  Run against a build of the kernel with the old floor(i z / H) -/+ 1
    search, every case at (2, 2), (1, 5), (5, 1), (2, 7), (3, 2) and (1, 1),
    (4, 4) with the eight sizes and (3, 5) at z = 16 failed (20 of the 25), as
    did test_adaptive_avgpool_module_on_2x2; (13, 17) and (4, 4) with
    (1, 3, 6, 8) or (6,) passed."""
    (H, W), sizes = case
    S = sum(z * z for z in sizes)
    n = R.bins_per_pixel(H, W, sizes)[None, :, :, None]
    for C in (4, 10):
        dy = R.randn((2, S, C), 20 + C)
        got = _pool_bwd_gpu(cuda, dy, H, W, sizes)
        assert bool(got.isfinite().all())
        ref = R.pool_bwd(dy.double(), H, W, sizes)
        ok, worst = _within(got, ref, (n + 1) * U * R.pool_bwd(dy.double().abs(), H, W, sizes))
        assert ok, (C, worst, float((got.double() - ref).abs().max()))


@gpu
@pytest.mark.parametrize("hw", [(13, 17), (27, 27)])
def test_adaptive_pool_bwd_order_unchanged(cuda, hw):
    """Where the old window already held every bin (the 13 x 17 test map, the
    27 x 27 pyramid map, sizes (1, 3, 6, 8)) the widened search adds the same
    terms in the same order: bit-identical to the float32 restatement in that
    order (levels, bin rows, bin columns ascending), which
    test_old_and_new_window_same_order_where_old_was_complete ties to the old
    window on the CPU."""
    H, W = hw
    dy = R.randn((2, 110, 12), 31)
    assert torch.equal(_pool_bwd_gpu(cuda, dy, H, W, PSP), R.pool_bwd(dy, H, W, PSP))


@gpu
def test_adaptive_avgpool_module_on_2x2(cuda):
    """modules.AdaptiveAvgPool2d(6) on a 2 x 2 map (a 64-pixel image at stride
    32), end to end: the input gradient against float64 autograd.  Every pixel
    lies in 9 bins of one pixel each: bar (9 + 1) 2^-24 sum|dy terms|; the
    forward copies pixels (sum of one term / 1): exact."""
    from jabd_amd.modules import AdaptiveAvgPool2d
    x = R.randn((2, 4, 2, 2), 32)
    w = R.randn((2, 4, 6, 6), 33)
    xr = x.double().requires_grad_(True)
    yr = F.adaptive_avg_pool2d(xr, 6)
    (gr,) = torch.autograd.grad(yr, xr, w.double())
    xg = x.to(cuda).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = AdaptiveAvgPool2d(6).to(cuda).train()(xg)
    assert torch.equal(y.detach().cpu(), yr.detach().float())
    (g,) = torch.autograd.grad(y, xg, w.to(cuda))
    xa = x.double().abs().requires_grad_(True)
    (ga,) = torch.autograd.grad(F.adaptive_avg_pool2d(xa, 6), xa, w.double().abs())
    ok, worst = _within(g.cpu(), gr, 10 * U * ga)
    assert ok, worst


# =========================================================== 2. adaptive pool forward
def _pool_fwd_gpu(cuda, x, sizes, ws_mode, x_bs=None):
    from jabd_amd._lib import lib
    B, H, W, C = x.shape
    S = sum(z * z for z in sizes)
    if x_bs is None:
        xd, x_bs = _at(cuda, x), H * W * C
    else:  # a batch slice of a wider buffer, NaN between the images
        wide = torch.full((B, x_bs), float("nan"))
        wide[:, :H * W * C] = x.reshape(B, -1)
        xd = _at(cuda, wide)
    need = int(lib().jabd_adaptive_pool_ws_floats(B, H, C, _i32(sizes), len(sizes)))
    assert need == B * H * sum(sizes) * C
    out = Guarded(cuda, B * S * C)
    if ws_mode == "none":
        ws, ws_ptr, ws_n = None, None, 0
    else:
        ws = Guarded(cuda, need)
        ws_ptr, ws_n = ws, need - (1 if ws_mode == "short" else 0)
    _call("jabd_adaptive_pool_f32", xd, x_bs, B, H, W, C, _i32(sizes), len(sizes),
          out, ws_ptr, ws_n)
    if ws is not None:
        used = ws.result()
        # the short workspace must not be touched: the one-pass form ran
        assert bool(used.isnan().all()) == (ws_mode == "short")
    return out.result().view(B, S, C)


def _pool_fwd_check(got, x, sizes):
    """A bin of n pixels is n - 1 adds and a division in any order: bar
    (n + 1) 2^-24 sum|x| / n."""
    _, H, W, _ = x.shape
    n = R.pool_counts(H, W, sizes)[None, :, None]
    ref = R.pool_fwd(x.double(), sizes)
    assert bool(got.isfinite().all())
    ok, worst = _within(got, ref, (n + 1) * U * R.pool_fwd(x.double().abs(), sizes))
    assert ok, worst


@gpu
@pytest.mark.parametrize("case", POOL_CASES, ids=_pid)
def test_adaptive_pool_fwd(cuda, case):
    """jabd_adaptive_pool_f32 in its two-pass form (workspace), its one-pass
    form (ws NULL, 0 floats) and with a workspace one float short of
    jabd_adaptive_pool_ws_floats (falls back to one pass, leaves the workspace
    alone), C = 1, 10 and 260 (the thread-stride loop over channels), each
    against float64."""
    (H, W), sizes = case
    for C in (1, 10, 260):
        x = R.randn((2, H, W, C), 40 + C)
        for mode in ("full", "none", "short"):
            _pool_fwd_check(_pool_fwd_gpu(cuda, x, sizes, mode), x, sizes)


@gpu
@pytest.mark.parametrize("mode", ["full", "none"])
def test_adaptive_pool_fwd_batch_stride(cuda, mode):
    """x_bs above H W C: each image is the head of a wider row (NaN behind it)."""
    x = R.randn((3, 2, 7, 10), 44)
    _pool_fwd_check(_pool_fwd_gpu(cuda, x, PSP, mode, x_bs=2 * 7 * 10 + 36), x, PSP)


@gpu
def test_adaptive_pool_refuses_bad_sizes(cuda):
    x, out = torch.zeros(2 * 4 * 4 * 4, device=cuda), torch.zeros(2 * 600 * 4, device=cuda)
    for sizes, n in (((), 0), ((1,) * 9, 9), ((1, 0, 3), 3)):
        _refused("jabd_adaptive_pool_f32", x, 64, 2, 4, 4, 4, _i32(sizes), n,
                 out, None, 0)
        _refused("jabd_adaptive_pool_bwd_f32", out, 2, 4, 4, 4, _i32(sizes), n,
                 x)


# ================================================================== 3. activations
_TORCH_FWD = {"relu": F.relu, "leaky": lambda t: F.leaky_relu(t, SLOPE), "hswish": F.hardswish,
              "hsigmoid": F.hardsigmoid, "sigmoid": torch.sigmoid}


def _act_fwd_gpu(cuda, x, kind, xo=0, yo=0):
    out = Guarded(cuda, x.numel(), yo)
    _call("jabd_act_f32", _at(cuda, x, xo), x.numel(), ACT[kind], SLOPE, out)
    return out.result()


def _act_bwd_gpu(cuda, x, dy, kind, xo=0, go=0, do=0):
    out = Guarded(cuda, x.numel(), do)
    _call("jabd_act_bwd_f32", _at(cuda, x, xo), _at(cuda, dy, go),
          x.numel(), ACT[kind], SLOPE, out)
    return out.result()


def _measured(kind, xs, dys):
    """torch's float32 CPU sigmoid error (forward, dy * s * (1 - s)) over all the
    inputs of one test together: a single short vector can by luck round
    correctly everywhere (3.4e-9 at the n = 4 case here) and is no measure."""
    if kind != "sigmoid":
        return 0.0, 0.0
    return R.sigmoid_measured(torch.cat(xs), torch.cat(dys))


def _check_act_fwd(got, x, kind, meas):
    """relu, leaky: one rounding at most, bit for bit against the float32
    restatement.  Others: _module_kernel_ref.act_fwd_bound."""
    if kind in ("relu", "leaky"):
        assert _same(got, R.act_fwd_f32(x, kind)), kind
        return
    xd = x.double()
    ok, worst = _within(got, R.act_fwd(xd, kind), R.act_fwd_bound(xd, kind, meas[0]))
    assert ok, (kind, worst)


def _check_act_bwd(got, x, dy, kind, meas):
    """relu, leaky, hardsigmoid: dy times a float32 constant, bit for bit.
    hardswish, sigmoid: _module_kernel_ref.act_bwd_bound against dy * table."""
    if kind in ("relu", "leaky", "hsigmoid"):
        assert _same(got, R.act_bwd_f32(x, dy, kind)), kind
        return
    xd, gd = x.double(), dy.double()
    ok, worst = _within(got, gd * R.act_deriv(xd, kind), R.act_bwd_bound(xd, gd, kind, meas[1]))
    assert ok, (kind, worst)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_act_sizes_and_alignment(cuda, kind):
    """n = 0, 1, 3, 4, 5, 1023, 1027 with every pointer 16-byte aligned, with
    x one float past a boundary, with only y (only dx) there, and each of the
    three backward pointers there in turn (any one sends the whole call down
    the scalar path); guards on both sides of every output."""
    cases = [(R.randn((n,), 50 + n, 4.0), R.randn((n,), 60 + n))
             for n in (0, 1, 3, 4, 5, 1023, 1027)]
    meas = _measured(kind, *zip(*cases))
    for x, dy in cases:
        for xo, yo in ((0, 0), (1, 0), (0, 1), (1, 1)):
            _check_act_fwd(_act_fwd_gpu(cuda, x, kind, xo, yo), x, kind, meas)
        for xo, go, do in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            _check_act_bwd(_act_bwd_gpu(cuda, x, dy, kind, xo, go, do), x, dy, kind, meas)


N_WRAP = 4 * 8192 * 256 + 4 * 300 + 3


@functools.lru_cache(maxsize=None)
def _wrap_inputs():
    return R.randn((N_WRAP,), 70, 4.0), R.randn((N_WRAP,), 71)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_act_past_the_grid_cap(cuda, kind):
    """n = 4 * 8192 * 256 + 4 * 300 + 3: the float4 kernels' 8192 workgroups
    take a second trip of the grid-stride loop for 300 float4, and 3 elements
    are left to the scalar kernel.  Aligned."""
    x, dy = _wrap_inputs()
    meas = _measured(kind, [x], [dy])
    _check_act_fwd(_act_fwd_gpu(cuda, x, kind), x, kind, meas)
    _check_act_bwd(_act_bwd_gpu(cuda, x, dy, kind), x, dy, kind, meas)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_act_at_the_kinks(cuda, kind):
    """Exactly -3, 3, 0, -0.0, the float32 values next to +-3 and 0, and a
    subnormal of each sign, against the convention table (not torch's CPU
    backward, which differs at +-3).  Once through the float4 kernel (aligned)
    and once through the scalar one."""
    x = R.kink_inputs()
    dy = torch.linspace(0.75, 2.5, x.numel())
    meas = _measured(kind, [x], [dy])
    for off in (0, 1):
        _check_act_fwd(_act_fwd_gpu(cuda, x, kind, off, 0), x, kind, meas)
        _check_act_bwd(_act_bwd_gpu(cuda, x, dy, kind, off, 0, 0), x, dy, kind, meas)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_act_nonfinite(cuda, kind):
    """NaN and +-inf (a 0 between them; the first four go through the float4
    kernel, the last three through the scalar tail).  Forward: equal to torch's
    float32 CPU forward, NaN positions included (relu(NaN) = NaN,
    hardsigmoid(NaN) = NaN, hardswish(-inf) = NaN, hardsigmoid(+-inf) = 1 / 0;
    the bare fmed3 of common.h's hsigmoid_f returned 0 for a NaN on the device,
    which is why modules.hip's mact passes a NaN through).
    Backward: the table taken literally in float32, a NaN failing every
    comparison (sigmoid' (NaN) = NaN)."""
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([nan, inf, -inf, 0.0, nan, inf, -inf])
    dy = torch.tensor([1.5, -2.0, 0.5, 4.0, -1.0, 3.0, 2.0])
    assert _same(_act_fwd_gpu(cuda, x, kind), _TORCH_FWD[kind](x)), kind
    want = dy * R.act_deriv(x, kind, torch.tensor(SLOPE))
    assert _same(_act_bwd_gpu(cuda, x, dy, kind), want), kind


@gpu
def test_act_refuses_unknown_kind(cuda):
    x, y = torch.zeros(8, device=cuda), torch.full((8,), SENTINEL, device=cuda)
    for act in (-1, 6):
        _refused("jabd_act_f32", x, 8, act, SLOPE, y)
        _refused("jabd_act_bwd_f32", x, x, 8, act, SLOPE, y)
        _refused("jabd_bn_eval_f32", x, 2, 4, x, x, 1e-5,
                 x, x, act, SLOPE, y)
    assert bool((y == SENTINEL).all())


# =============================================================== 4. eval BN + act
def _bn_gpu(cuda, x, rm, rv, eps, g, b, kind):
    M, C = x.shape
    out = Guarded(cuda, M * C)
    _call("jabd_bn_eval_f32", _at(cuda, x), M, C, _at(cuda, rm),
          _at(cuda, rv), eps, _at(cuda, g), _at(cuda, b),
          ACT[kind], SLOPE, out)
    return out.result().view(M, C)


def _bn_z(x, rm, rv, eps, g, b):
    e = torch.tensor(eps, dtype=torch.float32).double()
    return R.bn_eval(x.double(), rm.double(), rv.double(), e, g.double(), b.double())


def _bn_check(got, x, rm, rv, eps, g, b, kind, meas=0.0):
    """|kernel - float64| <= L 7 u M + act bar, with 7 u M the bar of the
    normalisation (_module_kernel_ref.bn_eval), L the activation's Lipschitz
    constant carrying it through (1, 1, 3/2, 1/6, 1/4) and the activation's own
    bar at the float64 z (0 for relu, u |z| for leaky's product)."""
    z, m = _bn_z(x, rm, rv, eps, g, b)
    bound = R.ACT_LIPSCHITZ[kind] * 7 * U * m
    if kind == "leaky":
        bound = bound + U * z.abs()
    elif kind in ("hswish", "hsigmoid", "sigmoid"):
        bound = bound + R.act_fwd_bound(z, kind, meas)
    ref = z if kind == "none" else R.act_fwd(z, kind)
    assert bool(got.isfinite().all())
    ok, worst = _within(got, ref, bound)
    assert ok, (kind, worst)


def _bn_params(C, seed):
    rm, g, b = R.randn((C,), seed, 2.0), R.randn((C,), seed + 1), R.randn((C,), seed + 2)
    rv = torch.rand(C, generator=torch.Generator().manual_seed(seed + 3)) + 0.5
    rv[0] = 0.0          # only eps under the root
    rv[-1] = 1e4 if C > 1 else 0.0
    return rm, rv, g, b


@gpu
@pytest.mark.parametrize("kind", ("none",) + KINDS)
def test_bn_eval(cuda, kind):
    """C = 1, 3, 10, 257 by M = 0, 1, 7 rows, running_var holding 0 and 1e4,
    each activation fused."""
    cases = []
    for C in (1, 3, 10, 257):
        p = _bn_params(C, 80 + C)
        cases += [(R.randn((M, C), 90 + M, 3.0) + p[0],) + p for M in (0, 1, 7)]
    meas = 0.0
    if kind == "sigmoid":  # torch's float32 sigmoid error over every z of this test
        zs = [_bn_z(x, rm, rv, 1e-5, g, b)[0].flatten() for x, rm, rv, g, b in cases]
        meas = R.sigmoid_measured(torch.cat(zs).float())
    for x, rm, rv, g, b in cases:
        _bn_check(_bn_gpu(cuda, x, rm, rv, 1e-5, g, b, kind), x, rm, rv, 1e-5, g, b, kind, meas)


@gpu
def test_bn_eval_mean_far_above_spread(cuda):
    """x = 1000 + 0.05 randn against a running mean of about 1000: x - mean is
    exact in float32 up to its own rounding, so the bar stays 7 u M with M of
    the order of |x - mean| / std.  A kernel folding the affine map into
    x * scale + shift errs by about 1000 u scale, thousands of times the bar."""
    C, M = 10, 7
    rm = 1000.0 + R.randn((C,), 100, 0.01)
    rv = torch.full((C,), 2.5e-3)
    g, b = R.randn((C,), 101), R.randn((C,), 102)
    x = 1000.0 + R.randn((M, C), 103, 0.05)
    _bn_check(_bn_gpu(cuda, x, rm, rv, 1e-5, g, b, "none"), x, rm, rv, 1e-5, g, b, "none")
    _bn_check(_bn_gpu(cuda, x, rm, rv, 1e-5, g, b, "hswish"), x, rm, rv, 1e-5, g, b, "hswish")


@gpu
def test_bn_eval_past_the_grid_cap(cuda):
    """M = 8200, C = 257: M C = 2 107 400 > 8192 * 256, the size at which a
    one-element-per-thread launch would run out of workgroups; the kernel's
    grid (one workgroup per 1024 elements) strides four times over it, with
    i % C taken of the strided index."""
    C, M = 257, 8200
    rm, rv, g, b = _bn_params(C, 110)
    x = R.randn((M, C), 111, 3.0) + rm
    _bn_check(_bn_gpu(cuda, x, rm, rv, 1e-5, g, b, "hswish"), x, rm, rv, 1e-5, g, b, "hswish")


# ================================================================ 5. channel scale
@gpu
@pytest.mark.parametrize("B,HW,C", [(3, 1, 4), (2, 5, 12), (1, 257, 40), (2, 32771, 128)])
def test_channel_scale(cuda, B, HW, C):
    """y = x * s[b][c], one rounding: bit for bit against the float32 product,
    every (b, c) with a scale of its own.  (2, 32771, 128) is 2 097 344 float4,
    past the 8192 * 256 of one trip: the image index of the second trip's
    elements must still come out as 1."""
    x = R.randn((B, HW, C), 120 + C)
    s = 0.5 + torch.arange(B * C, dtype=torch.float32).view(B, C) / 64
    out = Guarded(cuda, x.numel())
    _call("jabd_channel_scale_f32", _at(cuda, x), B, HW, C, _at(cuda, s),
          out)
    assert torch.equal(out.result().view(B, HW, C), x * s[:, None, :])


@gpu
def test_channel_scale_refuses_c6(cuda):
    x = torch.zeros(2 * 5 * 6, device=cuda)
    _refused("jabd_channel_scale_f32", x, 2, 5, 6, x, x)


# =============================================================== 6. scale backward
@gpu
@pytest.mark.parametrize("HW,nblk", [(1, 1), (5, 4), (300, 1), (513, 2), (70, 64), (16641, 64)])
def test_scale_bwd(cuda, HW, nblk):
    """jabd_scale_bwd_f32, B = 2, C = 4, 12, 260.  per = ceil(HW / nblk), so
    (5, 4) leaves block 3 and (70, 64) blocks 35..63 without a pixel: part is
    NaN before the call and must be finite everywhere after it (ScaleFn passes
    nblk = clamp(HW // 256, 1, 64), so Python cannot make an empty block
    today).  dx = da * s: bit for bit.  ds = the float64 sum of the block
    partials: HW fused multiply-adds and the adds joining them, bar
    (HW + 1) 2^-24 sum|da x|."""
    B = 2
    for C in (4, 12, 260):
        da, x = R.randn((B, HW, C), 130 + C), R.randn((B, HW, C), 131 + C, 2.0)
        s = 0.25 + torch.arange(B * C, dtype=torch.float32).view(B, C) / 32
        part, dx = Guarded(cuda, B * nblk * C), Guarded(cuda, B * HW * C)
        _call("jabd_scale_bwd_f32", _at(cuda, da), _at(cuda, x), B, HW, C,
              _at(cuda, s), part, nblk, dx)
        _, ds, ds_abs = R.scale_bwd(da.double(), x.double(), s.double())
        p = part.result().view(B, nblk, C)
        assert bool(p.isfinite().all()), C
        assert torch.equal(dx.result().view(B, HW, C), da * s[:, None, :]), C
        ok, worst = _within(p.double().sum(1), ds, (HW + 1) * U * ds_abs)
        assert ok, (C, worst)


def _conv_abs(w, t):
    """sum_t |w_t| t[b][c + t - h] (zero padded), t [B, C] >= 0."""
    k = w.numel()
    return F.conv1d(t.unsqueeze(1), w.abs().view(1, 1, k), padding=(k - 1) // 2).squeeze(1)


def _conv_abs_t(w, t):
    """The transposed sum: sum_t |w_t| t[b][c - t + h]."""
    return _conv_abs(w.flip(0), t)


ECA_CASES = [(2, 1, 1, 8, 3), (1, 3, 5, 12, 3), (2, 17, 16, 40, 5)]
KINK_MARGIN = 0.05


def _eca_inputs(B, H, W, C, k):
    """x (NCHW), the taps, the cotangent, the float64 pooled means and gate inputs.
    Each (b, c) plane is randn / 2 shifted to a mean drawn from U(-2.6, 2.6), so
    no pooled mean comes within 0.4 of +-3.  The taps are a fixed pattern scaled
    so that 3 is the geometric middle of the widest (ratio) gap between adjacent
    sorted |conv1d(mean)| in their 30%..70% quantile range: about half the gates
    saturate and none sits on a kink."""
    g = torch.Generator().manual_seed(140 + C)
    m = torch.empty((B, C, 1, 1), dtype=torch.float64).uniform_(-2.6, 2.6, generator=g)
    r = torch.randn((B, C, H, W), generator=g, dtype=torch.float64) * 0.5
    x = (r - r.mean((2, 3), keepdim=True) + m).float()
    u = torch.tensor([0.6, 1.7, -0.5] if k == 3 else [0.3, -0.8, 1.9, 0.7, -0.4],
                     dtype=torch.float64)
    mean = x.double().mean((2, 3))
    z0 = R.eca_fwd(x.double(), u, "hsigmoid")[1].abs().flatten().sort().values
    lo, hi = int(0.3 * z0.numel()), int(0.7 * z0.numel())
    j = lo + int((z0[lo + 1:hi + 1] / z0[lo:hi]).argmax())
    w = (u * 3.0 / float((z0[j] * z0[j + 1]).sqrt())).float()
    da = R.randn((B, C, H, W), 141 + C)
    return x, w, da, mean, R.eca_fwd(x.double(), w.double(), "hsigmoid")[1]


@functools.lru_cache(maxsize=None)
def _eca_sigmoid_measured():
    """torch's float32 sigmoid error over the gate inputs of all ECA cases."""
    zs = [R.eca_fwd(c[0].double(), c[1].double(), "sigmoid")[1].flatten()
          for c in (_eca_inputs(*case) for case in ECA_CASES)]
    return R.sigmoid_measured(torch.cat(zs).float())


@pytest.mark.parametrize("B,H,W,C,k", ECA_CASES)
def test_eca_inputs_stay_off_the_kinks(B, H, W, C, k):
    """By construction no pooled mean and no gate input of the ECA cases comes
    within 0.05 of +-3, and the hardsigmoid gate meets all three regions."""
    _, _, _, mean, z = _eca_inputs(B, H, W, C, k)
    assert float((mean.abs() - 3).abs().min()) > 0.39
    assert float((z.abs() - 3).abs().min()) > KINK_MARGIN
    assert bool((z > 3).any()) and bool((z < -3).any()) and bool((z.abs() < 3).any())


@gpu
@pytest.mark.parametrize("gate", ["sigmoid", "hsigmoid"])
@pytest.mark.parametrize("B,H,W,C,k", ECA_CASES)
def test_eca_bwd(cuda, gate, B, H, W, C, k):
    """jabd_eca_bwd_f32 through EcaScaleFn against the float64 autograd of
    x * gate(conv1d(mean_hw(x))), dx and the tap gradient.

    Bar, propagated term by term through the float64 graph with every term
    replaced by its magnitude (n = HW, m| | = mean_hw|x|, Z| | = sum|w| m| |):
      gate      ds_ = Lg (n + k + 4) u Z| | + Eg     Lg = 1/4, Eg = 4x torch's
                float32 sigmoid error; Lg = 1/6, Eg = 2 u for hardsigmoid
      ds        (n + 1) u sum|da x|                  the sequential-sum rule
      gate'     sigmoid s (1 - s): ds_ + 2 u; hardsigmoid 1/6: u / 6, the
                region being the reference's (means and z kept 0.05 from +-3:
                test_eca_inputs_stay_off_the_kinks, and asserted here)
      dz        ds-error * gate' + |ds| gate'-error + u |dz|
      dmean     sum|w| dz-error + (k + 1) u sum|w||dz|, then / n with 2 more
      dx        |da| ds_ + dmean-error + 2 u (|da s| + |dmean|)
      dw        sum (dz-error m| | + |dz| (n + 3) u m| |) + (B C + 1) u sum|dz| m| |
    """
    from jabd_amd.modules import EcaScaleFn
    n = H * W
    x, w, da, mean, _ = _eca_inputs(B, H, W, C, k)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr, z = R.eca_fwd(xr, wr, gate)
    gx, gw = torch.autograd.grad(yr, (xr, wr), da.double())
    if gate == "hsigmoid":  # the pooled means and the gate inputs stay off the kinks
        assert float((mean.abs() - 3).abs().min()) > KINK_MARGIN
        assert float((z.detach().abs() - 3).abs().min()) > KINK_MARGIN

    xg = x.to(cuda).permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    wg = w.to(cuda).view(1, 1, k).requires_grad_(True)
    y = EcaScaleFn.apply(xg, wg, gate)
    dx, dw = torch.autograd.grad(y, (xg, wg), da.to(cuda).permute(0, 2, 3, 1).contiguous())
    dx, dw = dx.cpu().permute(0, 3, 1, 2), dw.cpu().view(k)

    wd, xd, dd = w.double(), x.double(), da.double()
    m_abs = xd.abs().mean((2, 3))
    zd = z.detach()
    if gate == "sigmoid":
        s = torch.sigmoid(zd)
        d_s = 0.25 * (n + k + 4) * U * _conv_abs(wd, m_abs) + 4 * _eca_sigmoid_measured()
        gd = s * (1 - s)
        d_gd = d_s + 2 * U
    else:
        s = F.hardsigmoid(zd)
        d_s = (n + k + 4) * U * _conv_abs(wd, m_abs) / 6 + 2 * U
        gd = ((zd > -3) & (zd < 3)).double() / 6
        d_gd = torch.full_like(gd, U / 6)
        assert float((d_s * 6).max()) < KINK_MARGIN / 100   # the margin dwarfs z's float32 error
    ds_abs = (dd * xd).abs().sum((2, 3))
    d_dz = (n + 1) * U * ds_abs * gd + ds_abs * d_gd + U * ds_abs * gd
    dz_abs = ds_abs * gd
    dm_abs = _conv_abs_t(wd, dz_abs) / n
    d_dm = (_conv_abs_t(wd, d_dz) + (k + 3) * U * _conv_abs_t(wd, dz_abs)) / n
    das = dd.abs() * s[:, :, None, None]
    bound_x = dd.abs() * d_s[:, :, None, None] + d_dm[:, :, None, None] + \
        2 * U * (das + dm_abs[:, :, None, None])
    ok, worst = _within(dx, gx, bound_x)
    assert ok, ("dx", worst)
    h = (k - 1) // 2
    pad = lambda t: F.pad(t, (h, h))  # noqa: E731
    bound_w = torch.stack([
        ((d_dz + (n + 3 + B * C + 1) * U * dz_abs) * pad(m_abs)[:, t:t + C]).sum()
        for t in range(k)])
    ok, worst = _within(dw, gw, bound_w)
    assert ok, ("dw", worst)


# ============================================================= 7. nearest up-sample
@gpu
@pytest.mark.parametrize("src,dst", NEAREST)
def test_upsample_nearest(cuda, src, dst):
    """jabd_upsample_nearest_f32 (a copy: exact), jabd_upsample_nearest_add_f32
    with a non-zero lateral (one add: bit for bit) and
    jabd_upsample_nearest_bwd_f32 with accumulate 0 and 1 against the float64
    scatter-add: a source sums its n preimage pixels (and the value dsrc held),
    bar (n + 1) 2^-24 sum|terms|.  B = 3, C = 4 and 12."""
    (hs, ws), (h, w) = src, dst
    B = 3
    for C in (4, 12):
        s, lat = R.randn((B, hs, ws, C), 150 + C), R.randn((B, h, w, C), 151 + C)
        up = R.nearest_fwd(s, h, w)
        out = Guarded(cuda, B * h * w * C)
        _call("jabd_upsample_nearest_f32", _at(cuda, s), B, hs, ws, h, w, C, out)
        assert torch.equal(out.result().view(B, h, w, C), up)
        out = Guarded(cuda, B * h * w * C)
        _call("jabd_upsample_nearest_add_f32", _at(cuda, s), B, hs, ws, h, w, C,
              _at(cuda, lat), out)
        assert torch.equal(out.result().view(B, h, w, C), lat + up)

        g, held = R.randn((B, h, w, C), 152 + C), R.randn((B, hs, ws, C), 153 + C)
        n = R.nearest_bwd(torch.ones((1, h, w, 1), dtype=torch.float64), hs, ws)
        for acc in (0, 1):
            out = Guarded(cuda, B * hs * ws * C)
            if acc:
                out.view.copy_(held.reshape(-1))
            _call("jabd_upsample_nearest_bwd_f32", _at(cuda, g), B, h, w, hs, ws, C,
                  acc, out)
            ref = R.nearest_bwd(g.double(), hs, ws) + acc * held.double()
            mag = R.nearest_bwd(g.double().abs(), hs, ws) + acc * held.double().abs()
            ok, worst = _within(out.result().view(B, hs, ws, C), ref, (n + acc + 1) * U * mag)
            assert ok, (C, acc, worst)


@gpu
def test_upsample_nearest_refuses_downsampling(cuda):
    big, small = torch.zeros(3 * 8 * 8 * 4, device=cuda), torch.zeros(3 * 4 * 4 * 4, device=cuda)
    # backward: dxup [h, w] = 4 x 4, dsrc [hs, ws] = 8 x 4
    _refused("jabd_upsample_nearest_bwd_f32", small, 3, 4, 4, 8, 4, 4, 0,
             big)
    # up-sample + add: src 8 x 4 onto a 4 x 4 lateral
    _refused("jabd_upsample_nearest_add_f32", big, 3, 8, 4, 4, 4, 4, small,
             small)


# ================================================================== 8. max-pool 3/2/1
@gpu
@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (2, 9)])
def test_maxpool_tiny_maps(cuda, H, W):
    """jabd_maxpool_nhwc_f32 and jabd_maxpool_idx_nhwc_f32 against torch's CPU
    max_pool2d(3, 2, 1): a selection, bit for bit (inputs all distinct, so no
    tie decides).  jabd_maxpool_bwd_idx_f32 and the recomputing
    jabd_maxpool_bwd_f32 against CPU autograd in float64: a pixel sums the dy of
    the n <= 4 windows it wins, bar (n + 1) 2^-24 sum|dy terms|.  C = 4 (the
    row kernel), 12 (C / 4 not a power of two) and 512 (C / 4 above 64)."""
    B = 2
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    for C in (4, 12, 512):
        x, dy = R.distinct((B, H, W, C), 160 + C), R.randn((B, OH, OW, C), 161 + C)
        y_ref = R.torch_maxpool(x)
        assert y_ref.shape == (B, OH, OW, C)
        _, dx_ref = R.torch_maxpool(x.double(), dy.double())
        _, mag = R.torch_maxpool(x.double(), dy.double().abs())
        _, n = R.torch_maxpool(x.double(), torch.ones_like(dy, dtype=torch.float64))
        xd, dyd = _at(cuda, x), _at(cuda, dy)

        y = Guarded(cuda, y_ref.numel())
        _call("jabd_maxpool_nhwc_f32", xd, B, H, W, C, 3, 2, 1, y)
        assert torch.equal(y.result().view_as(y_ref), y_ref), C

        y = Guarded(cuda, y_ref.numel())
        idx = torch.full((y_ref.numel() + 64,), 255, dtype=torch.uint8, device=cuda)
        _call("jabd_maxpool_idx_nhwc_f32", xd, B, H, W, C, 3, 2, 1, y,
              idx)
        assert torch.equal(y.result().view_as(y_ref), y_ref), C
        ic = idx.cpu()
        assert bool((ic[:y_ref.numel()] < 9).all()) and bool((ic[y_ref.numel():] == 255).all())

        for name, first in (("jabd_maxpool_bwd_idx_f32", idx), ("jabd_maxpool_bwd_f32", xd)):
            dx = Guarded(cuda, x.numel())
            _call(name, first, dyd, B, H, W, C, 3, 2, 1, dx)
            ok, worst = _within(dx.result().view_as(x), dx_ref, (n + 1) * U * mag)
            assert ok, (name, C, worst)
