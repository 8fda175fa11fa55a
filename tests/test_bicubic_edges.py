"""Bicubic align_corners resize (csrc/upsample.hip) over every small ratio,
against F.interpolate in float64 on the CPU (tests/_small_kernel_ref.py).

The backward gathers: each input element sums the outputs inside out_range's
window, a hand-derived bound.  An output the window misses is a silently wrong
gradient, so the sweep runs every n -> on with n in 1..9 and on in 1..20 along
each axis — up-sampling to 19x, down-sampling to 1/9, on == 1 and n == 1 (the
`scale <= 0` window: every output reads the input) — and, besides the fp64
parity, checks an invariant that needs no reference: the four cubic weights of
an output sum to 1, so with grad_y = 1 every (b, c) plane of grad_x sums to
OH * OW; a missed output takes its weight out of that sum.

Which case reaches which branch:
  out_range scale <= 0 (n == 1 or on == 1)   the sweep's n = 1 column and on = 1
                                             row; (1,1,4,4,4), (9,1,1,9,5)
  out_range lo / hi windows, down-sampling   (20,20,7,7,8), (64,48,5,3,4)
  high up-sampling, all taps clamped         (2,2,37,41,3)
  non-integer ratio, C over one wavefront    (13,7,25,13,40)
  scale == 1: weights exactly (0, 1, 0, 0)   (7,13,7,13,4), bit-exact both ways
  batch == 0                                 test_bicubic_batch_zero

Bars: test_bicubic.py's own 1e-5, forward and backward, relative to the max
magnitude.  fp32 and fp64 may pick different floor(scale * o), but the cubic
kernel is continuous there, so the two still agree to fp32 rounding.  The
plane sums are held to 1e-5 * OH * OW.

Worst error measured on the MI355X: the sweep 1.0e-6 forward, 9.4e-7 backward,
1.6e-7 plane sums; the parity cases 1.3e-6 forward, 1.2e-6 backward (both on
(20,20,7,7,8)), 1.2e-7 plane sums.
"""
import ctypes

import pytest
import torch

import _small_kernel_ref as R
from _util import rel_err

BAR = 1e-5
CASES = [(20, 20, 7, 7, 8), (64, 48, 5, 3, 4), (2, 2, 37, 41, 3), (13, 7, 25, 13, 40),
         (1, 1, 4, 4, 4), (9, 1, 1, 9, 5)]


def _run(cuda, x_nchw, size, wts_nchw):
    """Forward and the gradient of sum(out * wts) on the device, as NCHW."""
    from jabd_amd import ops
    xg = x_nchw.permute(0, 2, 3, 1).contiguous().to(cuda).requires_grad_(True)
    out = ops.upsample_bicubic(xg, size)
    out.backward(wts_nchw.permute(0, 2, 3, 1).contiguous().to(cuda))
    return out.detach().permute(0, 3, 1, 2).cpu(), xg.grad.permute(0, 3, 1, 2).cpu()


def _plane_sum_err(cuda, shape, size):
    """max over (b, c) planes of |sum(grad_x) - OH * OW| / (OH * OW) for grad_y = 1."""
    B, C, H, W = shape
    _, gx = _run(cuda, torch.zeros(shape), size, torch.ones(B, C, *size))
    n = size[0] * size[1]
    return float((gx.double().sum((2, 3)) - n).abs().max()) / n


def test_plane_sum_invariant_holds_in_fp64():
    """The invariant itself, on the CPU: it is a property of the operation."""
    for H, W, OH, OW, C in CASES:
        _, gx = R.bicubic_ref(torch.zeros(1, C, H, W), (OH, OW), torch.ones(1, C, OH, OW))
        assert float((gx.sum((2, 3)) - OH * OW).abs().max()) < 1e-9 * OH * OW


@pytest.mark.gpu
def test_bicubic_every_small_ratio(cuda):
    g = torch.Generator().manual_seed(5)
    worst = {"fwd": 0.0, "bwd": 0.0, "sum": 0.0}
    for n in range(1, 10):
        for on in range(1, 21):
            for shape, size in (((1, 1, n, 2), (on, 2)), ((1, 1, 2, n), (2, on))):
                x = torch.randn(shape, generator=g)
                wts = torch.randn(1, 1, *size, generator=g)
                ref, ref_gx = R.bicubic_ref(x, size, wts)
                got, got_gx = _run(cuda, x, size, wts)
                e = {"fwd": rel_err(got, ref), "bwd": rel_err(got_gx, ref_gx),
                     "sum": _plane_sum_err(cuda, shape, size)}
                assert max(e.values()) < BAR, (shape, size, e)
                worst = {k: max(worst[k], e[k]) for k in e}
    print("sweep worst:", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,OH,OW,C", CASES)
def test_bicubic_edge_parity(cuda, H, W, OH, OW, C):
    g = torch.Generator().manual_seed(H * 31 + OW)
    x = torch.randn(2, C, H, W, generator=g)
    wts = torch.randn(2, C, OH, OW, generator=g)
    ref, ref_gx = R.bicubic_ref(x, (OH, OW), wts)
    got, got_gx = _run(cuda, x, (OH, OW), wts)
    e = {"fwd": rel_err(got, ref), "bwd": rel_err(got_gx, ref_gx),
         "sum": _plane_sum_err(cuda, (2, C, H, W), (OH, OW))}
    print((H, W, OH, OW, C), e)
    assert max(e.values()) < BAR, e


@pytest.mark.gpu
def test_bicubic_same_size_is_the_identity(cuda):
    """scale == 1: t == 0 and the fp32 weights are exactly (0, 1, 0, 0), so both
    directions copy bit for bit."""
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 4, 7, 13, generator=g)
    wts = torch.randn(2, 4, 7, 13, generator=g)
    got, got_gx = _run(cuda, x, (7, 13), wts)
    assert torch.equal(got, x) and torch.equal(got_gx, wts)


@pytest.mark.gpu
def test_bicubic_batch_zero(cuda):
    from jabd_amd import ops
    from jabd_amd._lib import call
    null = ctypes.c_void_p(0)
    call("jabd_upsample_bicubic_ac_f32", null, 0, 5, 6, 4, null, 9, 7, ops._stream())
    call("jabd_upsample_bicubic_ac_bwd_f32", null, 0, 5, 6, 4, null, 9, 7, ops._stream())
    x = torch.empty(0, 5, 6, 4, device=cuda, requires_grad=True)
    y = ops.upsample_bicubic(x, (9, 7))
    assert y.shape == (0, 9, 7, 4)
    y.sum().backward()
    assert x.grad.shape == x.shape
