"""The default expand + depthwise kernel (expdw1_kernel, csrc/expdw.hip) on the
shapes where its depthwise phase takes only the full-tile path, and on shapes
where every tile is ragged: the launch witness must show the default form, and
y, the ECA partials and the fused skip branch must equal the wave-specialised
form (jabd_expand_dw_select(2), which shares none of the default form's
addressing) bit for bit.  Block 2's fused-project form is compared with the
separate launches, NaN placement included, and the output stores are checked
against a canary around channel-slice views (pixel stride > channels)."""
import ctypes

import pytest
import torch

from _util import rel_err

# (k, Cin, E, stride, act)
CASES = [(3, 16, 16, 1, "relu"),
         (3, 24, 72, 1, "relu"), (5, 24, 72, 2, "relu"),        # two stages, 8-channel tail
         (5, 40, 120, 1, "relu"), (3, 40, 240, 2, "hswish"),    # three stages
         (3, 80, 200, 1, "hswish"),                             # last 16-channel tile half empty
         (5, 112, 672, 2, "hswish"),                            # the SKC = 112 skip form
         (5, 160, 672, 1, "hswish")]
RAGGED = [(2, 15, 17), (2, 33, 9), (1, 1, 1)]


def _full(k, s):
    """(B, H, W) whose tiles all lie whole inside the output map: 14x16 tiles
    for 3x3/s1, 16x16 for 5x5/s1, 8x8 outputs for stride 2."""
    return (2, 28, 32) if (s == 1 and k == 3) else (2, 32, 32)


def _layer(k, cin, E, s, seed, cuda):
    from jabd_amd import functional as F
    g = torch.Generator().manual_seed(seed)
    conv1 = torch.nn.Conv2d(cin, E, 1)
    conv2 = torch.nn.Conv2d(E, E, k, s, k // 2, groups=E)
    sdw = torch.nn.Conv2d(cin, cin, 3, 2, 1, groups=cin)
    with torch.no_grad():
        for c in (conv1, conv2, sdw):
            c.weight.copy_(torch.randn(c.weight.shape, generator=g) / c.weight[0].numel() ** 0.5)
            c.bias.copy_(0.3 * torch.randn(c.bias.shape, generator=g))
    pk = F.pack_conv(conv1.to(cuda))

    def tapmajor(c):
        return (c.weight.detach().reshape(c.weight.shape[0], -1).t().contiguous().to(cuda),
                c.bias.detach().contiguous().to(cuda))

    return g, pk, tapmajor(conv2), tapmajor(sdw)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", CASES, ids=lambda s: "k%d_c%d_e%d_s%d" % s[:4])
@pytest.mark.parametrize("shape", ["full"] + RAGGED, ids=lambda b: b if b == "full" else "%dx%dx%d" % b)
def test_default_form_bit_equal_form2(cuda, spec, shape):
    from jabd_amd import _lib
    from jabd_amd import functional as F
    k, cin, E, s, act = spec
    B, H, W = _full(k, s) if shape == "full" else shape
    g, pk, (dw_w, dw_b), skip = _layer(k, cin, E, s, k * 7 + cin + E + H, cuda)
    x = torch.randn(B, H, W, cin, generator=g).to(cuda)
    kw = {"act": act, "skip": skip} if s == 2 else {"act": act}
    _lib.launch_log_reset()
    got = F.expand_dw(x, pk, dw_w, dw_b, k, s, **kw)
    assert _lib.launch_log() == [("expand_dw", 0)], _lib.launch_log()
    try:
        _lib.lib().jabd_expand_dw_select(2)
        _lib.launch_log_reset()
        ref = F.expand_dw(x, pk, dw_w, dw_b, k, s, **kw)
        assert _lib.launch_log() == [("expand_dw_ws", 0)], _lib.launch_log()
    finally:
        _lib.lib().jabd_expand_dw_select(0)
    torch.cuda.synchronize()
    for i, (name, a, b) in enumerate(zip(("y", "partials", "skip"), got, ref)):
        if cin == 24 and i < 2:   # the 8-channel tail stage sums k in another order
            assert rel_err(a, b) < 1e-6, (name, rel_err(a, b))
        else:
            assert torch.equal(a, b), (name, rel_err(a, b))


def _block2(hw, B, act, cuda, nan=False):
    """Blocks 1 -> 2: (fused-project outputs, separate-launch outputs, launch log)."""
    from jabd_amd import _lib
    from jabd_amd import functional as F
    H, W = hw
    C, E = 16, 64
    g = torch.Generator().manual_seed(H * 7 + W)

    def conv_bn(cin, cout, k, s, groups=1):
        c = torch.nn.Conv2d(cin, cout, k, s, k // 2, groups=groups, bias=False)
        bn = torch.nn.BatchNorm2d(cout)
        with torch.no_grad():
            c.weight.copy_(torch.randn(c.weight.shape, generator=g) / c.weight[0].numel() ** 0.5)
            bn.weight.copy_(1 + 0.2 * torch.randn(cout, generator=g))
            bn.bias.copy_(0.3 * torch.randn(cout, generator=g))
            bn.running_mean.copy_(0.1 * torch.randn(cout, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(cout, generator=g))
        return c.eval().to(cuda), bn.eval().to(cuda)

    pk_p = F.pack_conv(*conv_bn(C, C, 1, 1))
    pk_e = F.pack_conv(*conv_bn(C, E, 1, 1))
    dw_w, dw_b = F.pack_dw(*conv_bn(E, E, 3, 2, groups=E))
    skip = F.pack_dw(*conv_bn(C, C, 3, 2, groups=C))
    d0 = torch.randn(B, H, W, C, generator=g).relu()
    x0 = torch.randn(B, H, W, C, generator=g)
    if nan:   # one residual element and one d element, at different in-image pixels
        x0[B - 1, H - 1, W // 2, 5] = float("nan")
        d0[0, H // 2, 0, 9] = float("nan")
    d0, x0 = d0.to(cuda), x0.to(cuda)
    gate = torch.rand(B, C, generator=g).to(cuda)
    out0 = F.conv(d0, pk_p, act=act, ascale=gate, res=x0)
    ref = F.expand_dw(out0, pk_e, dw_w, dw_b, 3, 2, act=act, skip=skip)
    _lib.launch_log_reset()
    got = F.expand_dw(d0, pk_e, dw_w, dw_b, 3, 2, act=act, skip=skip, pre=(pk_p, gate, x0, act))
    log = _lib.launch_log()
    torch.cuda.synchronize()
    return got, ref, log


BLOCK2_SHAPES = [(2, 32, 32), (2, 17, 19), (1, 1, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("bhw", BLOCK2_SHAPES, ids=lambda b: "%dx%dx%d" % b)
@pytest.mark.parametrize("act", ["relu", "hswish"])
def test_block2_fused_form(cuda, bhw, act):
    got, ref, log = _block2(bhw[1:], bhw[0], act, cuda)
    assert log == [("expand_dw (fused project, one chunk)", 0)], log
    for name, a, b in zip(("y", "partials", "skip"), got, ref):
        assert rel_err(a, b) < 1e-5, (name, rel_err(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("bhw", BLOCK2_SHAPES, ids=lambda b: "%dx%dx%d" % b)
@pytest.mark.parametrize("act", ["relu", "hswish"])
def test_block2_fused_form_nan_placement(cuda, bhw, act):
    """A NaN in the residual and one in d reach the same outputs as on the
    separate path (a residual tile loaded for the wrong pixel would move them)."""
    got, ref, log = _block2(bhw[1:], bhw[0], act, cuda, nan=True)
    assert log == [("expand_dw (fused project, one chunk)", 0)], log
    for name, a, b in zip(("y", "partials", "skip"), got, ref):
        na, nb = torch.isnan(a), torch.isnan(b)
        assert int(nb.sum()) > 0, name
        assert torch.equal(na, nb), (name, int(na.sum()), int(nb.sum()))
        if int((~nb).sum()):
            assert rel_err(a[~nb], b[~nb]) < 1e-5, (name, rel_err(a[~nb], b[~nb]))


CANARY = 1234.5


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [(3, 16, 64, 2, "relu"), (3, 40, 240, 2, "hswish"),
                                  (5, 24, 72, 2, "relu")], ids=lambda s: "k%d_c%d_e%d" % s[:3])
@pytest.mark.parametrize("bhw", [(2, 32, 32), (2, 17, 19)], ids=lambda b: "%dx%dx%d" % b)
def test_strided_outputs_leave_canary(cuda, spec, bhw):
    """y and the skip output as channel slices of wider tensors (y_ps > E,
    sy_ps > Cin): the slices equal the dense outputs bit for bit and the
    canary around them is untouched."""
    from jabd_amd import _lib
    from jabd_amd import functional as F
    from jabd_amd._lib import ExpDwArgs
    k, cin, E, s, act = spec
    B, H, W = bhw
    g, pk, (dw_w, dw_b), (skw, skb) = _layer(k, cin, E, s, 11 + cin + H, cuda)
    x = torch.randn(B, H, W, cin, generator=g).to(cuda)
    y0, part0, t0 = F.expand_dw(x, pk, dw_w, dw_b, k, s, act=act, skip=(skw, skb))
    OH, OW = y0.shape[1:3]
    ywide = torch.full((B, OH, OW, E + 12), CANARY, device=cuda)
    twide = torch.full((B, OH, OW, cin + 8), CANARY, device=cuda)
    y, t = ywide[..., 8:8 + E], twide[..., 4:4 + cin]
    part = torch.empty_like(part0)
    a = ExpDwArgs()
    a.x, a.x_bs, a.x_ps, a.Cin = x.data_ptr(), x.stride(0), cin, cin
    a.B, a.H, a.W, a.E = B, H, W, E
    a.we, a.be, a.Ntiles, a.Kc = pk.w.data_ptr(), pk.bias.data_ptr(), pk.Ntiles, pk.Kc
    a.wd, a.bd = dw_w.data_ptr(), dw_b.data_ptr()
    a.k, a.stride, a.act = k, s, F.ACT[act]
    a.y, a.y_bs, a.y_ps, a.OH, a.OW = y.data_ptr(), y.stride(0), y.stride(2), OH, OW
    a.nblk, a.part = part.shape[1], part.data_ptr()
    a.sw, a.sb = skw.data_ptr(), skb.data_ptr()
    a.sy, a.sy_bs, a.sy_ps = t.data_ptr(), t.stride(0), t.stride(2)
    _lib.launch_log_reset()
    _lib.call("jabd_expand_dw_nhwc_f32", ctypes.byref(a), F._stream())
    assert _lib.launch_log() == [("expand_dw", 0)], _lib.launch_log()
    torch.cuda.synchronize()
    assert torch.equal(y, y0) and torch.equal(t, t0) and torch.equal(part, part0)
    assert bool((ywide[..., :8] == CANARY).all()) and bool((ywide[..., 8 + E:] == CANARY).all())
    assert bool((twide[..., :4] == CANARY).all()) and bool((twide[..., 4 + cin:] == CANARY).all())
