"""Operator-level parity of the conv backward dispatch, one case per kernel
instance, with the launch witness telling which kernel produced the numbers.

Weight gradient: jabd_conv_wgrad_f32 (csrc/train.hip) picks stem_wgrad, the
stem7 form, one of eight conv_wgrad32_kernel<KT,NT,DB>, one of nine
conv_wgrad_v_kernel<KT,NT> or the scalar conv_wgrad_kernel over chunks of
pixels, then wgrad_reduce2_kernel in its 16- or 64-lane form.  Data gradient:
jabd_conv2d_nhwc_f32 with tconv = 1 over the transposed weight pack reaches the
32x32 tile GEMM's transposed k x k form, its four stride-2 sub-pixel phase
launches, conv3x3_tile's or conv_gemm's transposed form; a 1x1 / stride-1 data
gradient is a plain 1x1 (tconv = 0) over that pack.  The C entries are called
directly with hand-filled ConvArgs (as jabd_amd.train._wgrad / _conv_args do),
so the cases set the channel windows.  Every case

 1. asserts the launch log (kernel name and instance tag)
    against the route read off the dispatch code,
 2. checks the output against the float64 reference within the derived fp32
    bound of tests/_convgrad_ref.py (no measured constant), and
 3. checks the canaries: x and dy carry 4 NaN channels on each side of their
    window, gate rows a NaN tail; dw sits NaN-filled inside a larger NaN
    buffer, the partials are sized exactly by jabd_conv_wgrad_part_floats and
    followed by NaN guard floats; dx is NaN-filled with 4 extra channels on
    each side.  Outputs must come back finite, guards must stay NaN.

The exact-addressing probes run the weight-gradient families on a 3 x 67 x 65
map (M = 13065, 205 chunks) with a one-hot dy: dW[n] must then be the input
patch of that pixel bit for bit and every other dW[n'] exactly zero; for the
data-gradient families a one-hot dy must scatter the weight taps bit for bit.

Not covered: the depthwise gradient kernels (test_dwconvfn_grads* in
tests/test_train_ops.py), the JABD_* A/B environment forms (cached per
process), TM = 4 of conv_gemm, jabd_conv_wgrad_eca_f32's own reductions
(test_wgrad_eca there, which asserts the witness tag too).
"""
import ctypes

import pytest
import torch
from torch.nn.grad import conv2d_input, conv2d_weight

import _convgrad_ref as G
from _convref import check

NAN = float("nan")
GUARD = 64   # NaN floats on each side of dw and after the partials

# witness tag of a conv_wgrad launch: family * 1000000 + KT * 1000 + NT
SCALAR, V, W32, W32DB = 1, 2, 3, 4


def _t(family, kt, nt):
    return ("conv_wgrad", family * 1000000 + kt * 1000 + nt)


R16, R64 = ("wgrad_reduce", 16), ("wgrad_reduce", 64)
M32 = "conv1x1_m32"

# case -> launch log: the route read off csrc/train.hip (jabd_conv_wgrad_f32,
# wgrad_launch_parts, wgrad_vec_ok, wgrad32_ok, wg32_tile, wv_tile, stem_wgrad_ok,
# stem7_wgrad_on).  K = KH * KW * Cin.  wgrad32 needs K >= 64 and Cout >= 64;
# wg32_tile(n) is 128 when padding n to 128s wastes at most n / 8, else 64;
# wv_tile(n) is 16 / 32 / 64 for n <= 16 / <= 32 / above.  The reduce takes 64
# lanes when K * Cout >= 32768, else 16.
WROUTES = {
    # 1x1 / s1 / pad 0 with H == OH: the double-buffered form
    "f32_64_64": [_t(W32DB, 64, 64), R16],        # K 64, Cout 64: 128s would waste 64 > 8
    "f32_64_128": [_t(W32DB, 64, 128), R16],      # Cout 128 fills a 128 tile
    "f32_128_64": [_t(W32DB, 128, 64), R16],
    "f32_120_120": [_t(W32DB, 128, 128), R16],    # 8 wasted <= 120 / 8; K * Cout = 14400
    "f32_64_96": [_t(W32DB, 64, 64), R16],        # 96: 32 wasted > 12 -> two 64 tiles
    "f32_120_64_gated": [_t(W32DB, 128, 64), R16],
    # 3x3 or stride 2: the single-buffered form
    "g32_3x3_8_64": [_t(W32, 64, 64), R16],       # K 72: 56 wasted > 9 -> 64 tiles
    "g32_3x3_8_128": [_t(W32, 64, 128), R16],
    "g32_3x3_64_64": [_t(W32, 128, 64), R64],     # K 576: 640 - 576 = 64 <= 72; 36864 outputs
    "g32_3x3s2_64_128_odd": [_t(W32, 128, 128), R64],
    "g32_3x3s2_64_128_even": [_t(W32, 128, 128), R64],
    "g32_1x1s2_64_64": [_t(W32, 64, 64), R16],    # stride 2: not the fast form
    "g32_3x3_64_64_gated": [_t(W32, 128, 64), R64],
    # K < 64 or Cout < 64: conv_wgrad_v, (wv_tile(K), wv_tile(Cout))
    "v_16_16": [_t(V, 16, 16), R16], "v_16_24": [_t(V, 16, 32), R16],
    "v_16_64": [_t(V, 16, 64), R16], "v_24_16": [_t(V, 32, 16), R16],
    "v_24_24": [_t(V, 32, 32), R16], "v_24_72": [_t(V, 32, 64), R16],
    "v_72_16": [_t(V, 64, 16), R16],              # K 72 >= 64 but Cout 16 < 64
    "v_72_24": [_t(V, 64, 32), R16],
    "v_40_40": [_t(V, 64, 64), R16],
    "v_3x3_8_24": [_t(V, 64, 32), R16],           # K 72, Cout 24 < 64
    "v_24_24_gated": [_t(V, 32, 32), R16],
    # wgrad_vec_ok fails: the scalar kernel, 64 x 64 tiles
    "s_cin10": [_t(SCALAR, 64, 64), R16],         # Cin % 4 != 0 (and x_ps 18)
    "s_cout18": [_t(SCALAR, 64, 64), R16],        # Cout % 4 != 0 (and y_ps 26)
    "s_xc0_2": [_t(SCALAR, 64, 64), R16],         # x_c0 % 4 != 0
    "s_ybs": [_t(SCALAR, 64, 64), R16],           # y_bs != OH * OW * y_ps
    "s_gate_pitch": [_t(SCALAR, 64, 64), R16],    # ascale_bs % 4 != 0
    "s_nchw": [_t(SCALAR, 64, 64), R16],          # NCHW input, Cout 32 > 16: not stem_wgrad
    # NCHW input, K <= 32, Cout <= 16, stride <= 2: stem_wgrad (16-lane reduce)
    "stem_3x3": [("stem_wgrad", 0), R16],
    "stem_5x5": [("stem_wgrad", 0), R16],
    "stem_w64": [("stem_wgrad", 0), R16],
    # NCHW 3 -> 64 7x7 / s2 with float4-aligned dy rows: the stem7 form (64-lane reduce)
    "stem7_1x3": [("stem7_wgrad", 0), R64],
    "stem7_40x44": [("stem7_wgrad", 0), R64],
}

# case -> launch log: csrc/conv.hip (jabd_conv2d_nhwc_f32, conv_m32_route, use_conv32,
# conv3x3_tile_on, dispatch_conv), csrc/conv32.hip (launch_m32_as, m32_tile,
# jabd_conv_pack_tn32), csrc/conv_stream.hip.  The entry sees the transposed
# conv: its Cin is the forward Cout (dy's channels), its Cout the forward Cin.
DROUTES = {
    # k x k on the tile GEMM: entry Cin % 32 == 0, entry Cout >= 64, K >= 288;
    # tag 100 + tn32 of the entry Cout
    "m32_3x3_64_64": [(M32, 102)],
    "m32_3x3_128_64": [(M32, 104)],               # 128 dx channels: tn32 4
    # stride 2: one launch per non-empty sub-pixel phase
    "ph_64_64_10x11": [(M32, 102)] * 4, "ph_64_64_11x10": [(M32, 102)] * 4,
    "ph_128_128_10x11": [(M32, 104)] * 4, "ph_128_128_11x10": [(M32, 104)] * 4,
    "ph_64_64_h1": [(M32, 102)] * 2,              # one dx row: the odd-row phases are skipped
    "ph_1x1_512_256": [(M32, 104)] * 4,           # 1x1: entry Cout 512 >= 96, K 256 >= 96
    # 3x3 / s1 / pad 1, entry Cin 40 (not % 32, <= 64), tn 3: conv3x3_tile, 2 rows per wave
    "t3_40_40_9x10": [("conv3x3_tile", 203)],
    "t3_40_40_64x17": [("conv3x3_tile", 203)],
    # conv_gemm: tag 100 TM + tn; TM 1 on these small grids
    "gemm_3x3s2_12_10": [("conv_gemm", 101)],     # entry Cin 10: scalar loads; tn(12) = 1
    "gemm_3x3s2_48_96": [("conv_gemm", 103)],     # entry Cout 48 < 64: no tile GEMM; stride 2: no 3x3 tile
    "gemm_1x1s2_96_64": [("conv_gemm", 108)],     # 1x1 needs K >= 96 for the tile GEMM; K is 64
    # plain 1x1 over the transposed pack
    "p_m32_128_96": [(M32, 104)],                 # entry 96 -> 128: 3 K stages, not the streaming m32s
    "p_stream_64_16": [("conv1x1_stream", 104)],  # entry 16 -> 64: Kc 1, 4 N tiles
    "p_1x1_120_40": [("conv1x1", 108)],           # entry 40 -> 120: 8 N tiles > 5, no streaming instance
}


def _nhwc(v, lo, hi, cuda):
    """NCHW CPU -> NHWC GPU with lo / hi NaN channels around the window."""
    b, ch, h, w = v.shape
    buf = torch.full((b, h, w, lo + ch + hi), NAN)
    buf[..., lo:lo + ch] = v.permute(0, 2, 3, 1)
    return buf.to(cuda)


def _cdiv(a, b):
    return -(-a // b)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_wgrad(cuda, x, dy, gate, wshape, stride, pad, nchw=False, x_c0=4, y_bs_pad=0,
              gate_pad=4):
    """jabd_conv_wgrad_f32 on CPU operands (NCHW) with the canaries; returns
    (dW on the CPU, launch log, chunk length) after asserting the guards."""
    from jabd_amd import _lib
    cout, cin, kh, kw = wshape
    B, _, H, W = x.shape
    OH, OW = dy.shape[2], dy.shape[3]
    a = _lib.ConvArgs()
    if nchw:   # no channel window: NaN floats before and after the whole input
        xb = torch.full((x.numel() + 8,), NAN)
        xb[4:-4] = x.reshape(-1)
        xb = xb.to(cuda)
        a.x, a.x_bs, a.x_ps = xb.data_ptr() + 16, cin * H * W, 1
    else:
        xb = _nhwc(x, x_c0, 8 - x_c0, cuda)
        a.x, a.x_bs, a.x_ps, a.x_c0 = xb.data_ptr(), H * W * (cin + 8), cin + 8, x_c0
    a.B, a.H, a.W, a.Cin = B, H, W, cin
    if gate is not None:
        gb = torch.full((B, cin + gate_pad), NAN)
        gb[:, :cin] = gate
        gb = gb.to(cuda)
        a.ascale, a.ascale_bs = gb.data_ptr(), cin + gate_pad
    y_ps = cout + 8
    yb = torch.full((B, OH * OW * y_ps + y_bs_pad), NAN)
    yb[:, :OH * OW * y_ps].view(B, OH, OW, y_ps)[..., 4:4 + cout] = dy.permute(0, 2, 3, 1)
    yb = yb.to(cuda)
    a.y, a.y_bs, a.y_ps, a.y_c0 = yb.data_ptr(), OH * OW * y_ps + y_bs_pad, y_ps, 4
    a.OH, a.OW, a.Cout = OH, OW, cout
    a.KH, a.KW, a.stride, a.pad = kh, kw, stride, pad
    a.nchw_in = 1 if nchw else 0
    nparts = int(_lib.lib().jabd_conv_wgrad_part_floats(ctypes.byref(a)))
    n = cout * cin * kh * kw
    assert nparts > 0 and nparts % n == 0
    part = torch.full((nparts + GUARD,), NAN, device=cuda)
    dwb = torch.full((GUARD + n + GUARD,), NAN, device=cuda)
    _lib.launch_log_reset()
    _lib.call("jabd_conv_wgrad_f32", ctypes.byref(a), part.data_ptr(),
              dwb.data_ptr() + 4 * GUARD, _stream())
    log = _lib.launch_log()
    torch.cuda.synchronize()
    dwb, tail = dwb.cpu(), part[nparts:].cpu()
    assert bool(torch.isnan(dwb[:GUARD]).all()) and bool(torch.isnan(dwb[GUARD + n:]).all()), \
        "wrote outside dw"
    assert bool(torch.isnan(tail).all()), "wrote past jabd_conv_wgrad_part_floats"
    dw = dwb[GUARD:GUARD + n].view(wshape)
    assert bool(torch.isfinite(dw).all()), "non-finite dw"
    # jabd_conv_wgrad_f32's chunk length: M / chunks, rounded up to 64-pixel stages
    per = _cdiv(_cdiv(B * OH * OW, nparts // n), 64) * 64
    return dw, log, per


def run_dgrad(cuda, w, dy, xshape, stride, pad):
    """The data gradient through jabd_conv2d_nhwc_f32 as jabd_amd.train._dgrad
    calls it, with the canaries; returns (dx [B,Cin+8,H,W] on the CPU, log)."""
    from jabd_amd import _lib
    from jabd_amd import functional as F
    from jabd_amd.train import _conv_args
    B, cin, H, W = xshape
    pk = F.pack_weight_device(w.to(cuda), True)
    dyb = _nhwc(dy, 4, 4, cuda)
    dx = torch.full((B, H, W, cin + 8), NAN, device=cuda)
    plain = pk.KH == 1 and pk.KW == 1 and stride == 1 and pad == 0
    a = _conv_args(dyb, pk, dx, stride, pad, tconv=not plain, OH=H, OW=W)
    a.x_c0, a.y_c0 = 4, 4
    _lib.launch_log_reset()
    _lib.call("jabd_conv2d_nhwc_f32", ctypes.byref(a), _stream())
    log = _lib.launch_log()
    torch.cuda.synchronize()
    return dx.permute(0, 3, 1, 2).cpu(), log


def _dx_window(name, out, cin):
    win = out[:, 4:4 + cin]
    assert bool(torch.isfinite(win).all()), f"{name}: non-finite dx inside the window"
    assert bool(torch.isnan(out[:, :4]).all()) and bool(torch.isnan(out[:, 4 + cin:]).all()), \
        f"{name}: wrote outside the channel window [4, {4 + cin})"
    return win


def _run_wcase(cuda, name):
    c, t = G.WCASES[name], G.wtensors(name)
    return run_wgrad(cuda, t["x"], t["dy"], t["gate"], t["wshape"], t["stride"], t["pad"],
                     nchw=c["nchw"], x_c0=c["x_c0"], y_bs_pad=c["y_bs_pad"],
                     gate_pad=c["gate_pad"])


def test_route_tables_cover_the_cases():
    assert set(WROUTES) == set(G.WCASES) and set(DROUTES) == set(G.DCASES)
    tags = {r[0] for r in WROUTES.values()}
    for fam in (W32, W32DB):
        assert {_t(fam, kt, nt) for kt in (64, 128) for nt in (64, 128)} <= tags
    assert {_t(V, kt, nt) for kt in (16, 32, 64) for nt in (16, 32, 64)} <= tags
    assert {_t(SCALAR, 64, 64), ("stem_wgrad", 0), ("stem7_wgrad", 0)} <= tags
    assert {r[1] for r in WROUTES.values()} == {R16, R64}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(WROUTES))
def test_wgrad_route_and_parity(cuda, name):
    dw, log, _ = _run_wcase(cuda, name)
    assert log == WROUTES[name], f"{name}: launched {log}, expected {WROUTES[name]}"
    ref, E = G.wreference(name)
    ok, worst = check(dw, ref, E, "none")
    print(f"{name}: {log} worst |got - ref| / tolerance = {worst:.4f}")
    assert ok, f"{name}: {worst:.3f} x the fp32 bound"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DROUTES))
def test_dgrad_route_and_parity(cuda, name):
    t = G.dtensors(name)
    out, log = run_dgrad(cuda, t["w"], t["dy"], t["xshape"], t["stride"], t["pad"])
    assert log == DROUTES[name], f"{name}: launched {log}, expected {DROUTES[name]}"
    win = _dx_window(name, out, t["xshape"][1])
    ref, E = G.dreference(name)
    ok, worst = check(win, ref, E, "none")
    print(f"{name}: {log} worst |got - ref| / tolerance = {worst:.4f}")
    assert ok, f"{name}: {worst:.3f} x the fp32 bound"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["g32_3x3_64_64", "v_24_16", "s_cin10", "stem_3x3"])
def test_wgrad_deterministic(cuda, name):
    """A multi-chunk case of each family twice: bit-identical (the chunk
    combine is a fixed-order reduction, no atomics)."""
    a, log, _ = _run_wcase(cuda, name)
    b, _, _ = _run_wcase(cuda, name)
    assert log == WROUTES[name]
    assert torch.equal(a, b), f"{name}: two runs differ"


# --------------------------------------------------------------------------- probes
PROBE_B, PROBE_HW = 3, (67, 65)

# family -> (cin, cout, gated, launch of the 3x3 / s1 and the 3x3 / s2 case)
WPROBES = {
    "32": (64, 64, True, _t(W32, 128, 64)),
    "v": (16, 16, False, _t(V, 64, 16)),
    "scalar": (10, 12, False, _t(SCALAR, 64, 64)),
}
_PROBE_X = {}


def _probe_x(cin, gated):
    if (cin, gated) not in _PROBE_X:
        g = torch.Generator().manual_seed(4000 + cin)
        x = torch.randn(PROBE_B, cin, *PROBE_HW, generator=g)
        _PROBE_X[(cin, gated)] = (x, torch.rand(PROBE_B, cin, generator=g) if gated else None)
    return _PROBE_X[(cin, gated)]


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("family", sorted(WPROBES))
def test_wgrad_one_hot_probe(cuda, family, stride):
    """dy = 0 but for a single 1.0: dW[n] is the input patch of that pixel
    (fl(x * gate) when gated, zeros at the padded taps) bit for bit, every
    other dW[n'] exactly zero."""
    cin, cout, is_gated, tag = WPROBES[family]
    x, gate = _probe_x(cin, is_gated)
    H, W = PROBE_HW
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    M, ws = PROBE_B * OH * OW, (cout, cin, 3, 3)
    xs = G.gated(x, gate).double()   # fl(x * gate), held exactly
    per = 64                         # checked against the launch below
    spots = [(0, 0), (M - 1, cout - 1), (7 * per - 1, cout // 2)]   # (pixel, channel)
    for m, n in spots:
        b, r = divmod(m, OH * OW)
        dy = torch.zeros(PROBE_B, cout, OH, OW)
        dy[b, n, r // OW, r % OW] = 1.0
        dw, log, got_per = run_wgrad(cuda, x, dy, gate, ws, stride, 1)
        assert log[0] == tag and got_per == per and M > 8 * per, (log, got_per)
        want = conv2d_weight(xs, ws, dy.double(), stride, 1).float()   # one term: exact
        assert bool((want[n] != 0).any())
        assert torch.equal(dw, want), \
            f"{family} s{stride} pixel {m} channel {n}: {int((dw != want).sum())} of dW differ"


# family -> (cin, cout, stride, launch log)
DPROBES = {
    "m32_s1": (64, 64, 1, [(M32, 102)]),
    "m32_s2": (64, 64, 2, [(M32, 102)] * 4),
    "conv3x3_tile": (40, 40, 1, [("conv3x3_tile", 203)]),
    "conv_gemm": (48, 96, 2, [("conv_gemm", 103)]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(DPROBES))
def test_dgrad_one_hot_probe(cuda, family):
    """A one-hot dy: dx is the scattered weight taps of that pixel, bit for bit."""
    cin, cout, stride, want_log = DPROBES[family]
    H, W = PROBE_HW
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    g = torch.Generator().manual_seed(5000 + cin + stride)
    w = torch.randn(cout, cin, 3, 3, generator=g)
    xshape = (PROBE_B, cin, H, W)
    for b, n, oh, ow in [(0, 0, 0, 0), (PROBE_B - 1, cout - 1, OH - 1, OW - 1),
                         (1, cout // 2, OH // 2, OW // 2 + 1)]:
        dy = torch.zeros(PROBE_B, cout, OH, OW)
        dy[b, n, oh, ow] = 1.0
        out, log = run_dgrad(cuda, w, dy, xshape, stride, 1)
        assert log == want_log, log
        win = _dx_window(family, out, cin)
        want = conv2d_input(xshape, w.double(), dy.double(), stride, 1).float()   # exact
        assert bool((want != 0).any())
        assert torch.equal(win, want), \
            f"{family} dy[{b},{n},{oh},{ow}]: {int((win != want).sum())} of dx differ"
