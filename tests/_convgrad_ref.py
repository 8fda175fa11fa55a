"""Float64 references of the conv weight gradient and data gradient with
derived error bounds, and the operator-level cases of
tests/test_conv_backward_dispatch.py (shared with the CPU test of the bounds,
tests/test_convgrad_ref.py).

Everything here runs on the CPU; tensors are NCHW as in torch.

Weight gradient.  dW[n][ci][kh][kw] = sum over the M = B * OH * OW output
pixels of fl(x * gate) * dy, in fp32, in some order (pixel chunks, LDS stages,
MFMA steps, the fixed-order chunk combine).  For any order the computed sum of
M products differs from the exact one by at most gamma_M * sum |x gate dy|
(Higham, Accuracy and Stability, (3.5)); the gate multiply and the chunk
combine add one rounding each, so with u = 2^-24

    E = (M + 8) * u * mag,   mag = conv2d_weight(|x * gate|, |dy|)

bounds the error of every correct kernel.  Data gradient: dx is a sum of
Cout * KH * KW products w * dy, so

    E = (Cout * KH * KW + 8) * u * mag,   mag = conv2d_input(|w|, |dy|).

The check is _convref.check: |got - ref| <= E + 4 u |ref|.  No constant is
measured.

Size limit.  A typical product term is about 1 / (M^2 u) times E, so every
bound-checked weight-gradient case keeps M <= 2048: there a dropped or doubled
pixel is at least 4 x the bound.  (The exact-addressing probes of the GPU test
run at M = 13065 without a bound: they compare bit for bit.)
"""
import torch
from torch.nn.grad import conv2d_input, conv2d_weight

from _convref import U

M_MAX = 2048


def gated(x, gate):
    """fl(x * gate[b, c]) in x's dtype, or x."""
    return x if gate is None else x * gate.to(x.dtype)[:, :, None, None]


def wgrad_ref64(x, dy, wshape, stride, pad, gate=None):
    """(dW, E) of conv(x * gate) given dy, float64; x [B,Cin,H,W], dy
    [B,Cout,OH,OW], gate [B,Cin], wshape (Cout,Cin,KH,KW)."""
    d = torch.float64
    xs, g = gated(x.to(d), gate), dy.to(d)
    dw = conv2d_weight(xs, wshape, g, stride, pad)
    mag = conv2d_weight(xs.abs(), wshape, g.abs(), stride, pad)
    M = dy.shape[0] * dy.shape[2] * dy.shape[3]
    return dw, (M + 8) * U * mag


def dgrad_ref64(xshape, w, dy, stride, pad):
    """(dx, E) of conv(x, w) given dy, float64; w [Cout,Cin,KH,KW]."""
    d = torch.float64
    dx = conv2d_input(xshape, w.to(d), dy.to(d), stride, pad)
    mag = conv2d_input(xshape, w.to(d).abs(), dy.to(d).abs(), stride, pad)
    return dx, (w.shape[0] * w.shape[2] * w.shape[3] + 8) * U * mag


def out_hw(c):
    H, W = c["hw"]
    k, s, p = c["k"], c["stride"], c["pad"]
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


# --------------------------------------------------------------------------- the cases
# Forward notation throughout: cin -> cout of the forward conv, hw its input map.
# Layout fields only the GPU test uses: nchw (x is the NCHW network input),
# x_c0 (x's channel offset; 4 NaN channels on each side by default), y_bs_pad
# (floats the dy batch stride exceeds OH * OW * y_ps by), gate_pad (floats the
# gate rows' pitch exceeds Cin by).
def _w(cin, cout, B, hw, k=1, stride=1, pad=None, gate=False, nchw=False, x_c0=4, y_bs_pad=0,
       gate_pad=4):
    return dict(cin=cin, cout=cout, B=B, hw=hw, k=k, stride=stride,
                pad=k // 2 if pad is None else pad, gate=gate, nchw=nchw, x_c0=x_c0,
                y_bs_pad=y_bs_pad, gate_pad=gate_pad)


# M = B * OH * OW; chunks are 64 pixels at these sizes (wgrad_chunks, csrc/train.hip)
WCASES = {
    # conv_wgrad32, fast form (1x1 / s1, double-buffered)
    "f32_64_64": _w(64, 64, 2, (9, 13)),          # M 234: 4 chunks, last 42; image edge in chunk 1
    "f32_64_128": _w(64, 128, 3, (5, 6)),         # M 90: 2 chunks, last 26
    "f32_128_64": _w(128, 64, 2, (5, 6)),         # M 60: a single short chunk
    "f32_120_120": _w(120, 120, 3, (23, 21)),     # M 1449: 23 chunks, last 41; both tiles ragged
    "f32_64_96": _w(64, 96, 2, (9, 13)),          # second N tile half empty
    "f32_120_64_gated": _w(120, 64, 3, (9, 13), gate=True),   # M 351: 6 chunks, last 31
    # conv_wgrad32, general form
    "g32_3x3_8_64": _w(8, 64, 2, (9, 13), k=3),   # K 72: the second K tile holds 8 rows
    "g32_3x3_8_128": _w(8, 128, 3, (5, 6), k=3),
    "g32_3x3_64_64": _w(64, 64, 2, (23, 21), k=3),            # M 966; K * Cout >= 32768
    "g32_3x3s2_64_128_odd": _w(64, 128, 2, (23, 21), k=3, stride=2),   # 12 x 11 out, M 264
    "g32_3x3s2_64_128_even": _w(64, 128, 3, (10, 12), k=3, stride=2),  # 5 x 6 out, M 90
    "g32_1x1s2_64_64": _w(64, 64, 2, (9, 13), stride=2),      # 5 x 7 out, M 70
    "g32_3x3_64_64_gated": _w(64, 64, 3, (9, 13), k=3, gate=True),
    # conv_wgrad_v, the nine (KT, NT) instances, a 3x3 and a gated one
    "v_16_16": _w(16, 16, 2, (9, 13)),
    "v_16_24": _w(16, 24, 3, (5, 6)),
    "v_16_64": _w(16, 64, 2, (5, 6)),
    "v_24_16": _w(24, 16, 3, (23, 21)),
    "v_24_24": _w(24, 24, 2, (9, 13)),
    "v_24_72": _w(24, 72, 3, (9, 13)),
    "v_72_16": _w(72, 16, 2, (23, 21)),
    "v_72_24": _w(72, 24, 3, (5, 6)),
    "v_40_40": _w(40, 40, 2, (9, 13)),
    "v_3x3_8_24": _w(8, 24, 2, (9, 13), k=3),
    "v_24_24_gated": _w(24, 24, 3, (9, 13), gate=True),
    # scalar conv_wgrad_kernel, one case per reason wgrad_vec_ok fails
    "s_cin10": _w(10, 12, 2, (9, 13), k=3),
    "s_cout18": _w(16, 18, 3, (5, 6)),
    "s_xc0_2": _w(16, 16, 2, (9, 13), x_c0=2),
    "s_ybs": _w(16, 16, 3, (9, 13), y_bs_pad=8),
    "s_gate_pitch": _w(16, 16, 2, (9, 13), gate=True, gate_pad=2),
    "s_nchw": _w(3, 32, 2, (23, 21), k=3, stride=2, nchw=True),
    # stem_wgrad
    "stem_3x3": _w(3, 16, 2, (37, 51), k=3, stride=2, nchw=True),      # 19 x 26 out
    # 29 rows, not 33: 33 x 129 at B = 2 is M = 2210 > M_MAX; 15 x 65 out, M 1950,
    # the second 64-pixel segment of each row holds one pixel
    "stem_5x5": _w(1, 16, 2, (29, 129), k=5, stride=2, nchw=True),
    "stem_w64": _w(3, 16, 3, (9, 128), k=3, stride=2, nchw=True),      # 5 x 64 out
    # stem7 form
    "stem7_1x3": _w(3, 64, 2, (1, 3), k=7, stride=2, nchw=True),       # 1 x 2 out
    "stem7_40x44": _w(3, 64, 2, (40, 44), k=7, stride=2, nchw=True),   # 20 x 22 out, M 880
}


def _d(cin, cout, B, hw, k=1, stride=1, pad=None):
    return dict(cin=cin, cout=cout, B=B, hw=hw, k=k, stride=stride,
                pad=k // 2 if pad is None else pad)


DCASES = {
    # tile GEMM (conv1x1_m32) k x k, stride 1
    "m32_3x3_64_64": _d(64, 64, 2, (9, 13), k=3),
    "m32_3x3_128_64": _d(128, 64, 2, (5, 6), k=3),
    # tile GEMM, stride-2 sub-pixel phases
    "ph_64_64_10x11": _d(64, 64, 2, (10, 11), k=3, stride=2),
    "ph_64_64_11x10": _d(64, 64, 2, (11, 10), k=3, stride=2),
    "ph_128_128_10x11": _d(128, 128, 2, (10, 11), k=3, stride=2),
    "ph_128_128_11x10": _d(128, 128, 2, (11, 10), k=3, stride=2),
    "ph_64_64_h1": _d(64, 64, 2, (1, 12), k=3, stride=2),     # the odd-row phases are empty
    "ph_1x1_512_256": _d(512, 256, 2, (8, 9), stride=2),      # only phase (0, 0) has a tap
    # conv3x3_tile, transposed
    "t3_40_40_9x10": _d(40, 40, 2, (9, 10), k=3),
    "t3_40_40_64x17": _d(40, 40, 2, (64, 17), k=3),
    # conv_gemm, transposed
    "gemm_3x3s2_12_10": _d(12, 10, 2, (9, 11), k=3, stride=2),
    # 48 -> 96, not 64 -> 96: with 64 dx channels the 32x32 tile GEMM takes it
    "gemm_3x3s2_48_96": _d(48, 96, 2, (9, 10), k=3, stride=2),
    "gemm_1x1s2_96_64": _d(96, 64, 2, (7, 8), stride=2),
    # plain 1x1 data gradient (tconv = 0 over the transposed pack): dy channels
    # (cout) -> dx channels (cin) is the 1x1 the forward entry sees
    "p_m32_128_96": _d(128, 96, 2, (5, 7)),       # 96 -> 128
    "p_stream_64_16": _d(64, 16, 3, (4, 12)),     # 16 -> 64
    "p_1x1_120_40": _d(120, 40, 2, (5, 7)),       # 40 -> 120
}

_CACHE = {}


def wtensors(name):
    """The fp32 CPU operands of weight-gradient case `name` (seeded), cached
    and never modified: x, dy, gate (or None), wshape, stride, pad."""
    t = _CACHE.get(("w", name))
    if t is None:
        c = WCASES[name]
        g = torch.Generator().manual_seed(2000 + sorted(WCASES).index(name))
        OH, OW = out_hw(c)
        assert c["B"] * OH * OW <= M_MAX, name
        t = dict(stride=c["stride"], pad=c["pad"], wshape=(c["cout"], c["cin"], c["k"], c["k"]))
        t["x"] = torch.randn(c["B"], c["cin"], *c["hw"], generator=g)
        t["dy"] = torch.randn(c["B"], c["cout"], OH, OW, generator=g)
        t["gate"] = torch.rand(c["B"], c["cin"], generator=g) if c["gate"] else None
        _CACHE[("w", name)] = t
    return t


def wreference(name):
    """(dW, E) of weight-gradient case `name`, cached."""
    key = ("wref", name)
    if key not in _CACHE:
        t = wtensors(name)
        _CACHE[key] = wgrad_ref64(t["x"], t["dy"], t["wshape"], t["stride"], t["pad"], t["gate"])
    return _CACHE[key]


def dtensors(name):
    """The fp32 CPU operands of data-gradient case `name` (seeded), cached and
    never modified: w, dy, xshape, stride, pad."""
    t = _CACHE.get(("d", name))
    if t is None:
        c = DCASES[name]
        g = torch.Generator().manual_seed(3000 + sorted(DCASES).index(name))
        OH, OW = out_hw(c)
        k = c["k"]
        t = dict(stride=c["stride"], pad=c["pad"], xshape=(c["B"], c["cin"], *c["hw"]))
        t["w"] = torch.randn(c["cout"], c["cin"], k, k, generator=g) / (c["cin"] * k * k) ** 0.5
        t["dy"] = torch.randn(c["B"], c["cout"], OH, OW, generator=g)
        _CACHE[("d", name)] = t
    return t


def dreference(name):
    """(dx, E) of data-gradient case `name`, cached."""
    key = ("dref", name)
    if key not in _CACHE:
        t = dtensors(name)
        _CACHE[key] = dgrad_ref64(t["xshape"], t["w"], t["dy"], t["stride"], t["pad"])
    return _CACHE[key]
