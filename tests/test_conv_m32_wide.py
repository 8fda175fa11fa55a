"""Parity of the wide-N (tn32 >= 5) 1x1 layers of the 32x32 tile GEMM, whose
TM = 1 launches take the 8-wave workgroup form (conv1x1_m32w8_kernel,
csrc/conv32.hip) when the grid is below two workgroups per CU: waves w and
w + 4 share a 32-pixel row and split the workgroup's TN N-tiles
[(TN + 1) / 2 low, the rest high].

Shapes: the smallest that reach every edge of that form.  B = 2 on a 9 x 15
map is 135 pixels per image: one full 128-pixel tile plus a 7-pixel tile
(three of four row-waves empty, the fourth with 7 live pixels) per image when
gated, 270 = 2 x 128 + 14 pixels tiled flat when not.  Cin = 100: the last K
stage has 4 live channels.  Cout 132 (TN 5, 4 live channels in the last
N-tile, which the high wave half owns), 160 (3 + 2), 192 (3 + 3), 224 (4 + 3).

A gated GEMM keeps its tn32 N-tiles per workgroup only from 256 workgroups up
(m32_tn_launch; below that one N-tile per workgroup, tag 101, the 4-wave
kernel), so the gated variants run twice: at B = 2 on 9 x 15 (tag 101: the
gate / second-source paths of the 4-wave kernel next to the new form) and at
B = 2 on 117 x 139 = 16263 pixels per image = 127 full tiles + 7 pixels, 256
workgroups: the smallest gated grid that keeps TN, i.e. the gated 8-wave form
with the same partial last tile.

Checks per case, as tests/test_conv_dispatch.py: the launch log, the output
window against the float64 reference within tests/_convref.py's derived fp32
bound, nothing written outside the channel window (x, the output, the gate
and the residual carry NaN canaries).  And bit identity against the 4-wave
kernels: the same layer is run again as two launches over weight column
slices of 96..128 channels, [0, 96) and [min(96, Cout - 96), Cout), which
take the 4-wave TN <= 4 instances (a narrower second slice, Cout - 96 < 96
channels, would leave the 32x32 GEMM altogether: use_conv32 needs
Cout >= 96); each slice must equal the one-launch output bit for bit.  An
output element's accumulation order (K stages, 8-channel groups and
components in order) and epilogue do not depend on its N-tile, so a correct
8-wave form gives the same bits.
"""
import pytest
import torch

import _convref as R

M32 = "conv1x1_m32"
CIN, CIN2 = 100, 28
SMALL, LARGE = (9, 15), (117, 139)

# variant -> (gate, bias, res, act, cin2)
VARIANTS = {
    "plain": (False, False, False, "none", 0),
    "gated": (True, True, True, "hswish", 0),
    "gated_x2": (True, True, False, "none", CIN2),
}
TN = {132: 5, 160: 5, 192: 6, 224: 7}

# (variant, cout, map): every variant x Cout on the small map; the gated
# variants again at 256 workgroups, where the gated layer keeps its TN
CASES = [(v, c, SMALL) for v in VARIANTS for c in sorted(TN)]
CASES += [("gated", 132, LARGE), ("gated", 160, LARGE), ("gated", 224, LARGE),
          ("gated_x2", 160, LARGE), ("gated_x2", 192, LARGE)]

_T = {}


def _tensors(variant, cout, hw):
    """fp32 CPU operands (seeded), the float64 reference and its bound; cached,
    never modified."""
    key = (variant, cout, hw)
    if key not in _T:
        gate, bias, res, act, cin2 = VARIANTS[variant]
        g = torch.Generator().manual_seed(9000 + 16 * sorted(VARIANTS).index(variant) + cout + hw[0])
        H, W = hw
        ktot = CIN + cin2
        t = dict(act=act)
        t["x"] = torch.randn(2, CIN, H, W, generator=g)
        t["w"] = torch.randn(cout, CIN, 1, 1, generator=g) / ktot ** 0.5
        t["bias"] = torch.randn(cout, generator=g) * 0.5 if bias else None
        t["gate"] = torch.rand(2, CIN, generator=g) if gate else None
        t["x2"] = torch.randn(2, cin2, H, W, generator=g) if cin2 else None
        t["w2"] = torch.randn(cout, cin2, generator=g) / ktot ** 0.5 if cin2 else None
        t["res"] = torch.randn(2, cout, H, W, generator=g) if res else None
        t["ref"] = R.conv_ref64(t["x"], t["w"], t["bias"], 1, 0, t["gate"], t["x2"], t["w2"], 1,
                                t["res"], act, 0.0)
        _T[key] = t
    return _T[key]


def _launch(cuda, t, lo, hi):
    """The layer's output channels [lo, hi) as one launch with the canaries of
    tests/test_conv_dispatch.py; returns (out [B, hi - lo + 8, H, W] on the
    CPU, launch log)."""
    from jabd_amd import _lib
    from jabd_amd import functional as F
    nan = float("nan")
    cin2 = 0 if t["x2"] is None else t["x2"].shape[1]
    w2d = F.conv_weight_2d(t["w"][lo:hi])
    if cin2:
        w2d = torch.cat([w2d, t["w2"][lo:hi].t()], 0)
    bias = t["bias"][lo:hi].contiguous().to(cuda) if t["bias"] is not None else None
    pk = F.PackedConv(w2d.contiguous().to(cuda), bias, 1, 1, CIN, cin2)

    def nhwc(v, a=0, b=0):   # NCHW CPU -> NHWC GPU with a / b NaN channels around it
        n, ch, h, w = v.shape
        buf = torch.full((n, h, w, a + ch + b), nan)
        buf[..., a:a + ch] = v.permute(0, 2, 3, 1)
        return buf.to(cuda)

    x = nhwc(t["x"], 4, 4)
    B, _, H, W = t["x"].shape
    out = torch.full((B, H, W, hi - lo + 8), nan, device=cuda)
    gate = None
    if t["gate"] is not None:
        gate = torch.full((B, CIN + 4), nan)
        gate[:, :CIN] = t["gate"]
        gate = gate.to(cuda)
    x2 = nhwc(t["x2"]) if cin2 else None
    res = nhwc(t["res"][:, lo:hi], 0, 4) if t["res"] is not None else None
    _lib.launch_log_reset()
    with F.split_k(False):
        F.conv(x, pk, stride=1, pad=0, act=t["act"], slope=0.0, ascale=gate, x2=x2, x2_stride=1,
               res=res, out=out, out_c0=4, x_c0=4)
    log = _lib.launch_log()
    torch.cuda.synchronize()
    return out.permute(0, 3, 1, 2).cpu(), log


def _check_window(what, out, lo, hi, t):
    n = hi - lo
    _, y, E = t["ref"]
    win = out[:, 4:4 + n]
    assert bool(torch.isfinite(win).all()), f"{what}: non-finite output inside the window"
    ok, worst = R.check(win, y[:, lo:hi], E[:, lo:hi], t["act"])
    print(f"{what}: worst |got - ref| / tolerance = {worst:.4f}")
    assert ok, f"{what}: {worst:.3f} x the fp32 bound"
    assert bool(torch.isnan(out[:, :4]).all()) and bool(torch.isnan(out[:, 4 + n:]).all()), \
        f"{what}: wrote outside the channel window [4, {4 + n})"


@pytest.mark.gpu
@pytest.mark.parametrize("variant,cout,hw", CASES,
                         ids=[f"{v}-{c}-{h}x{w}" for v, c, (h, w) in CASES])
def test_wide_n_route_parity_and_bits(cuda, variant, cout, hw):
    t = _tensors(variant, cout, hw)
    gated = VARIANTS[variant][0]
    tiles = 2 * -(-hw[0] * hw[1] // 128)          # per-image 128-pixel tiles of the gated grid
    keeps_tn = not gated or tiles >= 256          # m32_tn_launch
    name = f"{variant} Cout {cout} {hw[0]}x{hw[1]}"
    out, log = _launch(cuda, t, 0, cout)
    # TN = N-tiles per workgroup: the packing's tn32, or 1 under the small-grid override
    assert log == [(M32, 100 + (TN[cout] if keeps_tn else 1))], f"{name}: launched {log}"
    _check_window(name, out, 0, cout, t)
    # the same layer on the 4-wave TN <= 4 instances, in two column slices
    for lo, hi in ((0, 96), (min(96, cout - 96), cout)):
        part, plog = _launch(cuda, t, lo, hi)
        tn = -(-(hi - lo) // 32)
        assert plog == [(M32, 100 + (tn if keeps_tn else 1))], f"{name} [{lo}, {hi}): {plog}"
        _check_window(f"{name} [{lo}, {hi})", part, lo, hi, t)
        assert torch.equal(part[:, 4:4 + hi - lo], out[:, 4 + lo:4 + hi]), \
            f"{name}: channels [{lo}, {hi}) differ from the 4-wave launch's bits"
