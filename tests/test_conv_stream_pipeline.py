"""conv1x1_stream after its K loop was pipelined (csrc/conv_stream.hip): the
LDS operands of a stage are read during the stage before, across the block
boundary too, the accumulators of a stage are interleaved, Kc == KC has a
compile-time form (FULL) and the rounded instances test p.Kc on their last
two stages only.  Every case goes through jabd_amd.functional.conv (the
statistics cases through jabd_conv1x1_bn_stats_f32), asserts the launch
witness (kernel name, tag 100 KC + TN) and compares with the float64
reference within the derived fp32 bound of tests/_convref.py.

Canaries as in tests/test_conv_dispatch.py: x has 4 NaN channels on each side
(x_c0 = 4), the output buffer is NaN-filled with 4 extra channels on each
side, the gate rows and the residual rows carry a NaN tail.

What the cases are for:
  instances   TN 1, 2, 3, 5; exact K (Kc 5, 6, 10, 13) and rounded K (Kc 7 ->
              KC 8, 9 -> 10, 14 -> 16, 17 -> 18); 4-wave (Kc TN <= 24) and
              8-wave workgroups
  operands    plain; gate; gate + K-concatenated second source whose boundary
              lies inside a stage (Cin 72) with Cin2 = 24 (not a multiple of
              16); gate + residual; bias with relu / hswish / leaky / none
  edges       M = 5 (one partial block, three waves without a block), two
              blocks with M % 16 != 0, exactly one block per wave, B = 1,
              16-pixel gated maps with B = 3 (every block another image), and
              a map with >= 3 blocks per wave (first, steady-state and last
              iteration; consecutive blocks of a wave lie in different images)
  statistics  TN 1 and 5 with Kc 1 and 4: y, the shift and the partial sums,
              on a grid whose last workgroup has three waves without a block

The statistics bound.  The kernel stores y (fp32), sh = y at pixel 0 and, per
channel, S1 = sum_m fl(y_m - sh) and S2 = sum_m fl(d_m^2) in fp32 in some
order.  With e_m = E_m + 4 u |y_m| the bound on y_m (tests/_convref.py) and
d_m = yref_m - sh (sh: the value the kernel stored, exact in float64), each
term errs by at most delta_m = e_m + u (|d_m| + e_m) and a sum of M terms in
any order by (M + 2) u times the sum of the terms' magnitudes, so

    |S1 - sum d_m|   <= sum delta_m + (M + 2) u sum (|d_m| + delta_m)
    |S2 - sum d_m^2| <= sum (2 |d_m| + delta_m) delta_m
                        + (M + 2) u sum (|d_m| + delta_m)^2.
"""
import ctypes

import pytest
import torch

import _convref as R

STREAM, STREAM_STATS = "conv1x1_stream", "conv1x1_stream_stats"


def _c(cin, cout, B, hw, tag, gate=False, bias=False, res=False, act="none", cin2=0):
    return dict(cin=cin, cout=cout, B=B, hw=hw, tag=tag, gate=gate, bias=bias, res=res, act=act,
                cin2=cin2)


# tag = 100 KC + TN; Kc = ceil((cin + cin2) / 16), TN = ceil(cout / 16)
CASES = {
    # TN 1, Kc 5 exact, 4 waves; plain; M = 70: five blocks, the last partial
    "tn1_k5_plain": _c(80, 16, 2, (5, 7), 501),
    # TN 2, Kc 10 exact (the compile-time form of a KC that also has the rounded
    # one), 4 waves; gate only
    "tn2_k10_gate": _c(160, 24, 3, (4, 8), 1002, gate=True),
    # TN 3, Kc 7 -> KC 8 (rounded, one padded stage), 4 waves; gate + residual
    "tn3_k7_gate_res": _c(112, 40, 2, (4, 8), 803, gate=True, bias=True, res=True, act="hswish"),
    # TN 5, Kc 9 -> KC 10 (rounded), 8 waves; bias + leaky
    "tn5_k9_leaky": _c(144, 80, 2, (5, 7), 1005, bias=True, act="leaky"),
    # TN 5, Kc 17 -> KC 18 (rounded, partial last real stage: K = 268), residual
    "tn5_k17_relu": _c(268, 80, 2, (3, 7), 1805, bias=True, res=True, act="relu"),
    # TN 5, Kc 14 -> KC 16: two padded stages; gated
    "tn5_k14_gate": _c(224, 80, 2, (4, 4), 1605, gate=True, bias=True),
    # gate + second source: boundary inside stage 4 (Cin 72), Cin2 24; 16-pixel
    # maps, B = 3: every block belongs to another image
    "x2_gate_b3": _c(72, 40, 3, (4, 4), 603, gate=True, bias=True, act="relu", cin2=24),
    # the same operands on an 8-wave instance with the rounded form (Kc 17 -> 18)
    "x2_gate_k17": _c(232, 80, 3, (4, 4), 1805, gate=True, bias=True, act="hswish", cin2=40),
    # M = 5: a single partial block; waves 1..3 have no block
    "m5": _c(40, 40, 1, (1, 5), 303, bias=True),
    # two blocks, M = 21
    "m21_res": _c(96, 40, 1, (3, 7), 603, bias=True, res=True, act="relu"),
    # exactly one block per wave (M = 64, 4 waves), B = 1, gate + residual
    "one_block_per_wave": _c(72, 24, 1, (8, 8), 502, gate=True, bias=True, res=True, act="relu"),
    # partial last stage with a gate (K = 200, Kc 13): the gate's padded lanes
    "tn5_k13_gate_res": _c(200, 80, 1, (4, 8), 1305, gate=True, bias=True, res=True,
                           act="hswish"),
}


def _tensors(c, seed):
    g = torch.Generator().manual_seed(seed)
    B, (H, W) = c["B"], c["hw"]
    ktot = c["cin"] + c["cin2"]
    t = dict(x=torch.randn(B, c["cin"], H, W, generator=g),
             w=torch.randn(c["cout"], c["cin"], 1, 1, generator=g) / ktot ** 0.5,
             bias=torch.randn(c["cout"], generator=g) * 0.5 if c["bias"] else None,
             gate=torch.rand(B, c["cin"], generator=g) if c["gate"] else None,
             x2=None, w2=None, res=None, slope=R.SLOPE if c["act"] == "leaky" else 0.0)
    if c["cin2"]:
        t["x2"] = torch.randn(B, c["cin2"], H, W, generator=g)
        t["w2"] = torch.randn(c["cout"], c["cin2"], generator=g) / ktot ** 0.5
    if c["res"]:
        t["res"] = torch.randn(B, c["cout"], H, W, generator=g)
    return t


def _run(cuda, c, t):
    """Launch through F.conv with the canaries; (out [B,Cout+8,H,W] CPU, launch log)."""
    from jabd_amd import _lib
    from jabd_amd import functional as F
    B, cin, cout = c["B"], c["cin"], c["cout"]
    H, W = c["hw"]
    nan = float("nan")
    w2d = F.conv_weight_2d(t["w"])
    if t["w2"] is not None:
        w2d = torch.cat([w2d, t["w2"].t()], 0)
    pk = F.PackedConv(w2d.contiguous().to(cuda), t["bias"].to(cuda) if c["bias"] else None,
                      1, 1, cin, c["cin2"])

    def nhwc(v, lo=0, hi=0):
        b, ch, h, w = v.shape
        buf = torch.full((b, h, w, lo + ch + hi), nan)
        buf[..., lo:lo + ch] = v.permute(0, 2, 3, 1)
        return buf.to(cuda)

    x = nhwc(t["x"], 4, 4)
    out = torch.full((B, H, W, cout + 8), nan, device=cuda)
    gate = None
    if c["gate"]:
        gate = torch.full((B, cin + 4), nan)
        gate[:, :cin] = t["gate"]
        gate = gate.to(cuda)
    x2 = nhwc(t["x2"]) if c["cin2"] else None
    res = nhwc(t["res"], 0, 4) if c["res"] else None
    _lib.launch_log_reset()
    F.conv(x, pk, act=c["act"], slope=t["slope"], ascale=gate, x2=x2, res=res, out=out,
           out_c0=4, x_c0=4)
    log = _lib.launch_log()
    torch.cuda.synchronize()
    return out.permute(0, 3, 1, 2).cpu(), log


def _check(name, c, t, out, log):
    cout = c["cout"]
    assert log == [(STREAM, c["tag"])], f"{name}: launched {log}"
    _, y, E = R.conv_ref64(t["x"], t["w"], t["bias"], 1, 0, t["gate"], t["x2"], t["w2"], 1,
                           t["res"], c["act"], t["slope"])
    win = out[:, 4:4 + cout]
    assert bool(torch.isfinite(win).all()), f"{name}: non-finite output inside the window"
    ok, worst = R.check(win, y, E, c["act"])
    print(f"{name}: {log} worst |got - ref| / tolerance = {worst:.4f}")
    assert ok, f"{name}: {worst:.3f} x the fp32 bound"
    assert bool(torch.isnan(out[:, :4]).all()) and bool(torch.isnan(out[:, 4 + cout:]).all()), \
        f"{name}: wrote outside the channel window [4, {4 + cout})"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_stream_pipeline_parity(cuda, name):
    c = CASES[name]
    t = _tensors(c, 4000 + sorted(CASES).index(name))
    out, log = _run(cuda, c, t)
    _check(name, c, t, out, log)


@pytest.mark.gpu
def test_stream_pipeline_three_blocks_per_wave(cuda):
    """A gated map large enough that every wave walks at least three blocks
    and some walk one more: nblk >= 3 x (CUs x 32, the most waves a CU holds)
    + NW + 1.  A wave's consecutive blocks are CUs x 32 blocks apart, several
    128 x 128 images, so the gate row changes with every block."""
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    need = 3 * cus * 32 + 4 + 1
    per_img = 128 * 128 // 16
    B = (need + per_img - 1) // per_img
    c = _c(16, 16, B, (128, 128), 101, gate=True, bias=True, res=True, act="relu")
    t = _tensors(c, 4100)
    out, log = _run(cuda, c, t)
    _check("three_blocks", c, t, out, log)


# (cin, cout, tag); M = 77: five blocks, a grid of two 4-wave workgroups.  Cin 60: a
# partial fourth stage (and not the Cin 64, Cout >= 64 shape conv1x1_m32s takes)
STATS = {
    "tn1_k1": (16, 16, 101), "tn5_k1": (16, 80, 105),
    "tn1_k4": (64, 16, 401), "tn5_k4": (60, 80, 405),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(STATS))
def test_stream_pipeline_statistics(cuda, name):
    from jabd_amd import _lib
    from jabd_amd import functional as F
    from jabd_amd import train
    cin, cout, tag = STATS[name]
    H, W = 7, 11
    M = H * W
    g = torch.Generator().manual_seed(4200 + sorted(STATS).index(name))
    x = torch.randn(1, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    pk = F.pack_weight_device(w.to(cuda), False)
    xg = x.permute(0, 2, 3, 1).contiguous().to(cuda)
    y = torch.full((1, H, W, cout), float("nan"), device=cuda)
    a = train._conv_args(xg, pk, y, 1, 0)
    nblk = int(_lib.lib().jabd_conv1x1_bn_stats_nblk(ctypes.byref(a)))
    assert nblk == 2, f"{name}: {nblk} partial rows (M = 77 is two 4-wave workgroups)"
    part = torch.full((nblk, 2, cout), float("nan"), device=cuda)
    shift = torch.full((cout,), float("nan"), device=cuda)
    _lib.launch_log_reset()
    _lib.call("jabd_conv1x1_bn_stats_f32", ctypes.byref(a), part.data_ptr(), nblk,
              shift.data_ptr(), train._st())
    log = _lib.launch_log()
    torch.cuda.synchronize()
    assert log == [(STREAM_STATS, tag)], f"{name}: launched {log}"

    _, yref, E = R.conv_ref64(x, w)
    got = y.permute(0, 3, 1, 2).cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: unwritten output"
    ok, worst = R.check(got, yref, E, "none")
    print(f"{name}: y worst / tolerance = {worst:.4f}")
    assert ok, f"{name}: y {worst:.3f} x the fp32 bound"
    sh = shift.cpu()
    assert torch.equal(sh, got[0, :, 0, 0]), f"{name}: shift is not the output at pixel 0"

    d = torch.float64
    yr = yref[0].reshape(cout, M)                       # [C, M]
    e = (E[0] + 4 * R.U * yref[0].abs()).reshape(cout, M)
    dm = yr - sh.to(d)[:, None]
    delta = e + R.U * (dm.abs() + e)
    t1 = delta.sum(1) + (M + 2) * R.U * (dm.abs() + delta).sum(1)
    t2 = ((2 * dm.abs() + delta) * delta).sum(1) + (M + 2) * R.U * ((dm.abs() + delta) ** 2).sum(1)
    p = part.cpu().to(d)
    assert bool(torch.isfinite(p).all()), f"{name}: unwritten partial row"
    s1, s2 = p[:, 0].sum(0), p[:, 1].sum(0)
    r1 = float(((s1 - dm.sum(1)).abs() / t1).max())
    r2 = float(((s2 - (dm ** 2).sum(1)).abs() / t2).max())
    print(f"{name}: S1 worst / tolerance = {r1:.4f}, S2 worst / tolerance = {r2:.4f}")
    assert r1 <= 1.0, f"{name}: sum(y - sh) {r1:.3f} x its bound"
    assert r2 <= 1.0, f"{name}: sum((y - sh)^2) {r2:.3f} x its bound"
