"""Operator-level parity of the inference conv dispatch, one case per kernel
instance, with the launch witness telling which kernel produced the numbers.

jabd_conv2d_nhwc_f32 routes a layer to one of the kernel families
conv1x1_m32 (tile kernel: 1x1, k x k, split-K + m32_ksplit_reduce),
conv1x1_m32s, conv1x1_stream, conv3x3_tile, conv1x1 and conv_gemm, each with
many template instances; the route depends on shape, alignment, gate, second
source, residual, grid size and the thread's split-K setting.  Every case here

 1. asserts the launch log (jabd_launch_log_*: kernel name and instance tag,
    INTEGRATION.md) against the route derived from the dispatch code,
 2. checks the output window against the float64 reference within the
    derived fp32 bound of tests/_convref.py (no measured constant), and
 3. checks that nothing was written outside the output's channel window.

Canaries: x carries 4 NaN channels on each side (x_c0 = 4, row pitch Cin + 8),
the output buffer is NaN-filled with 4 extra channels on each side
(out_c0 = 4), and the gate rows and the residual rows carry a NaN tail, so a
read outside [x_c0, x_c0 + Cin), a gate or residual over-read that reaches an
output, an unwritten output and a write outside [y_c0, y_c0 + Cout) all show.
(The second source and the residual have no channel offset in
jabd_amd.functional.conv; every kernel family here takes the x / y windows.)

The training forms (the weight-gradient kernels of jabd_conv_wgrad_f32 and the
transposed / data-gradient forms of the kernels here) are pinned the same way
in tests/test_conv_backward_dispatch.py.

Not covered: TM = 4 of conv1x1 / conv_gemm needs more than 262144 pixels at
K > 400 (a 400 MB case); the JABD_* A/B environment forms (cached per
process, not product paths); the depthwise gradient kernels
(test_dwconvfn_grads* in tests/test_train_ops.py); conv1x1_m32s and
conv3x3_tile keep their forward parity tests in tests/test_train_ops.py and
tests/test_fused.py, which assert the witness too.
"""
import pytest
import torch

import _convref as R

M32, SPLITK, REDUCE = "conv1x1_m32", "conv1x1_m32 (split K)", "m32_ksplit_reduce"

# case -> (kernel, tag): the route read off csrc/conv.hip (jabd_conv2d_nhwc_f32,
# use_conv32), csrc/conv32.hip (m32_tile, jabd_conv_pack_tn32) and
# csrc/conv_stream.hip (conv1x1_stream_dispatch).  Tags: INTEGRATION.md.
ROUTES = {
    # conv1x1_m32, 1x1 (Cout >= 96, K >= 96): tag 100 TM + TN, TN = tn32 = 32-channel N-tiles
    "a": (M32, 103),             # M = 70: three of four waves partly or wholly empty
    "b_none": (M32, 104),        # kEpiNone; K stage / N tile with 4 live channels
    "b_res": (M32, 104),         # kEpiRes
    "b_bias_leaky": (M32, 104),  # run-time epilogue
    "c": (M32, 101),             # gated, 3 per-image tiles x 1 N group < 256: TN = 1 override
    "d": (M32, 203),             # gated, M >= 65536: TM = 2; 258 tiles >= 256: tn32 kept
    "e160": (M32, 105), "e192": (M32, 106), "e224": (M32, 107),
    "f": (M32, 105),             # gated, 256 tiles: no override
    "g96_s1": (M32, 103), "g96_s2": (M32, 103),
    "g100_s1": (M32, 103), "g100_s2": (M32, 103),   # source boundary inside a stage
    "g100_s1_gated": (M32, 101),  # gate on the first source only (TN = 1 override)
    "h": (M32, 101),             # Cin > kGateLds: gate applied from global memory
    # conv1x1_m32, k x k (Cout >= 64, K >= 288, Cin % 32 == 0)
    "m": (M32, 101),             # gated: TN = 1 override
    "n": (M32, 102),             # K = 288, the threshold; one stage per tap
    # conv1x1 (conv.hip): gated maps with OH * OW % 16 != 0 (conv1x1_stream_dispatch
    # returns -1), TN / KC without a streaming instance, a strided second source
    "o1": ("conv1x1", 101), "o2": ("conv1x1", 102), "o3": ("conv1x1", 105),
    "o4": ("conv1x1", 105),
    "o": ("conv1x1", 104),       # no TN 4 / KC 16 streaming instance
    "p": ("conv1x1", 108),       # jabd_conv_pack_tn(120) = 8
    "q": ("conv1x1", 102),       # x2_stride 2
    "r": ("conv1x1", 201),       # 1024 workgroups at TM 2
    # conv1x1_stream: tag 100 KC + TN (KC = the instance's 16-channel K stages)
    "s": ("conv1x1_stream", 101),
    "t": ("conv1x1_stream", 1305),   # 8-wave workgroups, Kc 13
    "u": ("conv1x1_stream", 1805),   # 8-wave workgroups, Kc 18, K-concat
    "v": ("conv1x1_stream", 303),    # M % 16 != 0
    # conv_gemm
    "w": ("conv_gemm", 101),     # Cin % 4 != 0: scalar loads
    "x": ("conv_gemm", 102),     # Cout < 64 (not conv32), Cin > 64 (not the tile kernel)
    "y": ("conv_gemm", 103),     # stride 2, gate row pitch % 4 != 0
}
# split-K cases: the tile kernel's tag (plain with split-K off, split with it on)
SPLIT = {
    "i": 104,   # 33 stages, ks 8, chunks of 5: chunk 7 is empty
    "j": 102,   # 18 stages, ks 4, chunks of 5: chunk edges inside taps
    "k": 104,   # stride 2
    "l": 101,   # gated, per-image tiles, gate from global memory
}


def _run(cuda, name, img=None, split=False):
    """Launch case `name` with the canaries; returns (out [B,Cout+8,OH,OW] on
    the CPU, launch log, jabd_conv_workspace_size of the launched args)."""
    from jabd_amd import _lib
    from jabd_amd import functional as F
    c, t = R.CASES[name], R.tensors(name, img)
    B, cin, cout, k = t["x"].shape[0], c["cin"], c["cout"], c["k"]
    OH, OW = R.out_hw(c)
    nan = float("nan")
    w2d = F.conv_weight_2d(t["w"])
    if t["w2"] is not None:
        w2d = torch.cat([w2d, t["w2"].t()], 0)
    pk = F.PackedConv(w2d.contiguous().to(cuda), t["bias"].to(cuda) if c["bias"] else None,
                      k, k, cin, c["cin2"])

    def nhwc(v, lo=0, hi=0):   # NCHW CPU -> NHWC GPU with lo / hi NaN channels around it
        b, ch, h, w = v.shape
        buf = torch.full((b, h, w, lo + ch + hi), nan)
        buf[..., lo:lo + ch] = v.permute(0, 2, 3, 1)
        return buf.to(cuda)

    x = nhwc(t["x"], 4, 4)
    out = torch.full((B, OH, OW, cout + 8), nan, device=cuda)
    gate = None
    if c["gate"]:
        gate = torch.full((B, cin + (c["gate_pad"] or 4)), nan)
        gate[:, :cin] = t["gate"]
        gate = gate.to(cuda)
    x2 = nhwc(t["x2"]) if c["cin2"] else None
    res = nhwc(t["res"], 0, 4) if c["res"] else None
    ws = []
    real_call = F.call

    def spy(fn, *args):
        if fn == "jabd_conv2d_nhwc_f32":
            ws.append(int(_lib.lib().jabd_conv_workspace_size(args[0])))
        return real_call(fn, *args)

    F.call = spy
    try:
        _lib.launch_log_reset()
        with F.split_k(split):
            F.conv(x, pk, stride=c["stride"], pad=k // 2, act=c["act"], slope=t["slope"],
                   ascale=gate, x2=x2, x2_stride=c["x2_stride"], res=res, out=out, out_c0=4,
                   x_c0=4)
        log = _lib.launch_log()
    finally:
        F.call = real_call
    torch.cuda.synchronize()
    return out.permute(0, 3, 1, 2).cpu(), log, ws[0]


def _check(name, out, log, want_log, img=None):
    cout = R.CASES[name]["cout"]
    assert log == want_log, f"{name}: launched {log}, expected {want_log}"
    _, y, E = R.reference(name, img)
    win = out[:, 4:4 + cout]
    assert bool(torch.isfinite(win).all()), f"{name}: non-finite output inside the window"
    ok, worst = R.check(win, y, E, R.CASES[name]["act"])
    print(f"{name}: {log} worst |got - ref| / tolerance = {worst:.4f}")
    assert ok, f"{name}: {worst:.3f} x the fp32 bound"
    assert bool(torch.isnan(out[:, :4]).all()) and bool(torch.isnan(out[:, 4 + cout:]).all()), \
        f"{name}: wrote outside the channel window [4, {4 + cout})"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROUTES))
def test_conv_route_and_parity(cuda, name):
    out, log, _ = _run(cuda, name)
    _check(name, out, log, [ROUTES[name]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SPLIT))
def test_conv_split_k(cuda, name):
    """Split-K on: the tile kernel's partial-sum form + m32_ksplit_reduce (bias,
    residual and activation applied there); off: the plain kernel.  The
    workspace query must ask for a workspace exactly when the launch splits."""
    tag = SPLIT[name]
    out, log, ws = _run(cuda, name, split=True)
    assert (ws > 0) == (SPLITK in [n for n, _ in log]), (ws, log)
    _check(name, out, log, [(SPLITK, tag), (REDUCE, 0)])
    out, log, _ = _run(cuda, name, split=False)
    _check(name, out, log, [(M32, tag)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(set(ROUTES) - {"d", "f", "r"}))
def test_conv_workspace_query_matches_launch(cuda, name):
    """Under split_k() every other case either splits and was given a
    workspace, or does neither: jabd_conv_workspace_size > 0 exactly when the
    launch log shows the split (no workspace allocated for a layer another
    kernel serves, no split silently lost)."""
    out, log, ws = _run(cuda, name, split=True)
    names = [n for n, _ in log]
    assert (ws > 0) == (SPLITK in names), (ws, log)
    want = [(SPLITK, ROUTES[name][1]), (REDUCE, 0)] if SPLITK in names else [ROUTES[name]]
    _check(name, out, log, want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c", "a_b3"])
def test_conv_batch_invariance(cuda, name):
    """Split-K off: image 2 of the B = 3 run equals its bs1 run bit for bit
    (per-image tiles under the gate, flat M tiling without it)."""
    tag = ROUTES["c" if name == "c" else "a"]
    out3, log3, _ = _run(cuda, name)
    out1, log1, _ = _run(cuda, name, img=2)
    _check(name, out3, log3, [tag])
    _check(name, out1, log1, [tag], img=2)
    cout = R.CASES[name]["cout"]
    assert torch.equal(out3[2:3, 4:4 + cout], out1[:, 4:4 + cout])
