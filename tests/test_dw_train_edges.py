"""Exact-data edge tests of the depthwise training kernels: csrc/dwconv.hip
(dw_kernel, dw_rows_kernel) and the depthwise gradients of csrc/train.hip
(dw_dgrad_strip_kernel, dw_dgrad_bn_kernel, dw_dgrad_bn_rows_kernel,
dw_wgrad_strip_kernel, dw_wgrad_rows_kernel).  Inputs, fp64 references, case
tables, host-plan restatements and planted defects: tests/_dw_bn_exact.py.

Every operand is a small nonzero integer (the BN-input taps relu(bn(x)) are
multiples of 0.5), so every partial sum is exact in fp32 and the device result
must EQUAL the fp64 reference: y, shift, the summed statistics partials, dx,
de, dW, dbeta and dgamma are compared with array_equal.  Only mean / invstd
(<= 1 ulp of the fp64 value rounded to fp32), the running buffers (<= 2 ulp)
and the BatchNorm dx of the fused data gradient (the derived elementwise bound
of _dw_bn_exact.bn_dx_ref) carry a bar.  Each case asserts its route from the
launch log against the restated host plan; every output is prefilled with NaN
and must come back finite, and carries a 64-float sentinel tail that must come
back bit-identical.  The cases go through the C ABI, which is where the forms
(bias / activation in the statistics forward, dz NULL or not at either stride,
channel-slice views) can be chosen freely; the channel sweep at C = 12 / 260
runs again through jabd_amd.train's wrappers and F.dwconv, routes asserted.

Non-gpu self-checks: the 2^24 condition and order independence (numpy fp32,
row-major and a seeded permutation, bit-equal to fp64) for every case; the
references against torch's fp64 conv2d and its autograd; each planted defect
breaks equality on its named cases; the plan restatements equal the exported
counts; the C ABI's rejections.

Forms witnessed on the MI355X, per group:
  channel sweep (C 4..960, 1024 forward only; k 3/5, stride 1/2)
      dwconv_stats_rows (3x3), dwconv_stats (5x5), dw_dgrad, dw_dgrad_bn +
      bn_bwd_apply (dz stored) and + dw_dgrad_bn_apply (dz NULL) at both
      strides, dw_wgrad_rows (3x3), dw_wgrad (5x5), plain and BN-input
  spatial sweep (20 maps of {1,2,3,7,8,9,17}^2 x C 12/256): the same forms
  row-chunk seams   dw_wgrad_rows R = 1..5 (two chunks, last one short for odd
      OH), dwconv_stats_rows R = 1..5, both strides
  fallbacks         dw_wgrad at B = 1025 (B * nbands > 1024); dwconv_stats at
      C = 960 3x3/s2 OW = 8 (nbands 4 > nblk 2) and at stride 1 for C = 516,
      B = 1025, 1x8 (nbands 2 > nblk 1)
  block plans       dw_dgrad_bn spb = 2 (9225 groups, last block short);
      dw_wgrad 5x5 with 12 / 8 items per block over rows_pass = 4
  inference entry   dwconv on channel slices (pixel strides C + 8)
  switched forms (one child process each): JABD_DW_ROWS=0 -> dwconv_stats,
      JABD_DW_WGRAD_ROWS=0 -> dw_wgrad, JABD_DW_DGRAD_ROWS=1 -> dw_dgrad_bn_rows
      (+ dw_dgrad_bn_rows_apply), R = 1..5 at both strides
  training wrappers (_dw_fwd_bn_stats, _dw_bwd, _dw_bn_bwd) and F.dwconv with
      partials: the routes of the C-ABI cases, asserted from the launch log
Worst distance observed on the MI355X next to its bar:
  mean 0 ulp / 1    invstd 0 ulp / 1    running_mean 1 ulp / 2    running_var 2 ulp / 2
  BatchNorm dx of the fused data gradient 0.34 of the derived bound / 1 (strip forms),
  0.29 (JABD_DW_DGRAD_ROWS=1)
No case was taken out.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _dw_bn_exact as E
import _dw_bn_device as D
from _dw_bn_device import Out, L as _L, eq as _eq, logged as _logged, scratch as _scratch, up as _up

EPS = 1e-5
FIG = D.Figures()     # worst observed distances of this module's device runs
_note, _report = FIG.note, FIG.report


def _ulp(*a):
    D.ulp(FIG, *a)


# ------------------------------------------------------------------ CPU self-checks
GROUPS = sorted({c.group for c in E.ALL_DW_CASES + E.INFER_CASES})


def _cases(group):
    return [c for c in E.ALL_DW_CASES + E.INFER_CASES if c.group == group]


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a) and a.keys() == b.keys()


@pytest.mark.parametrize("group", GROUPS)
def test_exactness_condition_and_order_independence(group):
    """Every case keeps the 2^24 condition with 2x room, and an fp32 evaluation
    in two different orders reproduces the fp64 reference bit for bit."""
    for c in _cases(group):
        d = E.dw_data(c)
        want = E.case_groups(c)
        E.dw_conditions(c, d)
        ref = E.dw_eval(c, d, want=want)
        for sm in (E.Summer(f32=True), E.Summer(f32=True, seed=11)):
            assert _same(ref, E.dw_eval(c, d, sm, want=want)), E.dw_id(c)


def test_references_match_torch_fp64():
    """The numpy references are torch's fp64 conv2d and its autograd."""
    import torch.nn.functional as tF
    picks = [c for c in E.CHAN_CASES if c.C in (12, 260)] + \
        [c for c in E.SPATIAL_CASES if c.C == 12 and (c.H, c.W) in ((1, 1), (2, 2), (1, 17), (8, 9), (17, 3))]
    for c in picks:
        d, r = E.dw_data(c), E.dw_eval(c, E.dw_data(c))
        x = torch.from_numpy(d["x"]).permute(0, 3, 1, 2).clone().requires_grad_()
        w = torch.from_numpy(d["w"].T.reshape(c.C, 1, c.k, c.k).copy()).requires_grad_()
        y = tF.conv2d(x, w, torch.from_numpy(d["bias"]), c.s, c.k // 2, groups=c.C)
        act = E.case_act(c)
        y = torch.relu(y) if act == "relu" else tF.leaky_relu(y, 0.5) if act == "leaky" else y
        assert np.array_equal(y.detach().permute(0, 2, 3, 1).numpy(), r["y"]), E.dw_id(c)
        y2 = tF.conv2d(x, w, None, c.s, c.k // 2, groups=c.C)
        (y2 * torch.from_numpy(d["dy"]).permute(0, 3, 1, 2)).sum().backward()
        assert np.array_equal(x.grad.permute(0, 2, 3, 1).numpy(), r["dx"]), E.dw_id(c)
        assert np.array_equal(w.grad.reshape(c.C, -1).numpy(), r["dw"]), E.dw_id(c)


def _broken(c, defect, geom=None, want=None):
    """Names of the outputs on which the fp32 evaluation with `defect` differs."""
    d = E.dw_data(c)
    want = want or E.case_groups(c)
    ref = E.dw_eval(c, d, want=want)
    bad = E.dw_eval(c, d, E.Summer(f32=True), defect=defect, geom=geom, want=want)
    return {k for k in ref if not np.array_equal(ref[k], bad[k])}


def test_planted_defects_are_caught():
    """Each defect of the numpy evaluation breaks equality on its named cases."""
    sp = {(c.H, c.W, c.C, c.k, c.s): c for c in E.SPATIAL_CASES}
    # (a) the last column of every strip dropped: maps at least one strip wide
    for key in ((8, 9, 12, 3, 1), (8, 17, 256, 3, 1), (9, 9, 12, 5, 1), (8, 17, 12, 3, 2)):
        c = sp[key]
        for PW, names in ((E.wgrad_route(*c[1:]).PW, {"dw", "dwb"}),
                          (E.dw_fwd_route(*c[1:]).PW, {"S", "Q", "Sb", "Qb"}), (8, {"dx"})):
            if PW <= (c.W if "dx" in names else E.out_size(c.W, c.k, c.s)):
                assert names <= _broken(c, "drop_col", dict(PW=PW)), (E.dw_id(c), PW, names)
    # (b) the first row of the second row chunk dropped: the row-chunk cases
    for c in E.WG_ROWS_CASES:
        assert {"dw", "dwb"} <= _broken(c, "drop_row", dict(R=E.wgrad_route(*c[1:]).R)), E.dw_id(c)
    for c in E.FWD_ROWS_CASES:
        assert {"S", "Q", "Sb", "Qb"} <= _broken(c, "drop_row", dict(R=E.dw_fwd_route(*c[1:]).R)), \
            E.dw_id(c)
    # (c) the last row of a block counted twice: the block-plan cases
    for c in E.DGBN_SPB_CASES:
        nblk, spb, _ = E.dgbn_plan(c.B, c.H, c.W, c.C)
        assert {"dbeta", "dgamma"} <= _broken(c, "dup_row", dict(per=spb * c.W)), E.dw_id(c)
    for c in E.WG_PER_CASES + E.WG_FALLBACK_CASES:
        per = E.wgrad_route(*c[1:]).R
        assert "dw" in _broken(c, "dup_row", dict(per=per)), E.dw_id(c)
    # (d) one tap shifted by a pixel, (e) the live lane of the second channel
    # block skipped, (f) the stride-2 row parity inverted: the channel sweep
    every = {"y", "S", "Q", "yb", "Sb", "Qb", "dw", "dwb"}
    for c in E.CHAN_CASES:
        assert every <= _broken(c, "shift_tap"), E.dw_id(c)
        if c.C == 260:
            got = _broken(c, "skip_lane")
            assert every | {"dx", "dz", "dbeta", "dgamma", "shift", "shiftb"} <= got, E.dw_id(c)
        else:
            assert not _broken(c, "skip_lane"), E.dw_id(c)
        if c.s == 2:
            assert {"dx", "dz", "dbeta", "dgamma"} <= _broken(c, "flip_parity"), E.dw_id(c)
    assert not _broken(E.CHAN_CASES[0], None)      # the honest evaluation trips nothing


def test_route_predictions_name_the_planned_forms():
    """What the case tables are for, by the restated plans: the forms, the
    chunk seams and the block plans the issue names."""
    for c in E.CHAN_CASES + E.SPATIAL_CASES:
        # 3x3/s2 on a 1- or 2-row, 17-wide map at C = 256: 5 strips of 2 make
        # 2 bands for the forward's single block, so dw_kernel serves them
        low = (c.C, c.k, c.s, c.W) == (256, 3, 2, 17) and c.H <= 2
        assert E.dw_fwd_route(*c[1:]).name == ("dwconv_stats_rows" if c.k == 3 and not low
                                               else "dwconv_stats"), E.dw_id(c)
        assert E.wgrad_route(*c[1:]).name == ("dw_wgrad_rows" if c.k == 3 else "dw_wgrad")
        assert E.dgbn_route(*c[1:], True)[0][0] == "dw_dgrad_bn"
    for s in (1, 2):
        for cases, route, name in ((E.WG_ROWS_CASES, E.wgrad_route, "dw_wgrad_rows"),
                                   (E.FWD_ROWS_CASES, E.dw_fwd_route, "dwconv_stats_rows")):
            rs = [route(*c[1:]) for c in cases if c.s == s]
            assert all(r.name == name and r.nch >= 2 for r in rs)
            assert {r.R for r in rs} == {1, 2, 3, 4, 5}, (name, s)
        short = [c for c in E.WG_ROWS_CASES if c.s == s
                 and E.out_size(c.H, 3, s) % E.wgrad_route(*c[1:]).R]
        assert len(short) >= 3                      # a short last chunk
    for c in E.WG_ROWS_CASES:
        assert c.B * E.wgrad_route(*c[1:]).nbands == 512      # want = 2
    rs = [E.dgbn_route(*c[1:], True, rows_on=True)[1] for c in E.DG_ROWS_CASES]
    assert all(r.name == "dw_dgrad_bn_rows" and r.nch >= 2 for r in rs)
    assert {(c.s, r.R) for c, r in zip(E.DG_ROWS_CASES, rs)} == {(s, R) for s in (1, 2)
                                                                for R in (1, 2, 3, 4, 5)}
    for c in E.WG_FALLBACK_CASES:
        assert E.wgrad_route(*c[1:]).name == "dw_wgrad"
    for c in E.FWD_FALLBACK_CASES:
        assert E.dw_fwd_route(*c[1:]).name == "dwconv_stats"
        assert c.B * c.H * c.W * c.C * 4 < 64 << 20
    c = E.FWD_FALLBACK_CASES[0]                     # the issue's hand computation
    assert E.dw_nblk(c.B, 1, 8, 960) == 2 and E.cdiv(E.cdiv(8, 2), E.dw_sp(960)) == 4
    for c in E.DGBN_SPB_CASES:
        nblk, spb, groups = E.dgbn_plan(c.B, c.H, c.W, c.C)
        assert (groups, spb, nblk) == (9225, 2, 4613) and groups % spb == 1
    for c in E.WG_PER_CASES:
        assert E.wgrad_route(*c[1:]).R > E.ew_rows_pass(c.C)   # per > rows_pass
    # channel widths whose lanes do not divide 256, and the second channel block
    assert (E.bn_lanes(12), E.bn_rows_pass(12)) == (3, 85)
    assert E.bn_lanes(72) * E.bn_rows_pass(72) == 252
    assert E.cdiv(260 // 4, E.ew_lanes(260)) == 2 and 260 // 4 - 64 == 1


def test_restated_plans_equal_the_exported_counts():
    h = _L().lib()
    for c in E.ALL_DW_CASES + E.INFER_CASES:
        OH, OW = E.out_size(c.H, c.k, c.s), E.out_size(c.W, c.k, c.s)
        nb = E.dw_nblk(c.B, OH, OW, c.C)
        assert h.jabd_dw_nblk(c.B, OH, OW, c.C) == nb, E.dw_id(c)
        assert h.jabd_dwconv_stats_nblk(c.B, OH, OW, c.C) == nb * c.B, E.dw_id(c)
        assert h.jabd_dw_dgrad_bn_part_floats(c.B, c.H, c.W, c.C) == \
            E.dgbn_plan(c.B, c.H, c.W, c.C)[0] * 2 * c.C, E.dw_id(c)
        for rows_on in (True, False):               # both forms fit the 1024 partial blocks
            assert E.wgrad_route(*c[1:], rows_on=rows_on).nblk <= 1024
        assert h.jabd_dw_wgrad_part_floats(c.B * OH * OW, c.C, c.k) == 1024 * c.k * c.k * c.C
    assert h.jabd_dw_nblk(2, 5, 9, 1028) == -1 and h.jabd_dw_nblk(2, 5, 9, 10) == -1


def _dw_args(x, w, y, B, H, W, C, k, s, pad=None, OH=None, OW=None, bias=None, act="none"):
    a = _L().DwArgs()
    pad = k // 2 if pad is None else pad
    a.x, a.x_bs, a.x_ps = x, H * W * C, C
    a.B, a.H, a.W, a.C = B, H, W, C
    a.w, a.bias = w, bias
    OH = (H + 2 * pad - k) // s + 1 if OH is None else OH
    OW = (W + 2 * pad - k) // s + 1 if OW is None else OW
    a.y, a.y_bs, a.y_ps = y, OH * OW * C, C
    a.OH, a.OW, a.k, a.stride, a.pad, a.act = OH, OW, k, s, pad, E.ACT[act]
    a.slope = E.SLOPE
    return a


def test_argument_rejection_through_the_c_abi():
    """Bad depthwise arguments return JABD_EINVAL and launch nothing."""
    L = _L()
    h = L.lib()
    buf = _scratch(1 << 18)
    p = buf.data_ptr()
    EINVAL = 1

    def fwd(**kw):
        g = dict(B=1, H=4, W=4, C=8, k=3, s=1)
        g.update(kw)
        a = _dw_args(p, p, p, **g)
        return [h.jabd_dwconv_nhwc_f32(ctypes.byref(a), None),
                h.jabd_dwconv_stats_f32(ctypes.byref(a), p, p, None),
                h.jabd_dwconv_bnin_stats_f32(ctypes.byref(a), p, p, p, p, 1, 0.0, p, p, None)]

    def grads(B=1, H=4, W=4, C=8, k=3, s=1, pad=None, OH=None, OW=None):
        pad = k // 2 if pad is None else pad
        OH = E.out_size(H, k, s) if OH is None else OH
        OW = E.out_size(W, k, s) if OW is None else OW
        return [h.jabd_dw_dgrad_f32(p, p, B, H, W, C, OH, OW, k, s, pad, p, None),
                h.jabd_dw_dgrad_bn_bwd_f32(p, p, B, H, W, C, OH, OW, k, s, pad, p, p, p, p, p, 1,
                                           0.0, p, p, p, p, p, None),
                h.jabd_dw_wgrad_f32(p, p, B, H, W, C, OH, OW, k, s, pad, p, p, None),
                h.jabd_dw_wgrad_bnin_f32(p, p, B, H, W, C, OH, OW, k, s, pad, p, p, p, p, 1, 0.0,
                                         p, p, None)]

    L.launch_log_reset()
    assert fwd(C=1028) == [EINVAL] * 3              # past the whole-C workgroup
    assert fwd(C=10) == [EINVAL] * 3                # C % 4
    assert fwd(OH=5) == [EINVAL] * 3 and fwd(OW=3) == [EINVAL] * 3
    assert fwd(s=2, OH=4) == [EINVAL] * 3
    assert fwd(k=7) == [EINVAL] * 3
    assert grads(C=10) == [EINVAL] * 4
    assert grads(OH=5) == [EINVAL] * 4 and grads(OW=3) == [EINVAL] * 4
    assert grads(k=7) == [EINVAL] * 4
    assert grads(pad=0, OH=2, OW=2) == [EINVAL] * 4  # pad != k / 2, sizes consistent with it
    assert grads(k=5, pad=1) == [EINVAL] * 4
    assert grads(s=3, OH=2, OW=2) == [EINVAL] * 4
    assert L.launch_log() == []
    assert "dw" in L.last_error()


# ------------------------------------------------------------------ device harness
def _bn_dev(dev, bn):
    return [_up(dev, v) for v in (bn.mean, bn.invstd, bn.gamma, bn.beta)]


def run_forward(dev, c, d, ref, bnin, rows_on=True):
    """The statistics forward (plain with bias + activation, or the BN-input
    form with relu) and bn_stats_final on its partials."""
    L, cid = _L(), E.dw_id(c) + (" bnin" if bnin else "")
    tag = "b" if bnin else ""
    OH, OW = E.out_size(c.H, c.k, c.s), E.out_size(c.W, c.k, c.s)
    M = c.B * OH * OW
    x, w = _up(dev, d["x"]), _up(dev, d["w"])
    bias = None if bnin else _up(dev, d["bias"])
    y = Out(dev, c.B, OH, OW, c.C)
    a = _dw_args(x.data_ptr(), w.data_ptr(), y.ptr, c.B, c.H, c.W, c.C, c.k, c.s,
                 bias=None if bnin else bias.data_ptr(), act="none" if bnin else E.case_act(c))
    nblk = int(L.lib().jabd_dwconv_stats_nblk(c.B, OH, OW, c.C))
    part, shift = Out(dev, nblk, 2, c.C), Out(dev, c.C)
    if bnin:
        m, i, g, b = _bn_dev(dev, d["bn"])
        log = _logged("jabd_dwconv_bnin_stats_f32", ctypes.byref(a), m.data_ptr(), i.data_ptr(),
                      g.data_ptr(), b.data_ptr(), E.ACT["relu"], 0.0, part.ptr, shift.ptr, None)
    else:
        log = _logged("jabd_dwconv_stats_f32", ctypes.byref(a), part.ptr, shift.ptr, None)
    assert log == [E.dw_fwd_route(*c[1:], rows_on=rows_on).name], (cid, log)
    _eq("y", cid, y.get("y"), ref["y" + tag])
    _eq("shift", cid, shift.get("shift"), ref["shift" + tag])
    pt = part.get("stats partials")
    _eq("sum of partials (S)", cid, pt[:, 0].sum(0), ref["S" + tag])
    _eq("sum of partials (Q)", cid, pt[:, 1].sum(0), ref["Q" + tag])
    mean64, invstd64, unb64 = E.bn_stats_ref(ref["shift" + tag], ref["S" + tag], ref["Q" + tag], M, EPS)
    mom = 1.0 if (c.H + c.W + c.C // 4) % 2 else 0.1
    rm0, rv0 = E.running_start(mean64), np.ones(c.C)
    mean, invstd = Out(dev, c.C), Out(dev, c.C)
    rm, rv = Out(dev, c.C, init=rm0), Out(dev, c.C, init=rv0)
    log = _logged("jabd_bn_stats_final_f32", shift.ptr, part.ptr, nblk, M, c.C, mean.ptr, invstd.ptr,
                  rm.ptr, rv.ptr, mom, EPS, None)
    assert log == ["bn_stats_final"], (cid, log)
    _ulp("mean", cid, mean.get("mean"), mean64, 1)
    _ulp("invstd", cid, invstd.get("invstd"), invstd64, 1)
    _ulp("running_mean", cid, rm.get("running_mean"), E.running_ref(rm0, mean64, mom), 2)
    _ulp("running_var", cid, rv.get("running_var"), E.running_ref(rv0, unb64, mom), 2)


def run_dgrad(dev, c, d, ref):
    cid = E.dw_id(c)
    OH, OW = E.out_size(c.H, c.k, c.s), E.out_size(c.W, c.k, c.s)
    dy, w = _up(dev, d["dy"]), _up(dev, d["w"])
    dx = Out(dev, c.B, c.H, c.W, c.C)
    log = _logged("jabd_dw_dgrad_f32", dy.data_ptr(), w.data_ptr(), c.B, c.H, c.W, c.C, OH, OW, c.k,
                  c.s, c.k // 2, dx.ptr, None)
    assert log == ["dw_dgrad"], (cid, log)
    _eq("dx", cid, dx.get("dx"), ref["dx"])


def run_dgrad_bn(dev, c, d, ref, store_dz, rows_on=False):
    """The data gradient with the BatchNorm backward fused in: de stored to dz
    and applied (MODE 0), or dz NULL and de recomputed by the apply (MODE 1 + 2)."""
    L, cid = _L(), E.dw_id(c) + (" dz" if store_dz else " dz=NULL")
    OH, OW = E.out_size(c.H, c.k, c.s), E.out_size(c.W, c.k, c.s)
    M = c.B * c.H * c.W
    dy, w, x = _up(dev, d["dy"]), _up(dev, d["w"]), _up(dev, d["x"])
    m, i, g, b = _bn_dev(dev, d["bn"])
    nfl = int(L.lib().jabd_dw_dgrad_bn_part_floats(c.B, c.H, c.W, c.C))
    part = Out(dev, nfl)
    dgamma, dbeta = Out(dev, c.C), Out(dev, c.C)
    dz = Out(dev, c.B, c.H, c.W, c.C) if store_dz else None
    dx = Out(dev, c.B, c.H, c.W, c.C)
    act = E.case_act(c)
    log = _logged("jabd_dw_dgrad_bn_bwd_f32", dy.data_ptr(), w.data_ptr(), c.B, c.H, c.W, c.C, OH,
                  OW, c.k, c.s, c.k // 2, x.data_ptr(), m.data_ptr(), i.data_ptr(), g.data_ptr(),
                  b.data_ptr(), E.ACT[act], E.SLOPE, part.ptr, dgamma.ptr, dbeta.ptr,
                  dz.ptr if store_dz else None, dx.ptr, None)
    assert log == E.dgbn_route(*c[1:], store_dz, rows_on=rows_on)[0], (cid, log)
    part.get("dgrad_bn partials")
    if store_dz:
        _eq("de", cid, dz.get("de"), ref["dx"])
    _eq("dbeta", cid, dbeta.get("dbeta"), ref["dbeta"])
    _eq("dgamma", cid, dgamma.get("dgamma"), ref["dgamma"])
    dxr, bound = E.bn_dx_ref(ref["dz"], E.bn_xhat(d["x"], d["bn"]), d["bn"], ref["dbeta"],
                             ref["dgamma"], M)
    err = np.abs(dx.get("dx") - dxr)
    _note("dgrad_bn dx / bound", np.max(err / np.maximum(bound, 1e-300)))
    assert np.all(err <= bound), f"{cid} dx: {np.max(err / np.maximum(bound, 1e-300)):.3g} of the bound"


def run_wgrad(dev, c, d, ref, bnin, rows_on=True):
    L, cid = _L(), E.dw_id(c) + (" bnin" if bnin else "")
    OH, OW = E.out_size(c.H, c.k, c.s), E.out_size(c.W, c.k, c.s)
    x, dy = _up(dev, d["x"]), _up(dev, d["dy"])
    part = Out(dev, int(L.lib().jabd_dw_wgrad_part_floats(c.B * OH * OW, c.C, c.k)))
    dw = Out(dev, c.C, c.k * c.k)
    geo = (c.B, c.H, c.W, c.C, OH, OW, c.k, c.s, c.k // 2)
    if bnin:
        m, i, g, b = _bn_dev(dev, d["bn"])
        log = _logged("jabd_dw_wgrad_bnin_f32", x.data_ptr(), dy.data_ptr(), *geo, m.data_ptr(),
                      i.data_ptr(), g.data_ptr(), b.data_ptr(), E.ACT["relu"], 0.0, part.ptr, dw.ptr,
                      None)
    else:
        log = _logged("jabd_dw_wgrad_f32", x.data_ptr(), dy.data_ptr(), *geo, part.ptr, dw.ptr, None)
    assert log == [E.wgrad_route(*c[1:], rows_on=rows_on).name, "dw_wgrad_reduce"], (cid, log)
    part.get("wgrad partials", finite=None)         # 1024 blocks reserved, nblk of them written
    _eq("dW", cid, dw.get("dW"), ref["dwb" if bnin else "dw"])


def run_case(dev, c, want=None, fwd_rows=True, wg_rows=True, dg_rows=False):
    d = E.dw_data(c)
    want = want or E.case_groups(c)
    E.dw_conditions(c, d, want)                     # before any device work
    ref = E.dw_eval(c, d, want=want)
    if "fwd" in want:
        run_forward(dev, c, d, ref, False, fwd_rows)
    if "fwdbn" in want:
        run_forward(dev, c, d, ref, True, fwd_rows)
    if "dgrad" in want:
        run_dgrad(dev, c, d, ref)
    if "dgbn" in want:
        run_dgrad_bn(dev, c, d, ref, True, dg_rows)
        run_dgrad_bn(dev, c, d, ref, False, dg_rows)
    if "wgrad" in want:
        run_wgrad(dev, c, d, ref, False, wg_rows)
    if "wgradbn" in want:
        run_wgrad(dev, c, d, ref, True, wg_rows)


# ------------------------------------------------------------------ GPU cases
@pytest.mark.gpu
@pytest.mark.parametrize("k,s", E.KS)
def test_channel_sweep(cuda, k, s):
    """C in {4, 12, 72, 256, 260, 960} (and 1024, forward only) at 2x5x9: lanes
    that do not divide 256, the second channel block's single live lane, the
    forward's whole-C workgroup at its limit."""
    for c in E.CHAN_CASES + E.CHAN_FWD_ONLY:
        if (c.k, c.s) == (k, s):
            run_case(cuda, c)
    _report()


@pytest.mark.gpu
@pytest.mark.parametrize("C", (12, 256))
@pytest.mark.parametrize("k,s", E.KS)
def test_spatial_sweep(cuda, k, s, C):
    """Maps narrower than a strip and shorter than the kernel, the strip widths
    2 / 4 / 8, stride 2 on odd and even sizes."""
    for c in E.SPATIAL_CASES:
        if (c.k, c.s, c.C) == (k, s, C):
            run_case(cuda, c)
    _report()


@pytest.mark.gpu
@pytest.mark.parametrize("s", (1, 2))
def test_row_chunk_seams(cuda, s):
    """Every exit of the unrolled row loops of dw_wgrad_rows_kernel and
    dw_rows_kernel: R = 1..5 over two chunks, the last one short."""
    for c in E.WG_ROWS_CASES + E.FWD_ROWS_CASES + E.DG_ROWS_CASES:
        if c.s == s:
            run_case(cuda, c)
    _report()


@pytest.mark.gpu
def test_form_fallbacks_and_block_plans(cuda):
    """The strip weight gradient past 1024 (image, band) pairs, dw_kernel where
    the bands outnumber the forward's blocks, dgbn_plan's spb = 2 and the strip
    weight gradient's per > rows_pass."""
    for c in E.WG_FALLBACK_CASES + E.FWD_FALLBACK_CASES + E.DGBN_SPB_CASES + E.WG_PER_CASES:
        run_case(cuda, c)
    _report()


@pytest.mark.gpu
def test_inference_entry_on_channel_slices(cuda):
    """jabd_dwconv_nhwc_f32 with integer bias, relu and ECA partials; x and y
    are channel slices (pixel strides C + 8): y exact, the untouched columns
    untouched, and the partials sum to sum(y) exactly."""
    L = _L()
    for c in E.INFER_CASES:
        cid = E.dw_id(c)
        d = E.dw_data(c)
        E.dw_conditions(c, d, ("fwd",))
        tp = E.Taps(d["x"], c.k, c.s)
        yref = E.act_f(E.REF.taps(c.k * c.k + 1, lambda i: tp.view(i) * d["w"][i] if i < c.k * c.k
                                  else np.broadcast_to(d["bias"], tp.view(0).shape)), "relu")
        E.assert_exact("sum y", np.abs(yref).reshape(c.B, -1, c.C).sum(1))
        OH, OW, Cw = tp.OH, tp.OW, c.C + 8
        xw = np.full((c.B, c.H, c.W, Cw), 7.0)
        xw[..., 4:4 + c.C] = d["x"]
        x, w, bias = _up(cuda, xw), _up(cuda, d["w"]), _up(cuda, d["bias"])
        y = Out(cuda, c.B, OH, OW, Cw)
        nblk = int(L.lib().jabd_dw_nblk(c.B, OH, OW, c.C))
        part = Out(cuda, c.B, nblk, c.C)
        a = _dw_args(x.data_ptr() + 16, w.data_ptr(), y.ptr + 16, c.B, c.H, c.W, c.C, c.k, c.s,
                     bias=bias.data_ptr(), act="relu")
        a.x_ps, a.x_bs = Cw, c.H * c.W * Cw
        a.y_ps, a.y_bs = Cw, OH * OW * Cw
        a.nblk, a.part = nblk, part.ptr
        assert _logged("jabd_dwconv_nhwc_f32", ctypes.byref(a), None) == ["dwconv"], cid
        yg = y.get("y", finite=False)
        _eq("y", cid, yg[..., 4:4 + c.C], yref)
        assert np.isnan(yg[..., :4]).all() and np.isnan(yg[..., 4 + c.C:]).all(), \
            f"{cid}: columns outside the slice written"
        _eq("sum of ECA partials", cid, part.get("part").sum(1), yref.reshape(c.B, -1, c.C).sum(1))


def _wrapped(fn, *args, **kw):
    """fn(*args) and the names of the launches it made."""
    lib = _L()
    lib.launch_log_reset()
    out = fn(*args, **kw)
    return out, [n for n, _ in lib.launch_log()]


@pytest.mark.gpu
def test_training_wrappers_on_exact_data(cuda):
    """The same data through jabd_amd.train's wrappers (_dw_fwd_bn_stats,
    _dw_bwd, _dw_bn_bwd), which pick the mode themselves: no bias, BN-input
    relu, dz stored at stride 1 and NULL at stride 2; and F.dwconv with bias,
    relu and ECA partials on a contiguous tensor.  Every call's launches are
    the restated plan's."""
    from jabd_amd import functional as F
    from jabd_amd import train
    for c in E.CHAN_CASES:
        if c.C not in (12, 260):
            continue
        cid, d = "wrappers " + E.dw_id(c), E.dw_data(c)
        bn, M = d["bn"], c.B * E.out_size(c.H, c.k, c.s) * E.out_size(c.W, c.k, c.s)
        ref = E.dw_eval(c, d, act="relu")
        fwd, wg = E.dw_fwd_route(*c[1:]).name, E.wgrad_route(*c[1:]).name
        weight = _up(cuda, d["w"].T.reshape(c.C, 1, c.k, c.k))
        x, dy = _up(cuda, d["x"]), _up(cuda, d["dy"])
        st = tuple(_up(cuda, v) for v in (bn.gamma, bn.beta, bn.mean, bn.invstd))
        mod = torch.nn.BatchNorm2d(c.C).to(cuda)
        (y, wt, (mean, invstd)), log = _wrapped(train._dw_fwd_bn_stats, x, weight, c.s, mod,
                                                bnin=(st, "relu"))
        assert log == ["transpose", fwd, "bn_stats_final"], (cid, log)
        _eq("y", cid, y.cpu().numpy().astype(np.float64), ref["yb"])
        mean64, invstd64, _ = E.bn_stats_ref(ref["shiftb"], ref["Sb"], ref["Qb"], M, mod.eps)
        _ulp("mean", cid, mean.cpu().numpy(), mean64, 1)
        _ulp("invstd", cid, invstd.cpu().numpy(), invstd64, 1)
        (dx, dw), log = _wrapped(train._dw_bwd, dy, x, wt, c.k, c.s)
        assert log == ["dw_dgrad", wg, "dw_wgrad_reduce"], (cid, log)
        _eq("dx", cid, dx.cpu().numpy().astype(np.float64), ref["dx"])
        _eq("dW", cid, dw.cpu().numpy().astype(np.float64).reshape(c.C, -1), ref["dw"])
        (dxb, dgamma, dbeta, dwb), log = _wrapped(train._dw_bn_bwd, dy, None, wt, c.k, c.s, x, st,
                                                  "relu")
        store_dz = not (train.DGBN_RECOMPUTE and c.s == 2)
        assert log == E.dgbn_route(*c[1:], store_dz)[0] + [wg, "dw_wgrad_reduce"], (cid, log)
        _eq("dgamma", cid, dgamma.cpu().numpy().astype(np.float64), ref["dgamma"])
        _eq("dbeta", cid, dbeta.cpu().numpy().astype(np.float64), ref["dbeta"])
        _eq("dW (BN input)", cid, dwb.cpu().numpy().astype(np.float64).reshape(c.C, -1), ref["dwb"])
        dxr, bound = E.bn_dx_ref(ref["dz"], E.bn_xhat(d["x"], bn), bn, ref["dbeta"], ref["dgamma"],
                                 c.B * c.H * c.W)
        assert np.all(np.abs(dxb.cpu().numpy() - dxr) <= bound), f"{cid}: dx outside its bound"
        # F.dwconv: the plain forward's y (bias + relu) and its ECA partials
        (yi, part), log = _wrapped(F.dwconv, x, _up(cuda, d["w"]), _up(cuda, d["bias"]), c.k, c.s,
                                   act="relu", partials=True)
        assert log == ["dwconv"], (cid, log)
        assert tuple(part.shape) == (c.B, E.dw_nblk(c.B, *ref["y"].shape[1:3], c.C), c.C), cid
        E.assert_exact("sum y", np.abs(ref["y"]).reshape(c.B, -1, c.C).sum(1))
        _eq("F.dwconv y", cid, yi.cpu().numpy().astype(np.float64), ref["y"])
        _eq("F.dwconv partials", cid, part.cpu().numpy().astype(np.float64).sum(1),
            ref["y"].reshape(c.B, -1, c.C).sum(1))


# ------------------------------------------------------------------ switched forms
SWITCHES = {   # name -> (environment, run_case keywords, kernel families, cases)
    "fwd_rows_off": ({"JABD_DW_ROWS": "0"}, dict(fwd_rows=False), ("fwd", "fwdbn"),
                     E.CHAN_CASES + E.CHAN_FWD_ONLY + E.FWD_ROWS_CASES),
    "wgrad_rows_off": ({"JABD_DW_WGRAD_ROWS": "0"}, dict(wg_rows=False), ("wgrad", "wgradbn"),
                       E.CHAN_CASES + E.WG_ROWS_CASES),
    "dgrad_rows_on": ({"JABD_DW_DGRAD_ROWS": "1"}, dict(dg_rows=True), ("dgbn",),
                      E.CHAN_CASES + E.DG_ROWS_CASES + E.DGBN_SPB_CASES),
}


def _child(name):
    """One switched form, in this (fresh) process: the channel sweep and the
    row-chunk cases of the kernel the switch selects, same references, and the
    expected witness (run_case asserts the route with the switch applied)."""
    env, kw, want, cases = SWITCHES[name]
    for k, v in env.items():
        assert os.environ.get(k) == v, (k, os.environ.get(k))
    dev = torch.device("cuda:0")
    seen = set()
    for c in cases:
        run_case(dev, c, want=want, **kw)
        seen.add({"fwd_rows_off": E.dw_fwd_route(*c[1:], rows_on=False).name,
                  "wgrad_rows_off": E.wgrad_route(*c[1:], rows_on=False).name,
                  "dgrad_rows_on": E.dgbn_route(*c[1:], True, rows_on=True)[0][0]}[name])
    _report()
    print(f"child {name}: {len(cases)} cases ok, forms {sorted(seen)}")


@pytest.mark.gpu
def test_switched_forms_in_child_processes(cuda):
    """JABD_DW_ROWS=0, JABD_DW_WGRAD_ROWS=0 and JABD_DW_DGRAD_ROWS=1 are read
    once per process: one fresh child each, one after the other; a child that
    fails or times out fails the test and no further child is started."""
    for name, (env, _, _, _) in SWITCHES.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), name],
                           env={**os.environ, **env}, capture_output=True, text=True, timeout=240)
        print(r.stdout[-600:])
        assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        assert f"child {name}:" in r.stdout


if __name__ == "__main__":
    _child(sys.argv[1])
