"""Exact-data edge tests of the BatchNorm training kernels of csrc/train.hip:
bn_stats_part / bn_stats_final, bn_act_fwd, bn_act_fwd_sum and bn_bwd_part /
bn_bwd_final / bn_bwd_apply, through the C ABI.  Inputs, fp64 references, case
tables and planted defects: tests/_dw_bn_exact.py.

x, dy, res and the dy transform are small nonzero integers; where statistics
are passed in they are dyadic (integer mean, power-of-two invstd, gamma with
invstd * gamma an integer, beta = integer + 0.5, so no pre-activation is on a
kink).  Every sum is then exact in fp32 in any order:
  bn_stats        the shifted sums are exact, the final kernel works in fp64 and
                  rounds once: mean, invstd <= 1 ulp of the fp64 value rounded
                  to fp32, the running buffers <= 2 ulp (momentum 0.1 and 1.0)
  bn_act_fwd      y EQUALS the reference; columns outside [yc0, yc0 + C) of a
                  wider y keep their prefill
  bn_act_fwd_sum  y equals bn_act_fwd's bit for bit, the channel-sum partials
                  EQUAL the sums of y over each row block
  bn_act_bwd_ex   dbeta, dgamma and dres EQUAL the reference; dx within the
                  elementwise bound derived in _dw_bn_exact.bn_dx_ref
Every output body is prefilled with NaN and must come back finite; every
output carries a 64-float sentinel tail that must come back bit-identical; the
launch log must name the kernels.

Cases.  bn_stats and the backward: C in {4, 12, 72, 1024, 1028, 2048} (lanes
1 / 3 / 18 of a 256-thread block, the channel loop's second pass with one live
lane at 1028, two full passes at 2048) x M in {2, rows_pass - 1, rows_pass,
rows_pass + 1, 8 * rows_pass + 1, 2053}; bn_stats with ldx = C and C + 8; the
backward with and without res / dres, dy at column 4 of a C + 8 wide buffer,
and the dy transform with hw in {1, 3, 64} (a thread's consecutive rows cross
images on every step; hw > rows_pass at C = 72 and 1028).  bn_act_fwd: M on
both sides of the full-block test, res with ldr != C, ldy = C + 8 with yc0 0
and 4, none / relu / leaky(0.5).  bn_act_fwd_sum: C in {12, 72, 256, 260},
hw = one and three row blocks, B = 3.

Non-gpu self-checks: the 2^24 condition and order independence for every
case; a numpy fp32 evaluation of bn_bwd_apply_kernel's expression stays within
half of the dx bound; the planted defects (the last row of a block counted
twice, the live lane of the channel loop's second pass skipped) break
equality; the restated block counts equal jabd_bn_nblk / jabd_bn_sum_nblk; the
C ABI's rejections.

Worst distance observed on the MI355X next to its bar:
  bn_stats   mean 0 ulp / 1   invstd 0 ulp / 1   running_mean 0 ulp / 2   running_var 1 ulp / 2
  backward   dx 0.31 of the derived bound / 1 (a numpy fp32 evaluation: 0.32)
Forms witnessed: bn_stats_part + bn_stats_final, bn_act_fwd, bn_act_fwd_sum,
bn_bwd_part + bn_bwd_final + bn_bwd_apply (each with and without res; the
backward with and without the dy transform).  No case was taken out.
"""
import numpy as np
import pytest
import torch

import _dw_bn_exact as E
import _dw_bn_device as D
from _dw_bn_device import Out, L as _L, eq as _eq, logged as _logged, scratch as _scratch, up as _up

EPS = E.EPS
FIG = D.Figures()     # worst observed distances of this module's device runs
_note, _report = FIG.note, FIG.report


def _ulp(*a):
    D.ulp(FIG, *a)


# ------------------------------------------------------------------ CPU self-checks
def test_stats_exactness_and_order_independence():
    for c in E.BN_STATS_CASES:
        if c.pad_ld:
            continue                                  # same data as the ldx = C case
        x = E.bn_stats_data(c)
        assert np.all(x != 0) and np.array_equal(x, np.round(x))
        S, Q = E.bn_stats_sums(x)
        E.assert_exact("sum d", np.abs(x - x[0]).sum(0))
        E.assert_exact("sum d^2", Q)
        for sm in (E.Summer(f32=True), E.Summer(f32=True, seed=5)):
            S2, Q2 = E.bn_stats_sums(x, sm)
            assert np.array_equal(S, S2) and np.array_equal(Q, Q2), E.bn_id(c)
        mean, invstd, unb = E.bn_stats_ref(x[0], S, Q, c.M)
        assert invstd[1] == np.float64(1.0 / np.sqrt(np.longdouble(np.float32(EPS))))  # var = 0
        assert np.allclose(mean, x.mean(0), rtol=1e-13, atol=1e-13)
        assert np.allclose(invstd, 1 / np.sqrt(x.var(0) + EPS), rtol=1e-6)


def test_backward_exactness_and_order_independence():
    for c in E.BN_BWD_CASES:
        d = E.bn_bwd_data(c)
        E.bn_bwd_conditions(c, d)
        ref = E.bn_bwd_eval(c, d)
        for sm in (E.Summer(f32=True), E.Summer(f32=True, seed=5)):
            got = E.bn_bwd_eval(c, d, sm)
            assert np.array_equal(ref["dbeta"], got["dbeta"]), E.bn_id(c)
            assert np.array_equal(ref["dgamma"], got["dgamma"]), E.bn_id(c)


def test_forward_operands_are_exact():
    """y of bn_act_fwd and the channel sums of bn_act_fwd_sum: fp32, op for op
    as the kernels compute them, equals fp64."""
    f = np.float32
    for c in E.BN_ACT_CASES:
        d = E.bn_act_data(tuple(c), c.M, c.C)
        bn = d["bn"]
        y32 = (f(d["x"]) - f(bn.mean)) * f(bn.invstd) * f(bn.gamma) + f(bn.beta)
        y32 = E.act_f((y32 + f(d["res"])) if c.res else y32, c.act)
        assert y32.dtype == f and np.array_equal(y32.astype(np.float64), E.bn_act_ref(d, c.act, c.res))
        assert not np.any(E.bn_z(d["x"], bn, d["res"] if c.res else None) == 0)
    for c in E.BN_SUM_CASES:
        hw = c.blocks * E.bn_sum_rows(c.C)
        d = E.bn_act_data(tuple(c), E.BN_SUM_B * hw, c.C)
        y = E.bn_act_ref(d, c.act, False).reshape(-1, E.bn_sum_rows(c.C), c.C)
        E.assert_quantum("y", y, 0.25)
        E.assert_exact("channel sums", np.abs(y).sum(1), 0.25)


def test_dx_bound_holds_for_an_honest_fp32_evaluation():
    """bn_bwd_apply_kernel's expression in numpy fp32 stays within half of the
    derived bound (BatchNorm cases and the fused depthwise data gradient's)."""
    worst = 0.0
    todo = [(E.bn_id(c), E.bn_bwd_data(c), c) for c in E.BN_BWD_CASES]
    for name, d, c in todo:
        e = E.bn_bwd_eval(c, d)
        dx, bound = E.bn_dx_ref(e["dz"], e["xh"], d["bn"], e["dbeta"], e["dgamma"], c.M)
        got = E.bn_dx_f32(e["dz"], e["xh"], d["bn"], e["dbeta"], e["dgamma"], c.M)
        frac = np.max(np.abs(got.astype(np.float64) - dx) / np.maximum(bound, 1e-300))
        worst = max(worst, frac)
        assert frac <= 0.5, f"{name}: {frac:.3f} of the bound"
    for c in E.CHAN_CASES + E.DGBN_SPB_CASES:
        d = E.dw_data(c)
        r = E.dw_eval(c, d, want=("dgbn",))
        xh, M = E.bn_xhat(d["x"], d["bn"]), c.B * c.H * c.W
        dx, bound = E.bn_dx_ref(r["dz"], xh, d["bn"], r["dbeta"], r["dgamma"], M)
        got = E.bn_dx_f32(r["dz"], xh, d["bn"], r["dbeta"], r["dgamma"], M)
        frac = np.max(np.abs(got.astype(np.float64) - dx) / np.maximum(bound, 1e-300))
        worst = max(worst, frac)
        assert frac <= 0.5, f"{E.dw_id(c)}: {frac:.3f} of the bound"
    print(f"fp32 evaluation: worst {worst:.3f} of the bound")


def test_planted_defects_are_caught():
    n = 0
    for c in E.BN_STATS_CASES:
        if c.pad_ld or E.bn_nblk(c.M, c.C) < 2:
            continue
        x = E.bn_stats_data(c)
        S, Q = E.bn_stats_sums(x)
        S2, Q2 = E.bn_stats_sums(x, E.Summer(f32=True), "dup_row", E.bn_rows_per_blk(c.M, c.C))
        assert not np.array_equal(Q, Q2) or not np.array_equal(S, S2), E.bn_id(c)
        n += 1
    assert n >= 12
    n = 0
    for c in E.BN_BWD_CASES:
        d = E.bn_bwd_data(c)
        ref = E.bn_bwd_eval(c, d)
        if E.bn_nblk(c.M, c.C) >= 2:
            bad = E.bn_bwd_eval(c, d, E.Summer(f32=True), "dup_row")
            assert not np.array_equal(ref["dbeta"], bad["dbeta"]), E.bn_id(c)
            assert not np.array_equal(ref["dgamma"], bad["dgamma"]), E.bn_id(c)
            n += 1
        if c.C == 1028:
            bad = E.bn_bwd_eval(c, d, E.Summer(f32=True), "skip_lane")
            assert not np.array_equal(ref["dbeta"], bad["dbeta"]), E.bn_id(c)
    assert n >= 12


def test_restated_block_counts_equal_the_exported_ones():
    h = _L().lib()
    for C in sorted(set(E.BN_C) | {8, 16, 64, 256, 260, 512, 1020}):
        for M in (1, 2, 3, 84, 85, 86, 255, 256, 257, 1024, 1025, 2053, 70000, 1 << 20):
            assert h.jabd_bn_nblk(M, C) == E.bn_nblk(M, C), (M, C)
        rb = E.bn_sum_rows(C)
        for hw in (rb, 3 * rb, rb + 1, rb // 2, 1):
            assert h.jabd_bn_sum_nblk(hw, C) == E.bn_sum_nblk(hw, C), (hw, C)
    assert (E.bn_sum_rows(12), E.bn_sum_rows(72), E.bn_sum_rows(256), E.bn_sum_rows(260)) == \
        (512, 64, 32, 32)
    assert h.jabd_bn_nblk(5, 10) == -1 and h.jabd_bn_sum_nblk(5, 10) == 0
    for c in E.BN_ACT_CASES:                       # M on both sides of the full-block test
        assert c.M in (1, 7 * E.ew_rows_pass(c.C), 7 * E.ew_rows_pass(c.C) + 1,
                       8 * E.ew_rows_pass(c.C) + 3)


def test_argument_rejection_through_the_c_abi():
    """bn_act_fwd_sum with hw off its row block, and bad channel counts /
    leading dimensions, return JABD_EINVAL and launch nothing."""
    L = _L()
    h = L.lib()
    p = _scratch(1 << 18).data_ptr()
    L.launch_log_reset()
    rb = E.bn_sum_rows(12)
    assert h.jabd_bn_sum_nblk(rb + 8, 12) == 0
    assert h.jabd_bn_act_fwd_sum_f32(p, 3 * (rb + 8), 12, p, p, p, p, 1, 0.0, p, rb + 8, p, None) == 1
    assert "row block" in L.last_error()
    assert h.jabd_bn_act_fwd_sum_f32(p, 3 * rb + 1, 12, p, p, p, p, 1, 0.0, p, rb, p, None) == 1
    assert h.jabd_bn_stats_f32(p, 10, 16, 10, p, p, p, p, p, 0.1, EPS, None) == 1      # C % 4
    assert h.jabd_bn_stats_f32(p, 14, 16, 12, p, p, p, p, p, 0.1, EPS, None) == 1      # ldx % 4
    assert h.jabd_bn_act_fwd_f32(p, 12, 16, 12, p, p, p, p, None, 0, 1, 0.0, p, 14, 0, None) == 1
    assert h.jabd_bn_act_fwd_f32(p, 12, 16, 12, p, p, p, p, None, 0, 1, 0.0, p, 16, 2, None) == 1
    assert h.jabd_bn_act_bwd_ex_f32(p, 16, 2, p, 12, None, 0, 16, 12, p, p, p, p, 1, 0.0, None, None,
                                    0, p, p, p, p, None, None) == 1                    # dyc0 % 4
    assert h.jabd_bn_act_bwd_ex_f32(p, 12, 0, p, 12, None, 0, 16, 12, p, p, p, p, 1, 0.0, p, p,
                                    5, p, p, p, p, None, None) == 1                    # M % hw
    assert L.launch_log() == []


# ------------------------------------------------------------------ GPU cases
def _widen(a, width, c0=0, fill=7.0):
    out = np.full((a.shape[0], width), fill)
    out[:, c0:c0 + a.shape[1]] = a
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("C", E.BN_C)
def test_bn_stats(cuda, C):
    L = _L()
    for c in E.BN_STATS_CASES:
        if c.C != C:
            continue
        cid = "bn_stats " + E.bn_id(c)
        x = E.bn_stats_data(c)
        S, Q = E.bn_stats_sums(x)
        E.assert_exact("sum d^2", Q)                  # before any device work
        mean64, invstd64, unb64 = E.bn_stats_ref(x[0], S, Q, c.M)
        ldx = C + c.pad_ld
        xd = _up(cuda, _widen(x, ldx))
        nblk = int(L.lib().jabd_bn_nblk(c.M, C))
        part, mean, invstd = Out(cuda, nblk, 2, C), Out(cuda, C), Out(cuda, C)
        mom = 1.0 if (c.M + c.pad_ld // 8) % 2 else 0.1
        rm0, rv0 = E.running_start(mean64), np.ones(C)
        rm, rv = Out(cuda, C, init=rm0), Out(cuda, C, init=rv0)
        log = _logged("jabd_bn_stats_f32", xd.data_ptr(), ldx, c.M, C, part.ptr, mean.ptr,
                      invstd.ptr, rm.ptr, rv.ptr, mom, EPS, None)
        assert log == ["bn_stats_part", "bn_stats_final"], (cid, log)
        pt = part.get("partials")
        _eq("sum of partials (S)", cid, pt[:, 0].sum(0), S)
        _eq("sum of partials (Q)", cid, pt[:, 1].sum(0), Q)
        _ulp("mean", cid, mean.get("mean"), mean64, 1)
        _ulp("invstd", cid, invstd.get("invstd"), invstd64, 1)
        _ulp("running_mean", cid, rm.get("running_mean"), E.running_ref(rm0, mean64, mom), 2)
        _ulp("running_var", cid, rv.get("running_var"), E.running_ref(rv0, unb64, mom), 2)
    _report()


def _bn_ptrs(dev, bn):
    ts = [_up(dev, v) for v in (bn.mean, bn.invstd, bn.gamma, bn.beta)]
    return ts, [t.data_ptr() for t in ts]


@pytest.mark.gpu
def test_bn_act_fwd(cuda):
    for c in E.BN_ACT_CASES:
        cid = "bn_act_fwd " + E.bn_id(c)
        d = E.bn_act_data(tuple(c), c.M, c.C)
        ref = E.bn_act_ref(d, c.act, c.res)
        keep, bp = _bn_ptrs(cuda, d["bn"])
        ldx, ldr, ldy = c.C + 8, c.C + 4, c.C + 8
        x, res = _up(cuda, _widen(d["x"], ldx)), _up(cuda, _widen(d["res"], ldr))
        y = Out(cuda, c.M, ldy)
        log = _logged("jabd_bn_act_fwd_f32", x.data_ptr(), ldx, c.M, c.C, *bp,
                      res.data_ptr() if c.res else None, ldr, E.ACT[c.act], E.SLOPE, y.ptr, ldy,
                      c.yc0, None)
        assert log == ["bn_act_fwd"], (cid, log)
        yg = y.get("y", finite=False)
        _eq("y", cid, yg[:, c.yc0:c.yc0 + c.C], ref)
        assert np.isnan(yg[:, :c.yc0]).all() and np.isnan(yg[:, c.yc0 + c.C:]).all(), \
            f"{cid}: columns outside [yc0, yc0 + C) written"


@pytest.mark.gpu
def test_bn_act_fwd_sum(cuda):
    L = _L()
    for c in E.BN_SUM_CASES:
        cid = "bn_act_fwd_sum " + E.bn_id(c)
        rb = E.bn_sum_rows(c.C)
        hw = c.blocks * rb
        M = E.BN_SUM_B * hw
        d = E.bn_act_data(tuple(c), M, c.C)
        ref = E.bn_act_ref(d, c.act, False)
        E.assert_exact("channel sums", np.abs(ref).reshape(-1, rb, c.C).sum(1), 0.25)
        keep, bp = _bn_ptrs(cuda, d["bn"])
        x = _up(cuda, d["x"])
        nb = int(L.lib().jabd_bn_sum_nblk(hw, c.C))
        assert nb == c.blocks
        y, part, y0 = Out(cuda, M, c.C), Out(cuda, E.BN_SUM_B, nb, c.C), Out(cuda, M, c.C)
        log = _logged("jabd_bn_act_fwd_sum_f32", x.data_ptr(), M, c.C, *bp, E.ACT[c.act], E.SLOPE,
                      y.ptr, hw, part.ptr, None)
        assert log == ["bn_act_fwd_sum"], (cid, log)
        _logged("jabd_bn_act_fwd_f32", x.data_ptr(), c.C, M, c.C, *bp, None, 0, E.ACT[c.act],
                E.SLOPE, y0.ptr, c.C, 0, None)
        yg = y.get("y")
        _eq("y", cid, yg, ref)
        assert np.array_equal(yg, y0.get("y of bn_act_fwd")), f"{cid}: y differs from bn_act_fwd's"
        _eq("channel-sum partials", cid, part.get("part"),
            ref.reshape(E.BN_SUM_B, nb, rb, c.C).sum(2))


@pytest.mark.gpu
@pytest.mark.parametrize("C", E.BN_C + (260,))
def test_bn_act_bwd(cuda, C):
    L = _L()
    for c in E.BN_BWD_CASES:
        if c.C != C:
            continue
        cid = "bn_act_bwd " + E.bn_id(c)
        d = E.bn_bwd_data(c)
        E.bn_bwd_conditions(c, d)                     # before any device work
        e = E.bn_bwd_eval(c, d)
        dxr, bound = E.bn_dx_ref(e["dz"], e["xh"], d["bn"], e["dbeta"], e["dgamma"], c.M)
        keep, bp = _bn_ptrs(cuda, d["bn"])
        lddy = C + E.BWD_DY_PAD
        dy = _up(cuda, _widen(d["dy"], lddy, E.BWD_DYC0))
        x, res = _up(cuda, d["x"]), _up(cuda, d["res"])
        dys = _up(cuda, d["dys"]) if c.hw else None
        dya = _up(cuda, d["dya"]) if c.hw else None
        nblk = int(L.lib().jabd_bn_nblk(c.M, C))
        part, dgamma, dbeta = Out(cuda, nblk, 2, C), Out(cuda, C), Out(cuda, C)
        dx = Out(cuda, c.M, C)
        dres = Out(cuda, c.M, C) if c.res else None
        log = _logged("jabd_bn_act_bwd_ex_f32", dy.data_ptr(), lddy, E.BWD_DYC0, x.data_ptr(), C,
                      res.data_ptr() if c.res else None, C, c.M, C, *bp, E.ACT[c.act], E.SLOPE,
                      dys.data_ptr() if c.hw else None, dya.data_ptr() if c.hw else None, c.hw,
                      part.ptr, dgamma.ptr, dbeta.ptr, dx.ptr, dres.ptr if c.res else None, None)
        assert log == ["bn_bwd_part", "bn_bwd_final", "bn_bwd_apply"], (cid, log)
        pt = part.get("partials")
        _eq("sum of partials (dz)", cid, pt[:, 0].sum(0), e["dbeta"])
        _eq("dbeta", cid, dbeta.get("dbeta"), e["dbeta"])
        _eq("dgamma", cid, dgamma.get("dgamma"), e["dgamma"])
        if c.res:
            _eq("dres", cid, dres.get("dres"), e["dz"])
        err = np.abs(dx.get("dx") - dxr)
        frac = np.max(err / np.maximum(bound, 1e-300))
        _note("bn_bwd dx / bound", frac)
        assert np.all(err <= bound), f"{cid} dx: {frac:.3g} of the bound"
    _report()
