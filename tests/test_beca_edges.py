"""BECA gate (csrc/beca.hip) at the branches tests/test_beca.py never runs,
against an fp64 restatement of the reference block and its autograd (inputs,
reference and metric: tests/_small_kernel_ref.py).

Why the inputs differ from test_beca.py's: there every channel's std is about
2 and the taps are N(0, 3), so v = conv1d(std) lands beyond the Hardsigmoid's
kinks for almost every gate (gate 0 or 1: y, dx and dw are trivially 0 or the
input, and the whole std backward could be deleted unnoticed).  Here the stds
span 80x and the taps are scaled so that about 25 / 50 / 25 % of the gates are
closed / linear / open; the CPU tests below assert that, and that no |v| lies
within 1e-3 of a kink (100x the fp32 error of v), before anything is compared.

Which case reaches which branch, (B, C, pixels, k):
  beca_part_kernel<0/1/2>, nblk > 1, short last chunk, C4 = 10 not dividing 256
                                   (2, 40, 2051, 3)  (chunks 1026 + 1025)
  beca_part_kernel, nblk = 1       (3, 64, 1155, 3), (2, 256, 100, 5), (1, 100, 63, 5)
  C4 = 256, TPX = 1 (the largest C of the LDS branch)     (2, 1024, 64, 5)
  the C4 > 256 branch, two chunks                         (2, 1028, 2050, 5)
  C < k, nblk at its cap of 64, TPX = 256                 (1, 4, 65613, 5)
  beca_stats_kernel mode 0 and mode 1 (C % 4 != 0), ragged last 64-channel
  group                            (3, 70, 129, 3), (2, 6, 300, 3), (2, 66, 2049, 9)
  beca_stats_kernel through the C ABI: part == NULL, part_floats one short,
  x and grad_y 4 bytes off a 16-byte boundary     test_abi_part_modes, both shapes
  y == NULL (gate only)                           test_abi_gate_only
  batch == 0, even k, k == 0                      test_contract_sizes
  std == 0 (a constant channel)                   test_constant_channel
  two-pass std under a mean 1300x the std         test_large_mean

Bars: this module keeps test_beca.py's 1e-5 forward and 1e-4 gradients, under
the per-slice metric.  The large-mean case is ill-conditioned by construction
(zero-mean taps over a nearly constant std: v is a difference of nearly equal
terms), so an honest fp32 evaluation is itself near the bar; its bar is
max(file bar, 4 x the error of the fp32 torch-CPU restatement against fp64),
computed in the test — the ratio tests/test_beca_model.py uses.  The four stats
rows get 1e-5: the longest sequential fp32 sum in any path is 1025 terms (the
C4 > 256 branch), a random-walk rounding error of sqrt(1025) * 2^-24 = 1.9e-6,
with a factor of 5 for the tail.

Worst error measured on the MI355X, per case, y / dx / dw:
  (2, 40, 2051, 3)    1.8e-7 / 1.8e-7 / 1.4e-7    fallback forms 1.6e-7 / 1.5e-7 / 1.6e-7
  (3, 64, 1155, 3)    1.9e-7 / 3.3e-7 / 1.9e-7
  (2, 256, 100, 5)    1.9e-7 / 3.7e-7 / 1.3e-7
  (1, 100, 63, 5)     1.1e-7 / 2.7e-7 / 4.0e-8
  (2, 1024, 64, 5)    5.5e-7 / 1.9e-6 / 9.6e-8
  (2, 1028, 2050, 5)  1.0e-6 / 1.1e-6 / 4.2e-7    fallback forms 3.2e-7 / 3.2e-7 / 2.0e-7
  (1, 4, 65613, 5)    5.1e-8 / 5.4e-8 / 1.3e-6
  (3, 70, 129, 3)     1.2e-7 / 1.4e-7 / 1.4e-7
  (2, 6, 300, 3)      8.5e-8 / 1.2e-7 / 1.5e-7
  (2, 66, 2049, 9)    1.8e-7 / 1.9e-7 / 3.3e-7
  constant channel    7.9e-8 / 8.6e-8 / 2.9e-8 (C = 8)    6.9e-8 / 3.2e-7 / 5.4e-8 (C = 6)
  large mean          partials 7.5e-6 / 7.5e-5 / 6.3e-7, fallback 5.6e-6 / 6.3e-5 / 3.6e-7,
                      bars 4.0e-5 / 2.1e-4 (the fp32 restatement: 1.0e-5 / 5.2e-5 / 5.8e-7)
  stats rows          at most 9.8e-7 (mean), 5.4e-7 (std), 4.0e-7 (v), 1.0e-6 (gate), all on
                      (2, 1028, 2050, 5)'s 1025-term chains
The large-mean fallback first measured dx 2.08e-4 against its 2.07e-4 bar: the
one-chain-per-thread sums of beca_stats_kernel rounded the mean by 3.5e-5 (an
fp32 emulation on the CPU reproduces the figure); the kernel now sums four
chains per thread.
"""
import ctypes

import pytest
import torch

import _small_kernel_ref as R

FWD_BAR, GRAD_BAR, STATS_BAR = 1e-5, 1e-4, 1e-5


# --------------------------------------------------------------- CPU self-checks
@pytest.mark.parametrize("case", R.BECA_CASES, ids=R.beca_id)
def test_recipe_conditions(case):
    """The conditions every comparison below rests on, checked on the fp64
    reference alone: no gate near a kink, every regime populated."""
    B, C, _, _ = case
    _, _, _, ref = R.beca_case(case)
    lo, lin, hi, margin = R.beca_regimes(ref["v"])
    assert margin >= R.KINK_MARGIN, margin
    if B * C >= 24:
        assert min(lo, lin, hi) >= R.REGIME_MIN, (lo, lin, hi)
    else:
        assert lin > 0, (lo, lin, hi)


def test_recipe_conditions_special_cases():
    for case, kind in ((R.BECA_LARGE_MEAN, "large_mean"),):
        _, _, _, ref = R.beca_case(case, kind)
        lo, lin, hi, margin = R.beca_regimes(ref["v"])
        assert margin >= R.KINK_MARGIN and min(lo, lin, hi) >= R.REGIME_MIN, (lo, lin, hi, margin)
    x, w, gy = _constant_channel_inputs(8)
    lo, lin, hi, margin = R.beca_regimes(R.beca_ref(x, w, gy)["v"])
    assert margin >= R.KINK_MARGIN and lin > 0


def test_fp32_restatement_is_within_a_quarter_of_the_bars():
    """An honest fp32 evaluation of the recipe cases sits far inside the bars,
    so a device error near a bar is the kernel's, not the inputs'."""
    for case in R.BECA_CASES:
        x, w, gy, ref = R.beca_case(case)
        e = R.beca_errors(R.beca_ref(x, w, gy, torch.float32), ref, x, gy)
        assert e["y"] <= FWD_BAR / 4 and e["dx"] <= GRAD_BAR / 4 and e["dw"] <= GRAD_BAR / 4, \
            (case, e)


def test_metric_sees_a_dropped_std_backward():
    """The defect test_beca.py's saturated cases cannot see — dx = g * gate
    alone, dw = 0 — is far over the bars on every recipe case."""
    for case in R.BECA_CASES:
        x, w, gy, ref = R.beca_case(case)
        bad = {"y": ref["y"], "dx": gy.double() * ref["gate"][:, None, :],
               "dw": torch.zeros_like(ref["dw"])}
        e = R.beca_errors(bad, ref, x, gy)
        assert e["dx"] > 10 * GRAD_BAR and e["dw"] > 10 * GRAD_BAR, (case, e)


# ----------------------------------------------------------------- device helpers
def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _to_dev(t, dev, misalign):
    """t on the device; misalign: a view 4 bytes into a larger buffer (torch's
    allocations are 512-byte aligned, so the view is 4 off a 16-byte boundary)."""
    if not misalign:
        return t.to(dev)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _abi_run(dev, x, w, gy, part_mode="full", y_null=False, misalign=False):
    """jabd_beca_fwd_f32 then _bwd_f32 through the C ABI.  part_mode: "full"
    (ops.beca_part), "null" (no workspace), "short" (part_floats one too small).
    Every output and the workspace start as NaN, so an element the kernels skip
    shows."""
    from jabd_amd import ops
    from jabd_amd._lib import call
    B, P, C = x.shape
    k = w.numel()
    xd, gd, wd = _to_dev(x, dev, misalign), _to_dev(gy, dev, misalign), w.to(dev)
    nan = float("nan")
    y = None if y_null else torch.full_like(xd, nan)
    stats = torch.full((4, B * C), nan, device=dev)
    parts = [ops.beca_part(B, P, C, dev).fill_(nan) for _ in range(2)]
    n = parts[0].numel()
    pp = [None, None] if part_mode == "null" else parts
    pf = n - 1 if part_mode == "short" else n
    st = ops._stream()
    call("jabd_beca_fwd_f32", _p(xd), B, P, C, _p(wd), k, _p(y), _p(stats), _p(pp[0]), pf, st)
    out = {"stats": stats}
    if y_null:
        return {"stats": stats.cpu()}
    dx, dw = torch.full_like(xd, nan), torch.full((k,), nan, device=dev)
    ws = torch.full((2, B * C), nan, device=dev)
    call("jabd_beca_bwd_f32", _p(xd), _p(gd), B, P, C, _p(wd), k, _p(stats), _p(dx), _p(dw),
         _p(ws), _p(pp[1]), pf, st)
    out.update(y=y, dx=dx, dw=dw)
    return {n: t.cpu() for n, t in out.items()}


def _check(tag, got, ref, x, gy, fwd_bar=FWD_BAR, grad_bar=GRAD_BAR):
    e = R.beca_errors(got, ref, x, gy)
    print("%s: y %.2e / %.1e  dx %.2e / %.1e  dw %.2e / %.1e"
          % (tag, e["y"], fwd_bar, e["dx"], grad_bar, e["dw"], grad_bar))
    assert e["y"] < fwd_bar, (tag, e)
    assert e["dx"] < grad_bar and e["dw"] < grad_bar, (tag, e)


def _ops_run(dev, x, w, gy):
    from jabd_amd import ops
    B, P, C = x.shape
    xg = x.view(B, 1, P, C).to(dev).requires_grad_(True)
    wg = w.to(dev).requires_grad_(True)
    y = ops.beca(xg, wg)
    y.backward(gy.view(B, 1, P, C).to(dev))
    return {"y": y.detach().view(B, P, C), "dx": xg.grad.view(B, P, C), "dw": wg.grad}


# ------------------------------------------------------------------------ parity
@pytest.mark.gpu
@pytest.mark.parametrize("case", R.BECA_CASES, ids=R.beca_id)
def test_beca_edge_parity(cuda, case):
    x, w, gy, ref = R.beca_case(case)
    _check(R.beca_id(case), _ops_run(cuda, x, w, gy), ref, x, gy)


@pytest.mark.gpu
def test_large_mean(cuda):
    """x = 64 + 0.05 * randn: a one-pass E[x^2] - E[x]^2 in fp32 would lose the
    variance (2.5e-3) in the rounding of 64^2 (2.4e-4 per term)."""
    x, w, gy, ref = R.beca_case(R.BECA_LARGE_MEAN, "large_mean")
    own = R.beca_errors(R.beca_ref(x, w, gy, torch.float32), ref, x, gy)
    print("fp32 restatement:", own)
    fwd_bar = max(FWD_BAR, 4 * own["y"])
    grad_bar = max(GRAD_BAR, 4 * max(own["dx"], own["dw"]))
    for tag, got in (("large-mean ops", _ops_run(cuda, x, w, gy)),
                     ("large-mean fallback", _abi_run(cuda, x, w, gy, "null"))):
        _check(tag, got, ref, x, gy, fwd_bar, grad_bar)
        if "stats" in got:
            e = R.beca_stats_errors(got["stats"], ref, w)
            print(tag, "stats", e)
            assert e["mean"] < STATS_BAR and e["std"] < STATS_BAR, e


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.BECA_ABI_CASES, ids=R.beca_id)
def test_abi_part_modes(cuda, case):
    """The partial-sum path and the one-workgroup-per-image fallback (reached by
    part == NULL, by part_floats one float short, and by a misaligned x /
    grad_y) all agree with fp64, each bit-identical run to run."""
    x, w, gy, ref = R.beca_case(case)
    for mode, mis in (("full", False), ("null", False), ("short", False), ("full", True)):
        tag = "%s part=%s%s" % (R.beca_id(case), mode, " misaligned" if mis else "")
        a = _abi_run(cuda, x, w, gy, mode, misalign=mis)
        b = _abi_run(cuda, x, w, gy, mode, misalign=mis)
        for n in a:
            assert torch.isfinite(a[n]).all(), (tag, n)
            assert torch.equal(a[n], b[n]), (tag, n, "differs run to run")
        _check(tag, a, ref, x, gy)
        e = R.beca_stats_errors(a["stats"], ref, w)
        print(tag, "stats", e)
        assert max(e.values()) < STATS_BAR, (tag, e)


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.BECA_ABI_CASES + ((3, 70, 129, 3),), ids=R.beca_id)
def test_abi_gate_only(cuda, case):
    """y == NULL writes the same four stats rows, bit for bit."""
    x, w, gy, ref = R.beca_case(case)
    for mode in ("full", "null"):
        full = _abi_run(cuda, x, w, gy, mode)["stats"]
        gate_only = _abi_run(cuda, x, w, gy, mode, y_null=True)["stats"]
        assert torch.isfinite(gate_only).all()
        assert torch.equal(full, gate_only), mode
        e = R.beca_stats_errors(gate_only, ref, w)
        assert max(e.values()) < STATS_BAR, (mode, e)


@pytest.mark.gpu
def test_contract_sizes(cuda):
    from jabd_amd import ops
    from jabd_amd._lib import call
    null, st = ctypes.c_void_p(0), ops._stream()
    # batch == 0 is a success before any pointer is looked at
    call("jabd_beca_fwd_f32", null, 0, 16, 8, null, 3, null, null, null, 0, st)
    call("jabd_beca_bwd_f32", null, null, 0, 16, 8, null, 3, null, null, null, null, null, 0, st)
    x = torch.randn(1, 2, 8, 8, device=cuda)
    for k in (0, 2, 4):
        w = torch.ones(max(k, 1), device=cuda)
        y, stats = torch.empty_like(x), torch.empty(4, 8, device=cuda)
        with pytest.raises(RuntimeError, match="bad size"):
            call("jabd_beca_fwd_f32", _p(x), 1, 16, 8, _p(w), k, _p(y), _p(stats), null, 0, st)
        with pytest.raises(RuntimeError, match="bad size"):
            call("jabd_beca_bwd_f32", _p(x), _p(x), 1, 16, 8, _p(w), k, _p(stats), _p(y), _p(w),
                 _p(stats), null, 0, st)
    with pytest.raises(RuntimeError, match="bad size"):
        ops.beca(x, torch.ones(4, device=cuda))


def _constant_channel_inputs(C):
    x = R.beca_x(2, C, 50, 11).clone()
    x[1, :, 3] = 2.0
    return x, R.beca_taps(x, 3, 11), torch.randn(2, 50, C, generator=torch.Generator().manual_seed(12))


@pytest.mark.gpu
@pytest.mark.parametrize("C", [8, 6], ids=["partials", "fallback"])
def test_constant_channel(cuda, C):
    """A constant channel has std exactly 0.  The reference block's autograd
    divides by it: dx is NaN in exactly that (b, c) slice — the kernel's
    dstd * (x - mean) / (P * std) = 0 / 0 likewise — and nothing else is touched."""
    x, w, gy = _constant_channel_inputs(C)
    ref = R.beca_ref(x, w, gy)
    got = _abi_run(cuda, x, w, gy, "full")
    stats = got["stats"].view(4, 2, C)
    assert float(stats[0, 1, 3]) == 2.0 and float(stats[1, 1, 3]) == 0.0
    assert float(ref["std"][1, 3]) == 0.0
    dead = torch.zeros(2, 50, C, dtype=torch.bool)
    dead[1, :, 3] = True
    for name, r in (("reference", ref), ("kernel", got)):
        assert torch.isfinite(r["y"]).all() and torch.isfinite(r["dw"]).all(), name
        assert torch.equal(torch.isnan(r["dx"]), dead), name
    # everything outside the dead slice is held to the usual bars
    keep = (~dead).double()
    fix = lambda r: {"y": r["y"], "dw": r["dw"], "dx": torch.nan_to_num(r["dx"].double()) * keep}
    _check("constant-channel C=%d" % C, fix(got), fix(ref), x, gy)
