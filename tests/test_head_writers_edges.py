"""Parity of the kernels that write loc / conf / landm, and of the ECA pool, each
on its own and at its edges (references, inputs, case tables: tests/_head_ref.py).

heads_kernel (head.hip): HW 1 .. 400 at C = 40 (wave and workgroup tails, waves
with npx <= 0, the 20 x 20 level), C = 4 / 36 / 64 / 256, B = 1 / 3, a_off 0 /
6 / 130, softmax on and off, a channel-offset view with NaN around it, a
saturated softmax.  heads_scatter_kernel: the same HW list, plain / saturated /
equal logits.  heads_gather_kernel (train.hip): the same HW list, bit for bit.
ssh_tail_heads_kernel (ssh.hip): maps from 1 x 1 to 17 x 65 around its 8 x 32
tile, c33 contiguous and as a 20-of-32-channel view, through
engine.ssh_tail_pack.  channel_sum_kernel: C = 4 .. 960 over its three thread
mappings, blocks past the end, a channel-offset view.  Every output sits in a
guarded buffer (_head_ref.Guarded): 128 sentinel rows around each owed range,
owed rows NaN before the call; afterwards every owed element is finite and every
other one bit-identical.  jabd_heads_f32 and jabd_heads_gather_f32 refuse odd
A / a_off, a range past A and empty shapes.

Bars, the honest fp32 CPU error against fp64 (H), and the worst seen on the
MI355X (D), per kernel and group; for the derived per-element bars the figures
are the worst err / bar ratio:
  heads logits (loc, landm, conf without softmax)
      bar (C + 2) 2^-24 (|b| + sum|W x|), derived        H 0.086   D 0.090
      (at C = 4 the inputs sit on a grid and both are exactly 0: _head_ref.heads_inputs)
  heads conf with softmax
      bar 0.25 (d0 + d1) + r                             H 0.127   D 0.149
      r = SOFTMAX_R = 3.5e-7 = 4 x 8.64e-8, the worst torch-fp32 CPU softmax
      error over the exact fp32 logits of every heads and scatter case
  heads_scatter   loc / landm / conf logits bit-identical; conf softmax within r
                                                         H 8.1e-8  D 8.1e-8 (0.23 r)
  heads_gather    bit-identical
  ssh tail, max-norm relative error per tensor and image, bar 2e-5
      loc           H 2.7e-7     D 3.6e-7
      conf logits   H 2.5e-7     D 2.2e-7
      conf softmax  H 1.8e-7     D 1.9e-7
      landm         H 2.8e-7     D 3.3e-7
  ssh tail, _util.elem_rel_err (floor 1e-2) per tensor and image; the bar is
  4 x H rounded up in the second digit
      loc           bar 6.3e-5   H 1.565e-5   D 1.69e-5
      conf logits   bar 5.2e-5   H 1.278e-5   D 1.14e-5
      conf softmax  bar 2.7e-6   H 6.71e-7    D 1.03e-6
      landm         bar 5.3e-5   H 1.321e-5   D 1.71e-5
  channel_sum     bar n 2^-24 sum|x| (n pixels in the block), derived
                                                         H 0.201   D 0.136
No device figure is within 2x of its bar (the nearest is the SSH tail's conf
softmax elem_rel_err at 0.38 of it).

H for the SSH tail has to be one number on every machine, or a bar of 4 x H and
a check against a quarter of it cannot both hold.  Three things moved it by up
to 15 % between two CPUs and are avoided in _head_ref: torch's float32 conv2d
and matmul (blocking and FMA use depend on thread count and CPU; conv_taps
does one IEEE multiply and add per tap and channel), its float32 sqrt in the
BatchNorm fold and its vectorised expf (both taken through float64, which
rounds correctly).  All inputs are drawn in float64 and rounded (_randn).

CPU self-checks (not marked gpu): the index-arithmetic layout equals the
reference model's permute / view / cat bit for bit over three levels; the
hand-folded fp64 SSH graph equals the SSH module's own Conv2d / BatchNorm2d
forwards in double; honest fp32 stays within a quarter of every bar on every
case; the guard helper reports a fake kernel that writes one row too many or
too few and passes a correct one; each planted defect of the CPU emulation is
caught by these cases:
  swap_anchors (the position's two anchors exchanged): every heads and scatter
      case, through loc and landm (named: hw1, hw257, c256-hw300, plain-hw1)
  shift_rows (rows a_off + 2p + 2): every heads and scatter case, by the guard
      behind the level and by the level's first two rows left NaN
  wrong_pair (softmax over (c0, c2), (c1, c3)): every softmax-on case (heads
      hw1, hw64, hw65, hw256, hw257, hw400, c4-hw65, c36-hw257, c256-hw300,
      view-hw257, saturated-hw300; scatter: all but plain-hw65)
  u_outside (conv7X7_2 evaluated outside the image instead of zero): all nine
      SSH cases
  halo1 (1-pixel t halo): the SSH cases with more than one tile: 9x33, 17x65,
      20x20, 1x70, 40x1
  frag12 (conv7x7_3's head-weight fragment read at channel 20 + 12): all nine
  drop_last_group (channel_sum's last row group dropped): every case whose last
      group holds a pixel (named: c4-hw1000-n3, c40-hw256-n1, c100-hw63-n3,
      c128-hw63-n3, c960-hw256-n3)
  floor_per (block ranges with floor(HW / nblk)): every case with HW % nblk != 0
      (c4-hw1000-n3, c16-hw63-n64, c72-hw1000-n64, c200-hw256-n3, c250-hw1-n64,
      c480-hw1-n3, c960-hw256-n3, c960-hw63-n64)
"""
import copy

import pytest
import torch

import _head_ref as R

QUARTER = 0.25


def _by_name(table, name):
    hits = [c for c in table if c.name == name]
    assert len(hits) == 1, name
    return hits[0]


# --------------------------------------------------------------- CPU self-checks
def test_tables_cover_every_axis_value():
    assert sorted(c.HW for c in R.HEADS_CASES if c.C == 40 and c.kind == "plain") == list(R.HEADS_HW)
    assert {c.C for c in R.HEADS_CASES} == set(R.HEADS_C)
    assert {c.B for c in R.HEADS_CASES} == {1, 3}
    assert {c.a_off for c in R.HEADS_CASES} == {0, R.A_OFF_SMALL, R.A_OFF_BIG}
    assert {c.softmax for c in R.HEADS_CASES} == {True, False}
    assert {c.kind for c in R.HEADS_CASES} == {"plain", "view", "saturated"}
    for table in (R.SCATTER_CASES, R.GATHER_CASES):
        assert sorted(c.HW for c in table) == list(R.HEADS_HW)
        assert {c.B for c in table} == {1, 3} and {c.a_off > 0 for c in table} == {True, False}
    assert {c.kind for c in R.SCATTER_CASES} == {"plain", "saturated", "equal"}
    assert any(not c.softmax for c in R.SCATTER_CASES)
    assert [(c.H, c.W) for c in R.SSH_CASES] == list(R.SSH_HW)
    for axis in ("B", "view", "softmax"):
        assert len({getattr(c, axis) for c in R.SSH_CASES}) == 2, axis
    assert {c.a_off > 0 for c in R.SSH_CASES} == {True, False}
    assert {c.C for c in R.CSUM_CASES} >= set(R.CSUM_C)
    assert {c.HW for c in R.CSUM_CASES} == set(R.CSUM_HW)
    assert {c.nblk for c in R.CSUM_CASES} == set(R.CSUM_NBLK)
    assert any(c.nblk > c.HW for c in R.CSUM_CASES) and any(c.view for c in R.CSUM_CASES)
    for table in (R.HEADS_CASES, R.SCATTER_CASES, R.GATHER_CASES, R.SSH_CASES, R.CSUM_CASES):
        assert len({c.name for c in table}) == len(table)
        assert all(c.a_off % 2 == 0 for c in table if hasattr(c, "a_off"))


def _level_shapes(case):
    """Three levels with the case's own level at the case's a_off."""
    own = (case.H, case.W) if hasattr(case, "H") else (1, case.HW)
    if case.a_off:
        return [(1, case.a_off // 2), own, (1, 5)], 1
    return [own, (1, 7), (1, 5)], 0


@pytest.mark.parametrize("case", R.HEADS_CASES + R.SSH_CASES, ids=R.case_id)
def test_index_layout_equals_permute_view_cat(case):
    shapes, own = _level_shapes(case)
    g = torch.Generator().manual_seed(case.seed)
    # float64: there write_level's softmax is torch.softmax, as the reference model's
    levels = [torch.randn(case.B, 32, h, w, generator=g, dtype=torch.float64) for h, w in shapes]
    for softmax in (False, True):
        ref = R.layout_permute(levels, softmax)
        A = ref["loc"].shape[1]
        out = {n: torch.full((case.B, A, k), float("nan"), dtype=torch.float64)
               for n, k in (("loc", 4), ("conf", 2), ("landm", 10))}
        a_off = 0
        for i, o in enumerate(levels):
            assert i != own or a_off == case.a_off
            rows = o.permute(0, 2, 3, 1).reshape(case.B, -1, 32)
            R.write_level(rows, out["loc"], out["conf"], out["landm"], a_off, softmax)
            a_off += 2 * rows.shape[1]
        assert a_off == A
        for n in out:
            assert torch.equal(out[n].view(torch.int64), ref[n].view(torch.int64)), (n, softmax)
    # and the gather is the inverse
    rows = levels[own].permute(0, 2, 3, 1).reshape(case.B, -1, 32)
    back = R.gather_rows(out["loc"], R.layout_permute(levels)["conf"], out["landm"],
                         rows.shape[1], case.a_off)
    assert torch.equal(back, rows)


@pytest.mark.parametrize("case", R.SSH_CASES, ids=R.case_id)
def test_ssh_folded_graph_equals_the_modules(case):
    inp = R.ssh_inputs(case)
    with torch.no_grad():
        folded = R.ssh_features(inp)
    mods = R.ssh_graph_from_modules(inp)
    assert float((folded - mods).abs().max()) <= 1e-12 * float(mods.abs().max())
    assert float((folded[:, 20:] > 0).float().mean()) > 0.2      # the branches are alive


def test_softmax_term_is_four_times_the_measured_error():
    worst = R.softmax_fp32_worst()
    print(f"torch-fp32 CPU softmax worst {worst:.3e}, r {R.SOFTMAX_R:.3e}")
    # torch's vectorised expf is not the same code on every CPU: r is tied to the
    # measurement to within a factor 1.5 either way
    assert R.SOFTMAX_R / 1.5 <= 4 * worst <= 1.5 * R.SOFTMAX_R


def test_saturated_and_equal_inputs_do_what_they_say():
    case = _by_name(R.HEADS_CASES, "saturated-hw300")
    o = R.heads_ref(case)["o"]
    assert float((o[..., 8] - o[..., 9]).min()) > 100 and float((o[..., 10] - o[..., 11]).min()) > 100
    conf = R.heads_ref(case)["ref"]["conf"]
    assert float((conf - torch.tensor([1.0, 0.0], dtype=torch.float64)).abs().max()) < 1e-40
    for c in R.SCATTER_CASES:
        ref = R.layout_index(R.scatter_inputs(c).double(), True)["conf"]
        if c.kind == "saturated":
            assert float(torch.minimum(ref, 1 - ref).max()) < 1e-40
        elif c.kind == "equal":
            assert bool((ref == 0.5).all())


@pytest.mark.parametrize("case", R.HEADS_CASES, ids=R.case_id)
def test_heads_case_is_benign_in_fp32(case):
    ref = R.heads_ref(case)
    probs, worst = R.bar_check(R.heads_emulate(case), ref["ref"], ref["bar"], QUARTER)
    print(case.name, worst)
    assert not probs, probs


@pytest.mark.parametrize("case", R.SCATTER_CASES, ids=R.case_id)
def test_scatter_case_is_benign_in_fp32(case):
    assert not R.scatter_check(case, R.scatter_emulate(case))
    if case.softmax:   # torch's fp32 softmax within a quarter of r
        y = R.scatter_inputs(case)
        err = (R.layout_index(y, True)["conf"].double() - R.layout_index(y.double(), True)["conf"]).abs()
        assert float(err.max()) <= QUARTER * R.SOFTMAX_R


@pytest.mark.parametrize("case", R.SSH_CASES, ids=R.case_id)
def test_ssh_case_is_benign_in_fp32(case):
    """ssh_graph in float32, and the tile-by-tile evaluation the defects are
    planted in, against fp64 at a quarter of both bars."""
    for defect in (None, "tiled"):
        probs, errs = R.ssh_check(case, R.ssh_emulate(case, defect), QUARTER)
        print(case.name, defect, {g: (f"{a:.3e}", f"{b:.3e}") for g, (a, b) in errs.items()})
        assert not probs, (defect, probs)


@pytest.mark.parametrize("case", R.CSUM_CASES, ids=R.case_id)
def test_csum_case_is_benign_in_fp32(case):
    probs, worst = R.csum_check(case, R.csum_emulate(case), QUARTER)
    assert not probs, probs
    g = R.guarded_flat(case.B * case.nblk, case.C)          # torch's own fp32 sum
    part = g.owed().view(case.B, case.nblk, case.C)
    for i, (p0, p1) in enumerate(R.csum_blocks(case.HW, case.nblk)):
        part[:, i] = R.csum_inputs(case)[:, p0:p1].sum(1)
    probs, worst2 = R.csum_check(case, g, QUARTER)
    print(case.name, worst, worst2)
    assert not probs, probs


def test_planted_layout_defects_are_caught():
    for case in R.HEADS_CASES:
        ref = R.heads_ref(case)

        def caught(defect):
            return R.bar_check(R.heads_emulate(case, defect), ref["ref"], ref["bar"])[0]

        swap = caught("swap_anchors")
        assert any(p.startswith("loc:") for p in swap) and any(p.startswith("landm:") for p in swap), case
        shift = caught("shift_rows")
        for n in ("loc", "conf", "landm"):
            assert any(p.startswith(n) and "written outside" in p for p in shift), (case, n)
            assert any(p.startswith(n) and "unwritten" in p for p in shift), (case, n)
        assert bool(caught("wrong_pair")) == case.softmax, case
        assert not caught(None)
    for case in R.SCATTER_CASES:
        assert any(p.startswith("loc") for p in R.scatter_check(case, R.scatter_emulate(case, "swap_anchors")))
        shift = R.scatter_check(case, R.scatter_emulate(case, "shift_rows"))
        assert any("written outside" in p for p in shift) and any("unwritten" in p for p in shift)
        assert bool(R.scatter_check(case, R.scatter_emulate(case, "wrong_pair"))) == case.softmax, case
    for name in ("hw1", "hw257", "c256-hw300", "saturated-hw300"):
        case = _by_name(R.HEADS_CASES, name)
        assert R.bar_check(R.heads_emulate(case, "swap_anchors"), R.heads_ref(case)["ref"],
                           R.heads_ref(case)["bar"])[0]


@pytest.mark.parametrize("case", R.SSH_CASES, ids=R.case_id)
def test_planted_ssh_defects_are_caught(case):
    tiles = -(-case.H // R.SSH_TH) * -(-case.W // R.SSH_TW)
    for defect in R.SSH_DEFECTS:
        probs, _ = R.ssh_check(case, R.ssh_emulate(case, defect))
        groups = {p.split(":")[0] for p in probs}
        if defect == "halo1" and tiles == 1:
            assert not probs, "one tile: nothing of t lies beyond a 1-pixel halo"
        else:
            assert len(groups) == 3, (defect, probs)    # loc, conf and landm all over a bar
    assert {c.name for c in R.SSH_CASES
            if -(-c.H // R.SSH_TH) * -(-c.W // R.SSH_TW) > 1} == {"9x33", "17x65", "20x20", "1x70", "40x1"}


def test_planted_csum_defects_are_caught():
    drop, floor = set(), set()
    for case in R.CSUM_CASES:
        rows = max(1, R.CSUM_THREADS // case.C) if case.C < R.CSUM_THREADS else 1
        per = -(-case.HW // case.nblk)
        hit = bool(R.csum_check(case, R.csum_emulate(case, "drop_last_group"))[0])
        assert hit == (min(per, case.HW) >= rows), case     # the last group holds a pixel
        if hit:
            drop.add(case.name)
        hit = bool(R.csum_check(case, R.csum_emulate(case, "floor_per"))[0])
        assert hit == (case.HW % case.nblk != 0), case
        if hit:
            floor.add(case.name)
    assert {"c4-hw1000-n3", "c40-hw256-n1", "c100-hw63-n3", "c128-hw63-n3", "c960-hw256-n3"} <= drop
    assert floor == {"c4-hw1000-n3", "c16-hw63-n64", "c72-hw1000-n64", "c200-hw256-n3",
                     "c250-hw1-n64", "c480-hw1-n3", "c960-hw256-n3", "c960-hw63-n64"}


def test_guard_helper_reports_one_row_too_many_and_too_few():
    B, HW, a_off = 2, 5, 6

    def fake(extra):
        gl = R.guarded_level(B, HW, a_off)
        for g in gl.values():
            g.view[:, a_off:a_off + 2 * HW + extra] = 1.0
        return [p for g, n in ((gl[n], n) for n in gl) for p in g.problems(n)]

    assert not fake(0)
    over = fake(1)
    assert len(over) == 3 and all("written outside" in p and f"row {a_off + 2 * HW}" in p for p in over), over
    under = fake(-1)
    assert len(under) == 3 and all("unwritten" in p and f"row {a_off + 2 * HW - 1}" in p for p in under), under
    g = R.guarded_flat(7, 32)                   # in front of the first row
    g.rows[R.GUARD_ROWS - 1, 31] = 0.0
    g.owed()[:] = 1.0
    assert any("written outside" in p for p in g.problems("flat"))


# --------------------------------------------------------------------- GPU tests
def _report(name, worst):
    print(name, " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.HEADS_CASES, ids=R.case_id)
def test_heads_parity(cuda, case):
    from jabd_amd import functional as F
    from jabd_amd._lib import call
    x, W, b = R.heads_inputs(case)
    Wd, bd = W.to(cuda), b.to(cuda)
    gl = R.guarded_level(case.B, case.HW, case.a_off, cuda)
    loc, conf, landm = gl["loc"].view, gl["conf"].view, gl["landm"].view
    if case.kind == "view":
        buf, (off, x_bs, x_ps) = R.heads_view_buffer(case, x)
        buf = buf.to(cuda)
        call("jabd_heads_f32", buf.data_ptr() + 4 * off, x_bs, x_ps, case.B, case.HW, case.C,
             Wd.data_ptr(), bd.data_ptr(), loc.shape[1], case.a_off, int(case.softmax),
             loc.data_ptr(), conf.data_ptr(), landm.data_ptr(), None)
    else:
        xd = x.to(cuda).view(case.B, 1, case.HW, case.C)
        F.heads(xd, Wd, bd, loc, conf, landm, case.a_off, case.softmax)
    torch.cuda.synchronize()
    ref = R.heads_ref(case)
    probs, worst = R.bar_check(gl, ref["ref"], ref["bar"])
    _report("heads " + case.name, worst)
    assert not probs, probs


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.SCATTER_CASES, ids=R.case_id)
def test_heads_scatter_parity(cuda, case):
    from jabd_amd import functional as F
    y = R.scatter_inputs(case).to(cuda).view(case.B, 1, case.HW, 32)
    gl = R.guarded_level(case.B, case.HW, case.a_off, cuda)
    F.heads_scatter(y, gl["loc"].view, gl["conf"].view, gl["landm"].view, case.a_off, case.softmax)
    torch.cuda.synchronize()
    probs = R.scatter_check(case, gl)
    if case.softmax:
        ref = R.layout_index(R.scatter_inputs(case).double(), True)["conf"]
        print("scatter", case.name, "softmax err / r = %.3f" % (
            float((gl["conf"].owed().cpu().double() - ref).abs().max()) / R.SOFTMAX_R))
    assert not probs, probs


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.GATHER_CASES, ids=R.case_id)
def test_heads_gather_is_bit_identical(cuda, case):
    from jabd_amd._lib import call
    gl, gc, glm, want = R.gather_inputs(case)
    gl, gc, glm = gl.to(cuda), gc.to(cuda), glm.to(cuda)
    out = R.guarded_flat(case.B * case.HW, 32, cuda)
    call("jabd_heads_gather_f32", gl.data_ptr(), gc.data_ptr(), glm.data_ptr(), case.B,
         gl.shape[1], case.a_off, case.HW, out.owed().data_ptr(), None)
    torch.cuda.synchronize()
    assert not out.problems("dout")
    got = out.owed().cpu().view(case.B, case.HW, 32)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.SSH_CASES, ids=R.case_id)
def test_ssh_tail_parity(cuda, case):
    from jabd_amd import engine
    from jabd_amd import functional as F
    inp = R.ssh_inputs(case)
    ssh = copy.deepcopy(inp["ssh"]).to(cuda)
    wb = engine.ssh_tail_pack(ssh, (inp["Wh"].to(cuda), inp["bh"].to(cuda)))
    assert wb is not None
    c33 = (R.ssh_c33_buffer(case, inp["c33"]).to(cuda)[..., :20] if case.view
           else inp["c33"].to(cuda))
    assert c33.stride(2) == (32 if case.view else 20)
    gl = R.guarded_level(case.B, case.H * case.W, case.a_off, cuda)
    F.ssh_tail_heads(c33, inp["t"].to(cuda), wb, ssh.leaky, gl["loc"].view, gl["conf"].view,
                     gl["landm"].view, case.a_off, case.softmax)
    torch.cuda.synchronize()
    probs, errs = R.ssh_check(case, gl)
    print("ssh", case.name, " ".join(f"{g}: rel {a:.3e} elem {b:.3e} (bar {R.SSH_ELEM_BAR[g]:.1e})"
                                     for g, (a, b) in errs.items()))
    assert not probs, probs


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.CSUM_CASES, ids=R.case_id)
def test_channel_sum_parity(cuda, case):
    from jabd_amd import functional as F
    from jabd_amd._lib import call
    x = R.csum_inputs(case)
    if case.view:
        xd = R.csum_view_buffer(case, x).to(cuda)
        ptr, x_bs, x_ps = xd.data_ptr() + 4 * R.CSUM_VIEW_OFF, case.HW * R.CSUM_VIEW_PS, R.CSUM_VIEW_PS
    else:
        xd = x.to(cuda)
        ptr, x_bs, x_ps = xd.data_ptr(), case.HW * case.C, case.C
    g = R.guarded_flat(case.B * case.nblk, case.C, cuda)
    call("jabd_channel_sum_f32", ptr, x_bs, x_ps, case.B, case.HW, case.C, case.nblk,
         g.owed().data_ptr(), None)
    torch.cuda.synchronize()
    probs, worst = R.csum_check(case, g)
    print("csum", case.name, f"err/bar={worst:.3f}")
    assert not probs, probs
    got = g.owed().cpu().view(case.B, case.nblk, case.C)
    for i, (p0, p1) in enumerate(R.csum_blocks(case.HW, case.nblk)):
        if p0 == p1:
            assert bool((got[:, i] == 0).all()), f"block {i} past the end is not zero"
    if not case.view:   # the wrapper makes the same call
        part = F.channel_sums(xd.view(case.B, 1, case.HW, case.C), case.nblk)
        assert torch.equal(part.cpu(), got)


REJECT_HW, REJECT_B, REJECT_C = 64, 2, 40
REJECT_A = 2 * REJECT_HW + 2          # rows given to the call; the buffers hold more
# name -> (A, a_off, B, HW): each must be refused
HEADS_REJECT = {"odd-A": (REJECT_A + 1, 0, REJECT_B, REJECT_HW),
                "odd-a_off": (REJECT_A + 2, 1, REJECT_B, REJECT_HW),
                "range-past-A": (2 * REJECT_HW - 2, 0, REJECT_B, REJECT_HW),
                "a_off-past-A": (REJECT_A, 4, REJECT_B, REJECT_HW)}
GATHER_REJECT = dict(HEADS_REJECT, **{"B-zero": (REJECT_A, 0, 0, REJECT_HW),
                                      "B-negative": (REJECT_A, 0, -1, REJECT_HW),
                                      "HW-zero": (REJECT_A, 0, REJECT_B, 0),
                                      "HW-negative": (REJECT_A, 0, REJECT_B, -4)})


def _expect_rejected(args, outs, needle):
    from jabd_amd._lib import call
    before = [o.rows.clone() for o in outs]
    with pytest.raises(RuntimeError) as e:
        call(*args)
    assert needle in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for o, was in zip(outs, before):
        assert torch.equal(o.rows.view(torch.int32), was.view(torch.int32)), "a rejected call wrote"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HEADS_REJECT))
def test_heads_rejects_bad_anchor_ranges(cuda, name):
    """Buffers hold REJECT_B images of 2 HW + 6 + 128 rows and guards around
    them, so even an accepted call would stay inside them."""
    A, a_off, B, HW = HEADS_REJECT[name]
    gl = R.guarded_level(REJECT_B, REJECT_HW, 6, cuda)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(REJECT_B, REJECT_HW, REJECT_C, generator=g).to(cuda)
    W = torch.randn(32, REJECT_C, generator=g).to(cuda)
    b = torch.randn(32, generator=g).to(cuda)
    args = ("jabd_heads_f32", x.data_ptr(), REJECT_HW * REJECT_C, REJECT_C, B, HW, REJECT_C,
            W.data_ptr(), b.data_ptr(), A, a_off, 1, gl["loc"].view.data_ptr(),
            gl["conf"].view.data_ptr(), gl["landm"].view.data_ptr(), None)
    _expect_rejected(args, list(gl.values()), "heads:")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GATHER_REJECT))
def test_heads_gather_rejects_bad_shapes(cuda, name):
    A, a_off, B, HW = GATHER_REJECT[name]
    rows = REJECT_B * (REJECT_A + 8)
    g = torch.Generator().manual_seed(6)
    gl, gc, glm = (torch.randn(rows, k, generator=g).to(cuda) for k in (4, 2, 10))
    out = R.guarded_flat(REJECT_B * REJECT_HW, 32, cuda)
    args = ("jabd_heads_gather_f32", gl.data_ptr(), gc.data_ptr(), glm.data_ptr(), B, A, a_off,
            HW, out.owed().data_ptr(), None)
    _expect_rejected(args, [out], "heads_gather:")
