"""The IoU-family box losses (Iou, Giou, Diou, Ciou) of
nets/retinaface_training_DIOU.py: the paired-rows op (IouLoss,
bbox_overlaps_*) and the fused MultiBoxLoss kinds, against the torch-CPU
restatement in tests/_iou_family_ref.py.

Bars (tests/test_train.py's): scalars 1e-5 relative to the fp32 helper
(relative to max(1, |ref|)); per-row values 1e-5 absolute; gradients relative
Frobenius error < 1e-4 against the fp64 helper.  The fp32 helper itself is
within 1.0e-7 (sums), 1.1e-6 (rows) and 2.7e-7 (gradients) of fp64 on these
inputs, so the bars leave the device's expf/atanf/division about 10x."""
import functools

import pytest
import torch

import _iou_family_ref as ref
from oracle import box_ref

KINDS = ref.KINDS
VAR = [0.1, 0.2]
CFG = {"min_sizes": [[16, 32], [64, 128], [256, 512]], "steps": [8, 16, 32], "clip": False}

# name -> (image size, batch, loc scale, priors, positives from the CPU oracle)
CASES = {"64": (64, 2, 1.0, 168, 66), "256": (256, 4, 1.0, 2688, 546), "64x3": (64, 2, 3.0, 168, 66)}

# corner boxes b1, b2 and the fp64 values in the order Iou, Giou, Diou, Ciou
KATS = {
    "shift": ((0, 0, 2, 2), (1, 1, 3, 3), (1 / 7, -5 / 63, 2 / 63, 2 / 63)),
    "aspect": ((0, 0, 2, 1), (0, 0, 1, 2), (1 / 3, 1 / 12, 13 / 48, 0.237081665)),
    "disjoint": ((0, 0, 1, 1), (2, 0, 3, 1), (0.0, -1 / 3, -2 / 5, -2 / 5)),   # y edges tied
    "far": ((0, 0, .01, 1), (10, 10, 11, 10.01), (0.0, None, None, -1.0)),
    "equal": ((0, 0, 1, 2), (0, 0, 1, 2), (1.0, 1.0, 1.0, float("nan"))),
}
DISJOINT_DIOU_GRAD = (0.04, 0.04, -0.2, -0.04)   # of Σ(1 - val); y entries: the tie rule


def _fro(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return float((got - want).norm() / want.norm().clamp_min(1e-30))


def _close(got, want):
    return abs(float(got) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))


def _kat(name, kind, dtype):
    """(value, raw value, gradient of Σ(1 - value) w.r.t. b1) from the helper."""
    b1 = torch.tensor([KATS[name][0]], dtype=dtype, requires_grad=True)
    b2 = torch.tensor([KATS[name][1]], dtype=dtype)
    val = ref.overlaps(kind, b1, b2)
    (1.0 - val).sum().backward()
    return val.detach()[0], ref.raw_overlaps(kind, b1, b2).detach()[0], b1.grad[0]


# ------------------------------------------------------------------ CPU: the helper
def test_hand_kats_pin_the_helper():
    for name, (_, _, want) in KATS.items():
        for kind, w in zip(KINDS, want):
            val, raw, grad = _kat(name, kind, torch.float64)
            if w is None:
                continue
            if w != w:
                assert bool(torch.isnan(val)) and bool(torch.isnan(grad).all()), (name, kind)
            else:
                assert abs(float(val) - w) <= 1e-9, (name, kind, float(val), w)
    _, _, g = _kat("disjoint", "Diou", torch.float64)
    assert (g - torch.tensor(DISJOINT_DIOU_GRAD, dtype=torch.float64)).abs().max() <= 1e-9
    val, raw, g = _kat("far", "Ciou", torch.float64)
    assert abs(float(raw) - -1.387478807) <= 1e-9
    assert float(val) == -1.0 and float(1.0 - val) == 2.0 and bool((g == 0).all())
    val, _, g = _kat("far", "Iou", torch.float64)
    assert float(val) == 0.0 and bool((g == 0).all())
    for kind in ("Giou", "Diou"):
        val, raw, g = _kat("far", kind, torch.float64)
        assert float(val) == float(raw) > -1.0 and bool((g != 0).all()), kind


def test_argument_validation():
    from nets.retinaface_training_DIOU import (IouLoss, MultiBoxLoss, bbox_overlaps_ciou,
                                                bbox_overlaps_iou)
    for bad in ("diou", "CIoU", "", None):
        with pytest.raises(ValueError, match="Iou, Giou, Diou, Ciou"):
            IouLoss("Center", True, VAR, bad)
        with pytest.raises(ValueError, match="Iou, Giou, Diou, Ciou"):
            MultiBoxLoss(2, 0.35, 7, VAR, True, losstype=bad)
    crit = IouLoss("Center", True, VAR, "Giou")
    crit.loss = "giou"   # set after construction: caught when forward reads it
    with pytest.raises(ValueError, match="Iou, Giou, Diou, Ciou"):
        crit(torch.zeros(2, 4), torch.zeros(2, 4), torch.ones(2, 4))
    for fn in (bbox_overlaps_iou, bbox_overlaps_ciou):
        with pytest.raises(ValueError, match="paired rows"):
            fn(torch.zeros(3, 4), torch.zeros(2, 4))
    with pytest.raises(ValueError, match="first argument"):
        bbox_overlaps_iou(torch.zeros(2, 4), torch.zeros(2, 4, requires_grad=True))
    with pytest.raises(ValueError, match="paired rows"):
        ref.overlaps("Iou", torch.zeros(3, 4), torch.zeros(2, 4))
    with pytest.raises(ValueError, match="losstype"):
        ref.raw_overlaps("diou", torch.zeros(2, 4), torch.ones(2, 4))


# ------------------------------------------------------------------ shared inputs
@functools.lru_cache(maxsize=None)
def _case(name):
    from jabd_amd import synth
    size, B, scale, A, npos = CASES[name]
    pri = box_ref.anchors(CFG, (size, size))
    assert pri.shape[0] == A
    g = torch.Generator().manual_seed(4)
    loc = torch.randn(B, A, 4, generator=g) * scale
    conf = torch.randn(B, A, 2, generator=g) * 2
    landm = torch.randn(B, A, 10, generator=g)
    tg = [torch.from_numpy(t) for t in synth.targets(B, size, seed=11)]
    lt, ct, lmt = box_ref.match_iou_batch(tg, pri)
    assert int((ct != 0).sum()) == npos
    return pri, loc, conf, landm, tg, lt, ct, lmt


@functools.lru_cache(maxsize=None)
def _fused_ref(name, kind, dtype):
    """((loss_l, loss_c, loss_landm), [grad loc, conf, landm] of 2 l + c + lm)."""
    pri, loc, conf, landm, _, lt, ct, lmt = _case(name)
    leaves = [t.clone().to(dtype).requires_grad_(True) for t in (loc, conf, landm)]
    out = ref.multibox_loss(kind, *leaves, lt.to(dtype), ct, lmt.to(dtype), pri, VAR,
                            check_regular=(name == "64x3"))
    (2.0 * out[0] + out[1] + out[2]).backward()
    return [o.detach() for o in out[:3]], [t.grad for t in leaves]


def _fused_hip(name, kind, cuda, set_after=False):
    from nets.retinaface_training_DIOU import MultiBoxLoss
    pri, loc, conf, landm, tg = _case(name)[:5]
    if set_after:
        crit = MultiBoxLoss(2, 0.35, 7, VAR, True)
        crit.gious.loss = kind
    else:
        crit = MultiBoxLoss(2, 0.35, 7, VAR, True, losstype=kind)
    gl = [t.to(cuda).requires_grad_(True) for t in (loc, conf, landm)]
    l, c, lm = crit(tuple(gl), pri.to(cuda), [t.to(cuda) for t in tg])
    (2.0 * l + c + lm).backward()
    return [l.detach(), c.detach(), lm.detach()], [t.grad for t in gl]


@functools.lru_cache(maxsize=None)
def _rows_inputs(mode, P):
    """(pred, truth, priors or None), fp32 CPU.  Center: the small fused case's
    positives, repeated with seeded offsets on the loc beyond its 66 rows.
    Corner: seeded corner boxes, the truth a jittered copy (about a fifth of
    the pairs disjoint)."""
    g = torch.Generator().manual_seed(100 + P)
    if mode == "Center":
        pri, loc, _, _, _, lt, ct, _ = _case("64")
        lp, tr, pp = ref.positives(loc, lt, ct, pri)
        idx = torch.arange(P) % lp.shape[0]
        jit = 0.5 * torch.randn(P, 4, generator=g) * (torch.arange(P) >= lp.shape[0]).view(-1, 1)
        return (lp[idx] + jit).contiguous(), tr[idx].contiguous(), pp[idx].contiguous()
    xy = torch.rand(P, 2, generator=g) * 0.7
    wh = 0.02 + 0.28 * torch.rand(P, 2, generator=g)
    b1 = torch.cat((xy, xy + wh), 1)
    xy2 = xy + 0.25 * (torch.rand(P, 2, generator=g) - 0.5)
    wh2 = wh * (0.5 + torch.rand(P, 2, generator=g))
    return b1.contiguous(), torch.cat((xy2, xy2 + wh2), 1).contiguous(), None


def _rows_ref(kind, mode, P, dtype, size_sum=True):
    pred, truth, pri = _rows_inputs(mode, P)
    p = pred.clone().to(dtype).requires_grad_(True)
    pr = None if pri is None else pri.to(dtype)
    b = ref.decode(p, pr, VAR) if mode == "Center" else p
    val = ref.overlaps(kind, b, truth.to(dtype))
    loss = ref.iou_loss(kind, p, truth.to(dtype), pr, VAR, pred_mode=mode, size_sum=size_sum)
    loss.backward()
    return val.detach(), loss.detach(), p.grad


def _rows_hip(kind, mode, P, cuda, size_sum=True):
    from nets.retinaface_training_DIOU import IouLoss
    pred, truth, pri = _rows_inputs(mode, P)
    p = pred.to(cuda).requires_grad_(True)
    crit = IouLoss(mode, size_sum, VAR, kind)
    loss = crit(p, truth.to(cuda), None if pri is None else pri.to(cuda))
    loss.backward()
    return loss.detach(), p.grad


# ------------------------------------------------------------------ GPU: the rows op
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["Center", "Corner"])
@pytest.mark.parametrize("kind", KINDS)
def test_rows_op_parity(cuda, kind, mode):
    """Per-row values, Σ(1 - val) and the gradient at the wave edges, through
    IouLoss and the bbox_overlaps_* functions."""
    import nets.retinaface_training_DIOU as mod
    from jabd_amd import ops
    fn = getattr(mod, "bbox_overlaps_" + kind.lower())
    for P in (1, 63, 64, 65, 1000):
        pred, truth, pri = _rows_inputs(mode, P)
        v32, l32, _ = _rows_ref(kind, mode, P, torch.float32)
        _, _, g64 = _rows_ref(kind, mode, P, torch.float64)
        if mode == "Center":
            val = ops.iou_rows(pred.to(cuda), truth.to(cuda), kind, pri.to(cuda), VAR)
        else:
            val = fn(pred.to(cuda), truth.to(cuda))
        assert val.shape == (P,) and val.is_cuda
        err = float((val.cpu() - v32).abs().max())
        assert err <= 1e-5, (P, err)
        loss, grad = _rows_hip(kind, mode, P, cuda)
        assert loss.dim() == 0 and _close(loss, l32), (P, float(loss), float(l32))
        assert _fro(grad, g64) < 1e-4, (P, _fro(grad, g64))
    # size_sum=False divides by P; the overlap functions carry autograd to bboxes1
    loss, grad = _rows_hip(kind, mode, 65, cuda, size_sum=False)
    _, l32, _ = _rows_ref(kind, mode, 65, torch.float32, size_sum=False)
    _, _, g64 = _rows_ref(kind, mode, 65, torch.float64, size_sum=False)
    assert _close(loss, l32) and _fro(grad, g64) < 1e-4
    if mode == "Corner":
        pred, truth, _ = _rows_inputs(mode, 65)
        b1 = pred.to(cuda).requires_grad_(True)
        (1.0 - fn(b1, truth.to(cuda))).sum().backward()
        _, _, g64 = _rows_ref(kind, mode, 65, torch.float64)
        assert _fro(b1.grad, g64) < 1e-4


@pytest.mark.gpu
def test_rows_op_empty_launches_nothing(cuda):
    from jabd_amd import _lib, ops
    from nets.retinaface_training_DIOU import IouLoss
    e = torch.empty(0, 4, device=cuda)
    _lib.launch_log_reset()
    for kind in KINDS:
        assert ops.iou_rows(e, e, kind, e, VAR).shape == (0,)
        assert ops.iou_rows_backward(e, e, kind, torch.empty(0, device=cuda)).shape == (0, 4)
        p = e.clone().requires_grad_(True)
        loss = IouLoss("Center", True, VAR, kind)(p, e, e)
        assert loss.dim() == 0 and float(loss.detach()) == 0.0
    assert int(_lib.lib().jabd_launch_log_count()) == 0


@pytest.mark.gpu
def test_rows_op_hand_kats_on_device(cuda):
    """The CPU KAT rows as corner boxes on the device: the same exact zeros,
    the same -1 clamp with a zero gradient, the same NaN, the same tie-halved
    gradient."""
    import nets.retinaface_training_DIOU as mod
    names = list(KATS)
    b1 = torch.tensor([KATS[n][0] for n in names], dtype=torch.float32)
    b2 = torch.tensor([KATS[n][1] for n in names], dtype=torch.float32)
    got = {}
    for kind in KINDS:
        p = b1.to(cuda).requires_grad_(True)
        val = getattr(mod, "bbox_overlaps_" + kind.lower())(p, b2.to(cuda))
        (1.0 - val).sum().backward()
        got[kind] = (val.detach().cpu(), p.grad.cpu())
        want_v = torch.stack([_kat(n, kind, torch.float32)[0] for n in names])
        want_g = torch.stack([_kat(n, kind, torch.float64)[2] for n in names])
        assert torch.allclose(got[kind][0], want_v, rtol=0, atol=1e-5, equal_nan=True), kind
        assert torch.allclose(got[kind][1].double(), want_g, rtol=0, atol=1e-5,
                              equal_nan=True), kind
    i = {n: k for k, n in enumerate(names)}
    for n in ("disjoint", "far"):
        v, g = got["Iou"]
        assert float(v[i[n]]) == 0.0 and bool((g[i[n]] == 0).all()), n
    v, g = got["Ciou"]
    assert float(v[i["far"]]) == -1.0 and bool((g[i["far"]] == 0).all())
    assert bool(torch.isnan(v[i["equal"]])) and bool(torch.isnan(g[i["equal"]]).all())
    for kind in ("Giou", "Diou"):
        v, g = got[kind]
        assert float(v[i["far"]]) > -1.0 and bool((g[i["far"]] != 0).all()), kind
    tie = got["Diou"][1][i["disjoint"]].double() - torch.tensor(DISJOINT_DIOU_GRAD).double()
    assert float(tie.abs().max()) <= 1e-6, got["Diou"][1][i["disjoint"]]
    for kind in ("Iou", "Giou", "Diou"):
        assert float(got[kind][0][i["equal"]]) == 1.0, kind


@pytest.mark.gpu
def test_rows_op_is_deterministic(cuda):
    for kind in KINDS:
        a = _rows_hip(kind, "Center", 1000, cuda)
        b = _rows_hip(kind, "Center", 1000, cuda)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), kind


# ------------------------------------------------------------------ GPU: the fused loss
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("kind", KINDS)
def test_fused_loss_parity(cuda, kind, name):
    """test_multibox_diou_loss_parity's recipe for each kind: 64² is one block
    with a tail, 256² many blocks, 64² with loc x3 has positives whose
    intersection is empty (and none clamped at -1 or NaN: the helper asserts)."""
    if name == "64x3":
        pri, loc, _, _, _, lt, ct, _ = _case(name)
        lp, tr, pp = ref.positives(loc, lt, ct, pri)
        b = ref.decode(lp, pp, VAR)
        empty = ((torch.min(b[:, 2:], tr[:, 2:]) - torch.max(b[:, :2], tr[:, :2])) <= 0).any(1)
        assert 5 <= int(empty.sum()) <= 23, int(empty.sum())
    l32, _ = _fused_ref(name, kind, torch.float32)
    _, g64 = _fused_ref(name, kind, torch.float64)
    losses, grads = _fused_hip(name, kind, cuda)
    for got, want in zip(losses, l32):
        assert _close(got, want), (float(got), float(want))
    assert float(losses[0]) > 0.0
    for got, want in zip(grads, g64):
        assert _fro(got, want) < 1e-4, _fro(got, want)


@pytest.mark.gpu
def test_kind_selection(cuda):
    from jabd_amd import ops
    res = {k: _fused_hip("256", k, cuda) for k in KINDS}
    for k in KINDS:   # the constructor argument and the reference's attribute idiom agree
        late = _fused_hip("256", k, cuda, set_after=True)
        for a, b in zip(res[k][0] + res[k][1], late[0] + late[1]):
            assert torch.equal(a, b), k
    assert len({float(res[k][0][0]) for k in KINDS}) == 4, [float(res[k][0][0]) for k in KINDS]
    for k in KINDS[1:]:   # the CE and landmark terms do not depend on the kind
        assert torch.equal(res[k][0][1], res["Iou"][0][1])
        assert torch.equal(res[k][0][2], res["Iou"][0][2])
    # 'Diou' through the new route == the old diou=(priors, variances) form
    pri, loc, conf, landm, tg = _case("256")[:5]
    d = [t.to(cuda).contiguous() for t in (loc, conf, landm)]
    old = (pri.to(cuda), tuple(VAR))
    lt, ct, lmt = ops.match_encode([t.to(cuda) for t in tg], old[0], 0.35, VAR, raw_loc=True)
    sums, counts, sel = ops.multibox_sums(*d, lt, ct, lmt, 7, old)
    loss = ops.multibox_normalize(sums, counts)
    gout = torch.tensor([2.0, 1.0, 1.0], device=cuda)
    grads = ops.multibox_backward(*d, lt, ct, lmt, sel, gout, counts, old)
    for a, b in zip(list(loss) + list(grads), res["Diou"][0] + res["Diou"][1]):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_launch_count_is_the_same_for_every_kind(cuda):
    """One forward + backward of the fused criterion: the launch witness
    (every libjabd launch is logged) counts the same for each kind."""
    from jabd_amd import _lib
    counts = {}
    for k in KINDS:
        _lib.launch_log_reset()
        _fused_hip("64", k, cuda)
        counts[k] = int(_lib.lib().jabd_launch_log_count())
    assert counts["Iou"] > 0 and len(set(counts.values())) == 1, counts
