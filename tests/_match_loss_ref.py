"""Shared helpers of the match/encode and MultiBoxLoss parity tests
(test_loss_size.py, test_match_loss_edges.py): fixtures, the oracle's side
(oracle/box_ref.py) and the device-vs-oracle comparisons with their bars.

Bars, as test_loss_size.py states them: conf_t and landm_t bit-exact; loc_t
1e-5 for the encoded form (the log() ulp) and bit-exact for the raw corners;
the three losses 1e-5 relative; the OHEM-selected set equal to the oracle's,
or equal except for rows whose mining loss lies within 4 ulp of the image's
selection threshold (at most 2 per image, set sizes equal); gradients
rel_err < 1e-5.
"""
import ctypes
import functools

import numpy as np
import torch

from _util import rel_err
from oracle import box_ref

CFG_MNET = {"min_sizes": [[16, 32], [64, 128], [256, 512]], "steps": [8, 16, 32],
            "variance": [0.1, 0.2], "clip": False}
VAR = (0.1, 0.2)
MAX_GT = 3276   # csrc/box_ops.hip match_impl: max_gt * 5 floats of LDS


@functools.lru_cache(maxsize=None)
def priors(size):
    """CFG_MNET anchors of a size x size image: 32 -> 42, 64 -> 168, 128 -> 672."""
    return box_ref.anchors(CFG_MNET, (size, size))


def synth_targets(B, size, seed, **kw):
    from jabd_amd import synth
    return [torch.from_numpy(t) for t in synth.targets(B, size, seed=seed, **kw)]


# ----------------------------------------------------------------------------- match
def corner_truth(size, k, m, label=1.0):
    """A 16-px truth centred on the corner (8k, 8m) shared by four level-0
    cells: their four 16-px priors overlap it equally (every number is dyadic,
    so the four IoUs are the same fp32 value)."""
    h = 8.0 / size
    x, y = 8.0 * k / size, 8.0 * m / size
    row = [x - h, y - h, x + h, y + h]
    for fx, fy in ((.3, .35), (.7, .35), (.5, .55), (.35, .75), (.65, .75)):
        row += [x - h + 2 * h * fx, y - h + 2 * h * fy]
    return torch.tensor(row + [label], dtype=torch.float32)


def tied_priors(truth, pri):
    """(indices of the priors that attain the truth's maximum IoU, the oracle's
    best prior) for one truth row."""
    ov = box_ref.jaccard(truth[None, :4], box_ref.point_form(pri))[0]
    return (ov == ov.max()).nonzero().flatten().tolist(), int(ov.max(0)[1])


def _same_bits(got, ref):
    """Bit-exact where the oracle is a number, NaN where it is NaN (inf == inf)."""
    nan = torch.isnan(ref)
    return torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan], ref[~nan])


def check_match(cuda, tg, pri, threshold=0.35):
    """ops.match_encode, encoded and raw, against the oracle.  Returns the
    oracle's encoded (loc_t, conf_t, landm_t)."""
    from jabd_amd import ops
    d_tg, d_pri = [t.to(cuda) for t in tg], pri.to(cuda)
    out = None
    for raw in (False, True):
        rl, rc, rlm = (box_ref.match_iou_batch if raw else box_ref.match_batch)(
            tg, pri, threshold, VAR)
        gl, gc, glm = (t.cpu() for t in ops.match_encode(d_tg, d_pri, threshold, list(VAR),
                                                         raw_loc=raw))
        assert torch.equal(gc, rc), (raw, (gc != rc).nonzero()[:8].tolist())
        assert _same_bits(glm, rlm), raw
        if raw:
            assert _same_bits(gl, rl)
        else:
            # same NaN mask, same ±inf pattern, 1e-5 on the numbers
            fin = torch.isfinite(rl)
            assert torch.equal(torch.isfinite(gl), fin)
            assert _same_bits(gl[~fin], rl[~fin])
            torch.testing.assert_close(gl[fin], rl[fin], rtol=1e-5, atol=1e-5)
            out = rl, rc, rlm
    return out


def abi_match(cuda, name, tg, pri, threshold=0.35, fill=-7.0):
    """jabd_match_encode_f32 / jabd_match_iou_f32 through the C ABI with the
    images' rows back to back (an empty image is an empty tensor).  The outputs
    are pre-filled with `fill`, so an untouched output shows.  Returns the
    outputs on the CPU and the exception raised, if any."""
    from jabd_amd._lib import call
    B, A = len(tg), pri.shape[0]
    counts = [int(t.shape[0]) for t in tg]
    flat = torch.cat([t.reshape(-1, 15) for t in tg]).contiguous().to(cuda)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64).to(cuda)
    d_pri = pri.to(cuda).contiguous()
    loc_t = torch.full((B, A, 4), fill, dtype=torch.float32, device=cuda)
    conf_t = torch.full((B, A), int(fill), dtype=torch.int64, device=cuda)
    landm_t = torch.full((B, A, 10), fill, dtype=torch.float32, device=cuda)
    sz = ctypes.c_size_t()
    call("jabd_match_workspace_size", B, A, ctypes.byref(sz))
    ws = torch.empty(max(sz.value, 1), dtype=torch.uint8, device=cuda)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    err = None
    try:
        call(name, flat.data_ptr(), offs.data_ptr(), B, max(counts), d_pri.data_ptr(), A,
             float(threshold), VAR[0], VAR[1], loc_t.data_ptr(), conf_t.data_ptr(),
             landm_t.data_ptr(), ws.data_ptr(), sz.value, st)
    except RuntimeError as e:
        err = e
    torch.cuda.synchronize()
    return (loc_t.cpu(), conf_t.cpu(), landm_t.cpu()), err


# ----------------------------------------------------------------------------- loss
def _ulp_band(v, k=4):
    return k * np.spacing(np.float32(abs(v)) if v != 0 else np.float32(1e-38))


def _preds(B, A, seed, quant=None):
    g = torch.Generator().manual_seed(seed)
    loc = torch.randn(B, A, 4, generator=g)
    conf = torch.randn(B, A, 2, generator=g) * 2
    landm = torch.randn(B, A, 10, generator=g)
    if quant:
        # background logit 0 and the face logit on a 1/quant grid: equal
        # mining losses then come from equal (c0, c1) pairs only, so they are
        # equal in any exp/log implementation (pairs with the same c1 - c0 but
        # different c0 are equal in exact arithmetic, not in fp32)
        conf[..., 0] = 0.0
        conf[..., 1] = torch.round(conf[..., 1] * quant) / quant
    return loc, conf, landm


def direct_targets(conf_t, seed, raw=False):
    """Matched targets around a conf_t that the case sets itself: loc_t is
    N(0, 1) offsets, or (raw) finite truth corners for the IoU-family box
    term; landm_t is N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    B, A = conf_t.shape
    if raw:
        xy = torch.rand(B, A, 2, generator=g) * 0.6
        wh = 0.05 + torch.rand(B, A, 2, generator=g) * 0.35
        loc_t = torch.cat([xy, xy + wh], 2)
    else:
        loc_t = torch.randn(B, A, 4, generator=g)
    return loc_t, conf_t.clone(), torch.randn(B, A, 10, generator=g)


def loss_given_sel(loc, conf, landm, loc_t, conf_t, landm_t, sel, diou=None):
    """The three normalised losses (nets/retinaface_training.py:219-303) for a
    given selection `sel`, in the dtype of `loc`: oracle/box_ref.py's terms
    without the mining, so an fp64 run keeps the fp32 run's selected set."""
    pos1, pos = conf_t > 0, conf_t != 0
    s_landm = box_ref.smooth_l1_sum(landm[pos1].view(-1, 10), landm_t[pos1].view(-1, 10))
    if diou is None:
        s_loc = box_ref.smooth_l1_sum(loc[pos].view(-1, 4), loc_t[pos].view(-1, 4))
    else:
        pri_b = diou[0].to(loc.dtype).unsqueeze(0).expand_as(loc)
        s_loc = box_ref.diou_loss_sum(loc[pos].view(-1, 4), loc_t[pos].view(-1, 4),
                                      pri_b[pos].view(-1, 4), diou[1])
    s_c = torch.nn.functional.cross_entropy(conf[sel].view(-1, 2), pos.long()[sel],
                                            reduction="sum")
    n = max(float(pos.sum()), 1.0)
    n1 = max(float(pos1.sum()), 1.0)
    return s_loc / n, s_c / n, s_landm / n1


def oracle_threshold_spread(loc, conf, landm, lt, ct, lmt, neg_pos=7, diou=None):
    """CPU: rows on which the fp32 oracle's selection differs from its own fp64
    run — the rows a device may legitimately differ on."""
    s32 = box_ref.multibox_loss(loc, conf, landm, lt, ct, lmt, neg_pos, diou=diou)[3]["sel"]
    s64 = box_ref.multibox_loss(loc.double(), conf.double(), landm.double(), lt.double(), ct,
                                lmt.double(), neg_pos, diou=diou)[3]["sel"]
    return (s32 ^ s64).sum(1)


def _close(got, ref):
    got, ref = float(got), float(ref)
    return abs(got - ref) <= 1e-5 * max(1.0, abs(ref))


def _check_loss(cuda, pri, tg, loc, conf, landm, lt, ct, lmt, exact_sel=False, neg_pos=7,
                kind=None, nan_c=False):
    """Values, OHEM selection and gradients of the device loss vs the oracle.
    Returns (rows differing near the threshold, exact ties at the threshold).

    tg: the images' targets — the device matches them itself and the loss runs
    through the MultiBoxLoss module; (lt, ct, lmt) are the oracle's match.
    tg=None: (lt, ct, lmt) are matched targets the case set directly; the
    device takes them as they are, through ops.multibox_sums / _normalize /
    _backward and through the autograd node the modules run.
    kind: None for the smooth-L1 box term, or an IouLoss name ('Diou'), lt then
    holding raw truth corners.  nan_c: the oracle's loss_c is NaN and the
    device's must be; the conf gradient is then compared where it is a number.
    """
    from jabd_amd import ops
    from nets.retinaface_training import MultiBoxLoss, _MultiBoxLossFn
    from nets.retinaface_training_DIOU import MultiBoxLoss as IouMultiBoxLoss
    r_diou = None if kind is None else (pri, list(VAR))
    leaves = [t.clone().requires_grad_(True) for t in (loc, conf, landm)]
    rl, rc, rlm, info = box_ref.multibox_loss(*leaves, lt, ct, lmt, neg_pos, diou=r_diou)
    (2.0 * rl + rc + rlm).backward()

    # the selection the device loss made (bit 4 of sel), from the same call
    # the autograd node runs (ops.multibox_sums)
    d_loc, d_conf, d_landm = (t.to(cuda) for t in (loc, conf, landm))
    d_pri = pri.to(cuda)
    d_diou = None if kind is None else (d_pri, VAR, kind)
    if tg is None:
        d_lt, d_ct, d_lmt = lt.to(cuda), ct.to(cuda), lmt.to(cuda)
    else:
        d_lt, d_ct, d_lmt = ops.match_encode([t.to(cuda) for t in tg], d_pri, 0.35, [0.1, 0.2],
                                             raw_loc=kind is not None)
    sums, counts, sel = ops.multibox_sums(d_loc, d_conf, d_landm, d_lt, d_ct, d_lmt, neg_pos,
                                          d_diou)
    got_sel = (sel.cpu() & 4) != 0
    ref_sel = info["sel"]
    assert tuple(int(c) for c in counts.cpu()) == info["counts"]
    mine = info["mining"].detach()
    near, ties = 0, 0
    for b in range(loc.shape[0]):
        npos = int(info["pos"][b].sum())
        num_neg = min(neg_pos * npos, loc.shape[1] - 1)
        if num_neg == 0:
            assert torch.equal(got_sel[b], ref_sel[b])
            continue
        thr = float(torch.sort(mine[b], descending=True, stable=True)[0][num_neg - 1])
        ties += int((mine[b] == thr).sum()) - 1
        diff = (got_sel[b] ^ ref_sel[b]).nonzero().flatten()
        if len(diff):
            band = _ulp_band(thr)
            assert bool(((mine[b][diff] - thr).abs() <= band).all()), (b, diff[:8])
            assert int(got_sel[b].sum()) == int(ref_sel[b].sum()), b
            near += len(diff)
    print(f"OHEM: {near} rows differ within 4 ulp of a threshold, {ties} exact ties at it")
    if exact_sel:
        assert near == 0
    assert near <= 2 * loc.shape[0], near

    gl = [t.to(cuda).requires_grad_(True) for t in (loc, conf, landm)]
    if tg is None:
        l, c, lm = _MultiBoxLossFn.apply(*gl, d_lt, d_ct, d_lmt, neg_pos, None, d_diou)
    else:
        crit = (MultiBoxLoss(2, 0.35, neg_pos, [0.1, 0.2], True) if kind is None else
                IouMultiBoxLoss(2, 0.35, neg_pos, [0.1, 0.2], True, kind))
        l, c, lm = crit(tuple(gl), pri.to(cuda), [t.to(cuda) for t in tg])
    (2.0 * l + c + lm).backward()
    for got, ref in ((l, rl), (c, rc), (lm, rlm)):
        got, ref = float(got.detach()), float(ref.detach())
        if nan_c and ref != ref:
            assert got != got, got
            continue
        assert abs(got - ref) <= 1e-5 * max(1.0, abs(ref)), (got, ref)
    for g_, r_ in zip(gl, leaves):
        if nan_c:
            ok = ~torch.isnan(r_.grad)
            assert torch.equal(~torch.isnan(g_.grad.cpu()), ok)
            assert rel_err(g_.grad.cpu()[ok], r_.grad[ok]) < 1e-5
            continue
        assert rel_err(g_.grad, r_.grad) < 1e-5

    if tg is None:
        # the ops the node is made of give the node's numbers
        loss = ops.multibox_normalize(sums, counts)
        assert _same_bits(loss.cpu(), torch.stack([l, c, lm]).detach().cpu())
        gout = torch.tensor([2.0, 1.0, 1.0], device=cuda)
        grads = ops.multibox_backward(d_loc, d_conf, d_landm, d_lt, d_ct, d_lmt, sel, gout,
                                      counts, d_diou)
        for g_, a_ in zip(grads, gl):
            assert _same_bits(g_.cpu(), a_.grad.cpu())
        # fp64 values over the set the fp32 oracle selected
        if near == 0:
            r64 = loss_given_sel(loc.double(), conf.double(), landm.double(), lt.double(), ct,
                                 lmt.double(), ref_sel, r_diou)
            for got, ref in zip((l, c, lm), r64):
                if nan_c and float(ref) != float(ref):
                    continue
                assert _close(got.detach(), ref), (float(got), float(ref))
    return near, ties
