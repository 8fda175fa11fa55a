"""Edge-case parity of the match/encode and MultiBoxLoss kernels
(csrc/box_ops.hip: match_best_prior_kernel, match_assign_kernel<kRaw>,
conf_max_partial, loss_elem_kernel<kBox>, ohem_select_kernel,
loss_final_kernel, loss_normalize_kernel, loss_bwd_kernel<kBox>) against the
oracle restatement (oracle/box_ref.py) on inputs built to make the hand-written
rules fire: better()'s tie and NaN order, nan_min/nan_max, fkey_asc, the
num_neg clamp and the max(count, 1) normalisers.  synth.targets and randn, the
other match/loss tests' inputs, almost never reach them.

Match (ops.match_encode, encoded and raw, vs box_ref.match_batch /
match_iou_batch; CFG_MNET anchors: 32² -> 42, 64² -> 168, 128² -> 672):
  M1 four priors tie for a truth — inside one wave, across two waves of one
     stride pass, across two stride passes of the 256-thread loop, and with
     A = 42 < 64; the lowest index must win (run at 0.35 and at 0.5, where
     the forced prior alone stays positive); and a truth outside the image,
     which ties every prior, those of one thread's stride loop included.
  M2 A below a workgroup and below a wave.
  M3 NaN, zero-area and inverted truths: NaN beats numbers, the first NaN wins.
  M4 the threshold set on a realised overlap and one ulp above it (`<` is strict,
     so the kernel's IoU has to be torch's, bit for bit).
  M5 3276 truths in one image (the accepted cap, 65,520 bytes of LDS) and 3277.
  M6 an empty image between non-empty ones through the C ABI: zeros, and the
     neighbours untouched by it.
Loss (ops.multibox_sums / _normalize / _backward and the autograd node of the
MultiBoxLoss modules, smooth-L1 and DIoU box terms, vs box_ref.multibox_loss;
A = 168 with conf_t set directly unless stated):
  L1 images and a whole batch without positives.
  L2 7 npos > A - 1: the clamp, made visible by a non-positive row that ranks last.
  L3 one +120 logit: every other mining loss is -inf.
  L4 a NaN logit: every non-positive mining loss is NaN.
  L5 B = 65 > loss_final_kernel's stride of 64.
  L6 neg_pos 0, 1 and 1000.
Bars: those of test_loss_size.py (see _match_loss_ref.py).  Cases on logits of
a 1/4 grid must select the oracle's set exactly; the unquantised ones may
differ on rows within 4 ulp of an image's threshold, at most 2 per image, and
their seeds keep the fp32 oracle within that of its own fp64 run (CPU test).
"""
import numpy as np
import pytest
import torch

import _match_loss_ref as R
from _match_loss_ref import _check_loss, _preds
from oracle import box_ref

NAN = float("nan")
INF = float("inf")


# =============================================================================
# match fixtures
# =============================================================================
# name -> (size, [per image: ([(k, m), ...] corner truths, synth seed or None)])
TIE_CASES = {
    "one_wave": (128, [([(4, 1)], None)]),                 # 6, 8, 38, 40
    "two_waves": (128, [([(8, 4)], None)]),                # 110, 112 | 142, 144
    "two_passes": (128, [([(9, 8)], None)]),               # 240, 242 | 272, 274
    "64": (64, [([(2, 2)], None)]),                        # 18, 20, 34, 36
    "32": (32, [([(2, 2)], None)]),                        # 10, 12, 18, 20; A = 42
    "several": (128, [([(4, 1), (8, 4), (9, 8), (15, 15), (1, 9)], None)]),
    "with_ordinary": (128, [([(9, 8), (4, 1)], None), ([(8, 4)], 6), ([(9, 8)], 8)]),
}
TIE_SETS = {(128, 4, 1): [6, 8, 38, 40], (128, 8, 4): [110, 112, 142, 144],
            (128, 9, 8): [240, 242, 272, 274], (64, 2, 2): [18, 20, 34, 36],
            (32, 2, 2): [10, 12, 18, 20]}
TIE_THRESHOLD = 0.5   # above the tied IoU (0.39): only a forced prior stays positive


def _tie_case(name):
    """The case's targets, after asserting on the oracle that every corner
    truth's maximum IoU is attained by four priors and that the oracle's best
    prior is the lowest of them."""
    size, images = TIE_CASES[name]
    pri = R.priors(size)
    tg = []
    for i, (corners, seed) in enumerate(images):
        rows = [R.corner_truth(size, k, m, label=-1.0 if (k + m) % 3 == 0 else 1.0)
                for k, m in corners]
        for (k, m), row in zip(corners, rows):
            tied, best = R.tied_priors(row, pri)
            assert len(tied) == 4 and best == min(tied), (name, k, m, tied, best)
            if (size, k, m) in TIE_SETS:
                assert tied == TIE_SETS[(size, k, m)]
        if seed is not None:   # ordinary truths around the tied one
            extra = R.synth_targets(1, size, seed)[0]
            rows = list(extra[: len(extra) // 2]) + rows + list(extra[len(extra) // 2:])
        tg.append(torch.stack(rows))
    return pri, tg


def _far_truth_case(size):
    """One truth outside the image: IoU 0 with every prior, an A-way tie that
    also meets inside one thread's stride loop (priors 0, 256, 512)."""
    pri = R.priors(size)
    t = R.corner_truth(size, 2, 2)[None].clone()
    t[:, :14] += 64.0     # beyond the 512-px priors of a 32² image
    tied, best = R.tied_priors(t[0], pri)
    assert len(tied) == pri.shape[0] and best == 0
    return pri, [t]


def _rows(boxes, seed):
    g = torch.Generator().manual_seed(seed)
    b = torch.tensor(boxes, dtype=torch.float32)
    lab = torch.tensor([1.0, -1.0, 1.0, 1.0, -1.0, 1.0][: len(boxes)]).view(-1, 1)
    return torch.cat([b, torch.rand(len(boxes), 10, generator=g), lab], 1)


NONFINITE = {
    # an ordinary truth, a NaN coordinate, zero area, inverted
    "nan_zero_inverted": [[.2, .2, .5, .5], [NAN, .1, .3, .3], [.4, .4, .4, .4],
                          [.6, .6, .5, .5]],
    # two NaN truths, neither last: the first NaN must win every prior
    "two_nans": [[.2, .2, .5, .5], [.1, NAN, .3, .3], [.4, .4, .4, .4],
                 [.55, .1, .9, NAN], [.6, .6, .5, .5]],
}


def _nonfinite_case(name):
    """[the degenerate image, an ordinary image] at 64², after asserting on the
    oracle what the fixture is there for."""
    pri = R.priors(64)
    t = _rows(NONFINITE[name], 1)
    ov = box_ref.jaccard(t[:, :4], box_ref.point_form(pri))
    nan_rows = torch.isnan(ov).all(1).nonzero().flatten().tolist()
    assert nan_rows == [i for i, b in enumerate(NONFINITE[name]) if any(v != v for v in b)]
    best = ov.max(1)[1].tolist()
    assert best[0] == 36 and all(b == 0 for b in best[1:]), best   # NaN and all-zero rows: index 0
    loc, conf, landm, bti, bto = box_ref.match(0.35, t[:, :4], pri, list(R.VAR), t[:, -1],
                                               t[:, 4:14])
    # the first NaN truth owns every prior but the forced ones; NaN < thr is false
    forced = sorted(set(best))
    assert int((bti == nan_rows[0]).sum()) == 168 - len(forced)
    assert bool(torch.isnan(bto[[a for a in range(168) if a not in forced]]).all())
    assert int((conf != 0).sum()) == 168
    assert int((~torch.isfinite(loc)).any(1).sum()) == 167
    return pri, [t, R.synth_targets(1, 64, 9)[0]]


def _threshold_case():
    """64², B = 3: eight realised best-truth overlaps in (0.05, 1) as thresholds."""
    pri = R.priors(64)
    tg = R.synth_targets(3, 64, 5)
    bto = torch.stack([box_ref.match(0.35, t[:, :4], pri, list(R.VAR), t[:, -1], t[:, 4:14])[4]
                       for t in tg])
    v = torch.unique(bto)
    v = v[(v > 0.05) & (v < 1.0)]
    assert len(v) >= 64
    picks = [float(x) for x in v[:: len(v) // 8][:8]]
    assert len(set(picks)) == 8
    return pri, tg, bto, picks


def _cap_targets(n):
    """synth.targets rows repeated to n rows, and a small second image."""
    base = R.synth_targets(1, 64, 12)[0]
    assert 1 < base.shape[0] < n
    big = base.repeat((n + base.shape[0] - 1) // base.shape[0], 1)[:n].contiguous()
    return [big, R.synth_targets(1, 64, 13)[0]]


# =============================================================================
# loss fixtures
# =============================================================================
def _l1_conf_t(A=168):
    """Image 0 without positives; image 1 with 30 (7 * 30 > A - 1); image 2
    with {5: +1, 70: -1, 130: +1}."""
    ct = torch.zeros(3, A, dtype=torch.int64)
    idx = torch.randperm(A, generator=torch.Generator().manual_seed(3))[:30]
    ct[1, idx] = 1
    ct[1, idx[::4]] = -1
    ct[2, 5], ct[2, 70], ct[2, 130] = 1, -1, 1
    return ct


def _l1_inputs(kind, quant=4, conf_t=None, seed=31):
    """(pri, loc, conf, landm, loc_t, conf_t, landm_t) of L1 at A = 168."""
    ct = _l1_conf_t() if conf_t is None else conf_t
    pri = R.priors({42: 32, 168: 64, 672: 128}[ct.shape[1]])
    loc, conf, landm = _preds(ct.shape[0], ct.shape[1], seed, quant=quant)
    return (pri, loc, conf, landm) + R.direct_targets(ct, 7, raw=kind is not None)


def _oracle(inp, kind, neg_pos=7):
    pri, loc, conf, landm, lt, ct, lmt = inp
    return box_ref.multibox_loss(loc, conf, landm, lt, ct, lmt, neg_pos,
                                 diou=None if kind is None else (pri, list(R.VAR)))


def _l2_conf_t():
    """A = 42: image 0 has 7 positives (49 > 41), image 1 one (7 negatives)."""
    ct = torch.zeros(2, 42, dtype=torch.int64)
    ct[0, [1, 4, 9, 16, 25, 36, 40]] = torch.tensor([1, 1, -1, 1, 1, -1, 1])
    ct[1, 20] = 1
    return ct


def _l5_conf_t(B=65, A=42):
    """Every fifth image without positives, the others with one to three."""
    rng = np.random.default_rng(65)
    ct = torch.zeros(B, A, dtype=torch.int64)
    for b in range(B):
        if b % 5 == 0:
            continue
        for a in rng.choice(A, 1 + b % 3, replace=False):
            ct[b, int(a)] = 1 if rng.uniform() < 0.7 else -1
    assert int((ct[64] != 0).sum()) > 0 and int((ct[0] != 0).sum()) == 0
    return ct


def _run(cuda, inp, kind, **kw):
    pri, loc, conf, landm, lt, ct, lmt = inp
    return _check_loss(cuda, pri, None, loc, conf, landm, lt, ct, lmt, kind=kind, **kw)


KINDS = [None, "Diou"]
UNQUANT = {"L1": 31, "L5": 32}   # seeds of the unquantised cases (CPU-checked below)


# =============================================================================
# CPU: the fixtures are what they claim to be, on the oracle
# =============================================================================
@pytest.mark.parametrize("name", list(TIE_CASES))
def test_tie_fixture_oracle(name):
    pri, tg = _tie_case(name)
    assert pri.shape[0] == {128: 672, 64: 168, 32: 42}[TIE_CASES[name][0]]
    # in the oracle's match the tied truth is forced onto its lowest tied prior
    for t in tg:
        _, _, _, bti, bto = box_ref.match(0.35, t[:, :4], pri, list(R.VAR), t[:, -1], t[:, 4:14])
        for j in range(t.shape[0]):
            tied, best = R.tied_priors(t[j], pri)
            if len(tied) == 4:
                assert float(bto[best]) == 2.0
                assert not any(float(bto[a]) == 2.0 and int(bti[a]) == j for a in tied[1:])
                assert float(box_ref.jaccard(t[j:j + 1, :4], box_ref.point_form(pri)).max()) \
                    < TIE_THRESHOLD
        if t.shape[0] == 1:   # above the tied IoU the winner alone is positive
            ct = box_ref.match_batch([t], pri, TIE_THRESHOLD, R.VAR)[1][0]
            assert ct.nonzero().flatten().tolist() == [R.tied_priors(t[0], pri)[1]]


@pytest.mark.parametrize("size", [32, 128])
def test_far_truth_fixture_oracle(size):
    pri, tg = _far_truth_case(size)
    assert box_ref.match_batch(tg, pri)[1][0].nonzero().flatten().tolist() == [0]


@pytest.mark.parametrize("name", list(NONFINITE))
def test_nonfinite_fixture_oracle(name):
    _nonfinite_case(name)


def test_threshold_fixture_oracle():
    pri, tg, bto, picks = _threshold_case()
    for thr in picks:
        up = float(np.nextafter(np.float32(thr), np.float32(2)))
        assert int((bto == thr).sum()) >= 1
        a = box_ref.match_batch(tg, pri, thr, R.VAR)[1]
        b = box_ref.match_batch(tg, pri, up, R.VAR)[1]
        assert not torch.equal(a, b)
        assert bool((a[bto == thr] != 0).all()) and bool((b[bto == thr] == 0).all())


def test_loss_fixtures_oracle():
    """The clamp, the -inf and the NaN fixtures on the oracle."""
    inp = _l1_inputs(None)
    info = _oracle(inp, None)[3]
    npos = info["pos"].sum(1).tolist()
    assert npos == [0, 30, 3] and min(7 * npos[1], 167) == 167
    assert info["sel"].sum(1).tolist() == [0, 168, 24]
    # L3: one +120 logit
    pri, loc, conf, landm, lt, ct, lmt = inp
    c3 = conf.clone()
    c3[2, 150, 1] = 120.0
    info = box_ref.multibox_loss(loc, c3, landm, lt, ct, lmt)[3]
    m = info["mining"].clone()
    assert float(m[2, 150]) == 120.0
    m[2, 150] = -INF
    assert bool((m[~info["pos"]] == -INF).all())
    assert info["sel"].sum(1).tolist() == [0, 167, 21]
    assert info["sel"][2].nonzero().flatten().tolist() == \
        [a for a in range(18)] + [70, 130, 150]
    # L4: a NaN logit in a row the oracle does not select / selects
    for row, col, selected in ((160, 0, False), (2, 1, True)):
        c4 = conf.clone()
        c4[2, row, col] = NAN
        out = box_ref.multibox_loss(loc, c4, landm, lt, ct, lmt)
        assert bool(torch.isnan(out[3]["mining"][~out[3]["pos"]]).all())
        assert out[3]["sel"].sum(1).tolist() == [0, 168, 24]
        assert bool(out[3]["sel"][2, row]) == selected
        assert bool(torch.isnan(out[1])) == selected
        assert bool(torch.isfinite(out[0])) and bool(torch.isfinite(out[2]))


def test_clamp_fixture_oracle():
    """L2: with 7 npos > A - 1 the oracle leaves out exactly the row that ranks
    last, and that row is a non-positive (so the clamp shows)."""
    for variant in ("plain", "outlier"):
        inp = _l2_inputs(None, variant)
        info = _oracle(inp, None)[3]
        npos = info["pos"].sum(1).tolist()
        assert npos == [7, 1] and min(7 * npos[0], 41) == 41 < 7 * npos[0]
        want = {"plain": [42, 8], "outlier": [41, 7]}[variant]
        assert info["sel"].sum(1).tolist() == want
        if variant != "plain":
            assert not bool(info["sel"][0, 41]) and not bool(info["pos"][0, 41])


def test_unquantised_seeds_oracle():
    """The unquantised cases' seeds: the fp32 oracle and its own fp64 run
    differ on at most 2 rows per image."""
    for kind in KINDS:
        for inp in (_l1_inputs(kind, quant=None, seed=UNQUANT["L1"]),
                    _l1_inputs(kind, quant=None, conf_t=_l5_conf_t(), seed=UNQUANT["L5"])):
            pri, loc, conf, landm, lt, ct, lmt = inp
            d = None if kind is None else (pri, list(R.VAR))
            spread = R.oracle_threshold_spread(loc, conf, landm, lt, ct, lmt, 7, d)
            assert int(spread.max()) <= 2, spread.tolist()


def test_neg_pos_fixture_oracle():
    inp = _l1_inputs(None)
    info = _oracle(inp, None, 0)[3]
    assert torch.equal(info["sel"], info["pos"])
    assert _oracle(inp, None, 1)[3]["sel"].sum(1).tolist() == [0, 60, 6]
    assert _oracle(inp, None, 1000)[3]["sel"].sum(1).tolist() == [0, 168, 168]


def _l2_inputs(kind, variant):
    """plain: positives rank last, so every row is selected with or without the
    clamp.  outlier: a +120 logit makes every other mining loss -inf; the
    positives' 0 then ranks above them and the clamp leaves out the last row."""
    inp = list(_l1_inputs(kind, conf_t=_l2_conf_t(), seed=33))
    conf = inp[2]
    if variant == "outlier":
        conf[1, 30, 1] = 120.0
    return tuple(inp)


# =============================================================================
# GPU: match
# =============================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TIE_CASES))
def test_m1_prior_ties(cuda, name):
    """At the training threshold all four tied priors (IoU 144/368 = 0.39) are
    positive whichever of them is forced, and with one truth in the image they
    all encode that truth: the forced prior would not show.  At 0.5 only the
    forced prior stays positive, so conf_t names the winner."""
    pri, tg = _tie_case(name)
    R.check_match(cuda, tg, pri)
    _, ct, _ = R.check_match(cuda, tg, pri, TIE_THRESHOLD)
    for t, c in zip(tg, ct):
        if t.shape[0] == 1:
            assert c.nonzero().flatten().tolist() == [R.tied_priors(t[0], pri)[1]]


@pytest.mark.gpu
@pytest.mark.parametrize("size", [32, 128])
def test_m1_every_prior_ties(cuda, size):
    pri, tg = _far_truth_case(size)
    _, ct, _ = R.check_match(cuda, tg, pri)
    assert ct[0].nonzero().flatten().tolist() == [0]     # the forced prior alone


@pytest.mark.gpu
@pytest.mark.parametrize("size", [32, 64])
@pytest.mark.parametrize("B,seed", [(1, 1), (3, 2), (5, 3)])
def test_m2_small_a(cuda, size, B, seed):
    tg = R.synth_targets(B, size, seed)
    if B == 1:
        tg = [tg[0][:1]]       # one truth, one image
    assert R.priors(size).shape[0] == {32: 42, 64: 168}[size]
    _, ct, _ = R.check_match(cuda, tg, R.priors(size))
    assert int((ct != 0).sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NONFINITE))
def test_m3_nonfinite_truths(cuda, name):
    pri, tg = _nonfinite_case(name)
    lt, ct, lmt = R.check_match(cuda, tg, pri)
    assert int(torch.isnan(lt[0]).sum()) > 0 and bool(torch.isfinite(lt[1]).all())


@pytest.mark.gpu
def test_m4_threshold_on_realised_overlap(cuda):
    from jabd_amd import ops
    pri, tg, bto, picks = _threshold_case()
    d_tg, d_pri = [t.to(cuda) for t in tg], pri.to(cuda)
    for thr in picks:
        up = float(np.nextafter(np.float32(thr), np.float32(2)))
        got = []
        for v in (thr, up):
            want = box_ref.match_batch(tg, pri, v, R.VAR)[1]
            for raw in (False, True):
                gc = ops.match_encode(d_tg, d_pri, v, list(R.VAR), raw_loc=raw)[1].cpu()
                assert torch.equal(gc, want), (v, raw, (gc != want).nonzero()[:8].tolist())
            got.append(want)
        assert int((bto == thr).sum()) >= 1 and not torch.equal(got[0], got[1])


@pytest.mark.gpu
def test_m5_max_gt_cap(cuda):
    pri = R.priors(64)
    tg = _cap_targets(R.MAX_GT)
    assert tg[0].shape[0] == 3276
    R.check_match(cuda, tg, pri)
    for name in ("jabd_match_encode_f32", "jabd_match_iou_f32"):
        out, err = R.abi_match(cuda, name, _cap_targets(R.MAX_GT + 1), pri)
        assert isinstance(err, RuntimeError) and "3276" in str(err), err
        assert all(bool((t == -7).all()) for t in out)    # nothing was written


@pytest.mark.gpu
def test_m6_empty_image_between_others(cuda):
    """offsets [0, n0, n0, n0 + n2] through the C ABI: the empty image is all
    background with zero targets (include/jabd.h), its neighbours are matched
    as if it were not there; ops.match_encode still refuses the list."""
    from jabd_amd import ops
    pri = R.priors(64)
    t0, t2 = R.synth_targets(2, 64, 21)
    tg = [t0, torch.empty(0, 15), t2]
    for name, ref in (("jabd_match_encode_f32", box_ref.match_batch),
                      ("jabd_match_iou_f32", box_ref.match_iou_batch)):
        (gl, gc, glm), err = R.abi_match(cuda, name, tg, pri)
        assert err is None, err
        assert bool((gl[1] == 0).all()) and bool((gc[1] == 0).all()) and bool((glm[1] == 0).all())
        rl, rc, rlm = ref([t0, t2], pri, 0.35, R.VAR)
        keep = [0, 2]
        assert torch.equal(gc[keep], rc) and torch.equal(glm[keep], rlm)
        if ref is box_ref.match_iou_batch:
            assert torch.equal(gl[keep], rl)
        else:
            torch.testing.assert_close(gl[keep], rl, rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError):
        ops.match_encode([t.to(cuda) for t in tg], pri.to(cuda), 0.35, list(R.VAR))


# =============================================================================
# GPU: loss
# =============================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("quant", [4, None])
def test_l1_images_without_positives(cuda, kind, quant):
    inp = _l1_inputs(kind, quant=quant, seed=31 if quant else UNQUANT["L1"])
    info = _oracle(inp, kind)[3]
    assert info["sel"].sum(1).tolist() == [0, 168, 24] and info["counts"] == (33, 24)
    _run(cuda, inp, kind, exact_sel=quant is not None)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_l1_batch_without_positives(cuda, kind):
    """Both normalisers clamp to 1; losses and gradients are exactly zero."""
    from jabd_amd import ops
    inp = _l1_inputs(kind, conf_t=torch.zeros(3, 168, dtype=torch.int64))
    out = _oracle(inp, kind)
    assert out[3]["counts"] == (0, 0) and all(float(v) == 0.0 for v in out[:3])
    _run(cuda, inp, kind, exact_sel=True)
    pri, loc, conf, landm, lt, ct, lmt = (t.to(cuda) for t in inp)
    d = None if kind is None else (pri, R.VAR, kind)
    sums, counts, sel = ops.multibox_sums(loc, conf, landm, lt, ct, lmt, 7, d)
    loss = ops.multibox_normalize(sums, counts)
    assert counts.tolist() == [0, 0] and int(sel.sum()) == 0
    assert bool((loss == 0).all())
    gout = torch.tensor([2.0, 1.0, 1.0], device=cuda)
    for g in ops.multibox_backward(loc, conf, landm, lt, ct, lmt, sel, gout, counts, d):
        assert bool((g == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("variant", ["plain", "outlier"])
def test_l2_num_neg_clamp(cuda, kind, variant):
    inp = _l2_inputs(kind, variant)
    info = _oracle(inp, kind)[3]
    assert info["sel"].sum(1).tolist() == {"plain": [42, 8], "outlier": [41, 7]}[variant]
    _run(cuda, inp, kind, exact_sel=True)


@pytest.mark.gpu
def test_l2_clamp_through_the_modules(cuda):
    """synth.targets at 32² (A = 42) through both MultiBoxLoss modules, the
    device matching the targets itself: an image's 7 npos exceeds 41."""
    pri = R.priors(32)
    tg = R.synth_targets(3, 32, 2)
    loc, conf, landm = _preds(3, 42, 34, quant=4)
    for kind in KINDS:
        ref = box_ref.match_batch if kind is None else box_ref.match_iou_batch
        lt, ct, lmt = ref(tg, pri)
        assert int((ct != 0).sum(1).max()) * 7 > 41
        _check_loss(cuda, pri, tg, loc, conf, landm, lt, ct, lmt, exact_sel=True, kind=kind)


@pytest.mark.gpu
def test_l3_minus_inf_mining(cuda):
    pri, loc, conf, landm, lt, ct, lmt = _l1_inputs(None)
    conf[2, 150, 1] = 120.0
    info = box_ref.multibox_loss(loc, conf, landm, lt, ct, lmt)[3]
    m = info["mining"].clone()
    m[2, 150] = -INF
    assert bool((m[~info["pos"]] == -INF).all())          # no denormal involved
    assert info["sel"].sum(1).tolist() == [0, 167, 21]
    _check_loss(cuda, pri, None, loc, conf, landm, lt, ct, lmt, exact_sel=True)


@pytest.mark.gpu
@pytest.mark.parametrize("row,col,selected", [(160, 0, False), (2, 1, True)])
def test_l4_nan_logit(cuda, row, col, selected):
    pri, loc, conf, landm, lt, ct, lmt = _l1_inputs(None)
    conf[2, row, col] = NAN
    out = box_ref.multibox_loss(loc, conf, landm, lt, ct, lmt)
    assert bool(out[3]["sel"][2, row]) == selected
    assert bool(torch.isnan(out[1])) == selected
    assert out[3]["sel"].sum(1).tolist() == [0, 168, 24]
    _check_loss(cuda, pri, None, loc, conf, landm, lt, ct, lmt, exact_sel=True,
                nan_c=selected)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("quant", [4, None])
def test_l5_batch_above_64(cuda, kind, quant):
    inp = _l1_inputs(kind, quant=quant, conf_t=_l5_conf_t(), seed=35 if quant else UNQUANT["L5"])
    assert inp[1].shape[:2] == (65, 42)
    _run(cuda, inp, kind, exact_sel=quant is not None)


@pytest.mark.gpu
@pytest.mark.parametrize("neg_pos", [0, 1, 1000])
def test_l6_neg_pos(cuda, neg_pos):
    inp = _l1_inputs(None)
    info = _oracle(inp, None, neg_pos)[3]
    assert info["sel"].sum(1).tolist() == {0: [0, 30, 3], 1: [0, 60, 6],
                                           1000: [0, 168, 168]}[neg_pos]
    _run(cuda, inp, None, exact_sel=True, neg_pos=neg_pos)
