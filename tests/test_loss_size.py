"""A7-A9 at the training shapes: batched match/encode and MultiBoxLoss (OHEM)
of the HIP path against the oracle restatement (oracle/box_ref.py) at the
sizes the training configs run, not only at 256².

Cases (VERDICT r04 "next round" 1):
  (i)   1024² (A = 43,008), bs32, the bench's own targets (synth seed 4321,
        bench.py C4 leg) — C4's loss leg;
  (ii)  one 1024² image with 1000 ground-truth boxes (synth.targets' cap),
        holding exact duplicates and groups of near-copies whose best prior
        collides (the last-writer-wins loop, nets/retinaface_training.py:129-130);
  (iii) the reference's own training size 840² (A = 29,126), bs8
        (train_mobilenetV3_ecagai.py trains at 840, utils/config.py).

Bars: conf_t (the assignment) bit-exact; landm_t bit-exact; loc_t 1e-5 (the
log() ulp, as test_box_ops.test_match_parity); the three losses 1e-5 relative;
the OHEM-selected set equal to the oracle's, or equal except for rows whose
mining loss lies within 4 ulp of the image's selection threshold (torch-CPU's
vectorised exp/log and the device's expf/logf may round such a pair apart) —
the number of such rows is counted and bounded; loc/conf/landm gradients 1e-5
relative.  A quantised-logit case (background logit 0, face logit on a 1/4
grid) makes exact ties at the threshold common: there the set must be
bit-identical (lowest index first among equal values,
the oracle's stable sort and csrc/box_ops.hip ohem_select_kernel) and the tie
count at the threshold is asserted to be non-zero.
Reference: nets/retinaface_training.py:93-162 (match), :183-303 (MultiBoxLoss;
OHEM sort :270-271, num_neg clamp :279).
"""
import numpy as np
import pytest
import torch

from _match_loss_ref import CFG_MNET, _check_loss, _preds
from oracle import box_ref


def _targets(B, size, seed):
    from jabd_amd import synth
    return [torch.from_numpy(t) for t in synth.targets(B, size, seed=seed)]


def _crowd_image(size, seed=77, n=1000):
    """1000 truths: 700 random faces, 100 exact duplicates of some of them, and
    20 groups of 10 near-copies (sub-pixel jitter, so every member has the same
    best prior and the later one must win it)."""
    from jabd_amd import synth
    rng = np.random.default_rng(seed)
    base = synth.targets(1, size, seed=seed, max_faces=n)[0]
    while base.shape[0] < 700:
        base = np.concatenate([base, synth.targets(1, size, seed=int(rng.integers(1 << 30)),
                                                   max_faces=n)[0]])
    base = base[:700]
    dup = base[rng.integers(0, 700, 100)]
    groups = []
    for _ in range(20):
        src = base[rng.integers(0, 700)].copy()
        g = np.repeat(src[None], 10, 0)
        jit = rng.uniform(-0.05, 0.05, (10, 1)).astype(np.float32) / size
        g[:, 0:4] += jit
        groups.append(g)
    t = np.concatenate([base, dup] + groups).astype(np.float32)
    assert t.shape[0] == n
    perm = rng.permutation(n)
    return [torch.from_numpy(np.ascontiguousarray(t[perm]))]


def _check_match(cuda, tg, pri):
    from jabd_amd import ops
    rl, rc, rlm = box_ref.match_batch(tg, pri)
    gl, gc, glm = ops.match_encode([t.to(cuda) for t in tg], pri.to(cuda), 0.35, [0.1, 0.2])
    assert torch.equal(gc.cpu(), rc)
    torch.testing.assert_close(gl.cpu(), rl, rtol=1e-5, atol=1e-5)
    assert torch.equal(glm.cpu(), rlm)
    return rl, rc, rlm


@pytest.mark.gpu
def test_match_loss_c4_shape(cuda):
    """(i) 1024², bs32, the C4 bench's targets (bench.py: synth.targets seed 4321)."""
    pri = box_ref.anchors(CFG_MNET, (1024, 1024))
    assert pri.shape[0] == 43008
    tg = _targets(32, 1024, 4321)
    lt, ct, lmt = _check_match(cuda, tg, pri)
    assert int((ct != 0).sum()) > 0
    loc, conf, landm = _preds(32, pri.shape[0], 21)
    _check_loss(cuda, pri, tg, loc, conf, landm, lt, ct, lmt)


@pytest.mark.gpu
def test_match_loss_c4_shape_exact_ties(cuda):
    """(i) with logits on a 1/4 grid: thousands of exactly equal mining losses,
    many at each image's threshold — the selected set must still be the
    oracle's, bit for bit (lowest index first among equals)."""
    pri = box_ref.anchors(CFG_MNET, (1024, 1024))
    tg = _targets(32, 1024, 4321)
    lt, ct, lmt = box_ref.match_batch(tg, pri)
    loc, conf, landm = _preds(32, pri.shape[0], 22, quant=4)
    near, ties = _check_loss(cuda, pri, tg, loc, conf, landm, lt, ct, lmt, exact_sel=True)
    assert ties > 32, ties


@pytest.mark.gpu
def test_match_loss_crowd_image(cuda):
    """(ii) one image, 1000 truths with duplicates and best-prior collisions."""
    pri = box_ref.anchors(CFG_MNET, (1024, 1024))
    tg = _crowd_image(1024)
    # the collisions really happen: several truths share a best prior
    ov = box_ref.jaccard(tg[0][:, :4], box_ref.point_form(pri))
    bp = ov.max(1)[1]
    assert len(torch.unique(bp)) < 1000 - 100
    lt, ct, lmt = _check_match(cuda, tg, pri)
    loc, conf, landm = _preds(1, pri.shape[0], 23)
    _check_loss(cuda, pri, tg, loc, conf, landm, lt, ct, lmt)


@pytest.mark.gpu
def test_match_loss_reference_train_size(cuda):
    """(iii) 840² (A = 29,126), bs8 — the reference's training resolution."""
    pri = box_ref.anchors(CFG_MNET, (840, 840))
    assert pri.shape[0] == 29126
    tg = _targets(8, 840, 840)
    lt, ct, lmt = _check_match(cuda, tg, pri)
    loc, conf, landm = _preds(8, pri.shape[0], 24)
    _check_loss(cuda, pri, tg, loc, conf, landm, lt, ct, lmt)


def test_crowd_image_oracle_collisions():
    """CPU: the crowd fixture has exact duplicates and shared best priors, and
    the oracle's last-writer-wins rule gives every collided prior to the
    highest-index truth that claims it (nets/retinaface_training.py:129-130)."""
    pri = box_ref.anchors(CFG_MNET, (1024, 1024))
    t = _crowd_image(1024)[0]
    _, _, _, bti, bto = box_ref.match(0.35, t[:, :4], pri, [0.1, 0.2], t[:, -1], t[:, 4:14])
    ov = box_ref.jaccard(t[:, :4], box_ref.point_form(pri))
    bp = ov.max(1)[1]
    for p in torch.unique(bp):
        claim = (bp == p).nonzero().flatten()
        assert int(bti[p]) == int(claim.max())
        assert float(bto[p]) == 2.0
