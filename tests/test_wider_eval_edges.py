"""WIDER evaluation core (csrc/wider_eval.hip) and its numpy oracle
(oracle/wider_ref.py) at the edges tests/test_wider_eval.py never reaches
(cases and set builders: tests/_small_kernel_ref.py).

The oracle is pinned on the CPU by nine hand cases, each derived below from
utils/evaluation.py:255-305: a tie in the row argmax, IoU == iou_thresh,
score == threshold, a NaN overlap (from a NaN coordinate and from 0 / 0) and
unsorted scores.  The kernel must then equal the oracle exactly — the curve
holds integer counts — on those and on sets that make its three
`+= blockDim.x` loops (256 wide) take more than one trip:
  predictions  700 (three trips) and 257 (two, the second one lane wide)
  ground truths 300 and 257 (the recall[] reset loop)
  thresholds   thresh_num 257 and 1000; 1, 7, 255 and 256 stay within one
and that put empty images (no preds, no gts, neither) first, in the middle and
last, make every image empty, use 300 workgroups in one launch, and set every
ground truth ignored or kept.  Through the C ABI: pr_curve is accumulated into
(a second call doubles it, a pre-filled one is added to), num_images == 0
leaves it alone, and a workspace one byte short is refused.
"""
import ctypes

import numpy as np
import pytest

import _small_kernel_ref as R
from oracle import wider_ref


def _oracle(preds, gts, igs, iou, T):
    return wider_ref.pr_curve(preds, gts, [np.asarray(i, np.uint8) for i in igs], iou, T)


# ------------------------------------------------------------------- CPU: oracle
@pytest.mark.parametrize("name", list(R.WIDER_HAND))
def test_oracle_hand_case(name):
    """Derivations (image_eval :255-288, img_pr_info :291-308; a row of the
    curve is [proposals, recalled] at threshold 1 - (t + 1) / T):

    argmax-tie-*: both gts equal the pred, IoU 1 and 1; numpy's argmax returns
      the first index (:278), so gt 0 decides.  Ignored (ignore == 0, :280):
      proposal_list[h] = -1 and nothing is recalled -> [0, 0].  Kept: recalled,
      still a proposal -> [1, 1].  Score 0.9 passes all four thresholds.
    iou-equals-thresh: pred 10 x 5 inside gt 10 x 10: inter 50, union
      100 + 50 - 50 = 100, IoU = 0.5 exactly; `>=` (:279) recalls it -> [1, 1].
      With iou_thresh one ulp above 0.5 it is a plain proposal -> [1, 0].
    score-*: T = 7 and the score is 1 - 3/7 as :299 computes it, so `>=` (:300)
      first holds at t = 2; one ulp lower first holds at t = 3.  The pred misses
      the gt: proposals 1, recalled 0.
    nan-coordinate: x = NaN makes the whole overlap row NaN; NaN >= thresh is
      False (:279), so the pred stays a proposal and recalls nothing; the next
      pred is an exact hit -> [2, 1] at all four thresholds.
    zero-over-zero: a 0 x 0 pred on a 0 x 0 gt: inter 0, union 0, 0 / 0 = NaN;
      numpy's max of a row holding NaN is NaN (:278) -> a proposal.  The second
      pred's row is [0 / 100, 1] -> recalled.  [2, 1].
    unsorted-scores: scores .2, .9, .6.  r_index is the LAST index whose score
      passes (:305), whatever the order: threshold .8 -> index 1, preds 0..1 are
      both proposals and pred 0 already recalled the gt -> [2, 1]; thresholds
      .6 (1 - 2/5 == 0.6 in binary64), .4, .2, 0 -> index 2 -> [3, 1]."""
    preds, gts, igs, iou, T, expected = R.WIDER_HAND[name]
    assert np.array_equal(_oracle(preds, gts, igs, iou, T), np.asarray(expected, np.float64))


def test_hand_case_inputs_are_what_they_claim():
    p, g, _, iou, _, _ = R.WIDER_HAND["iou-equals-thresh"]
    a, b = p[0][:, :4].copy(), g[0].copy()
    a[:, 2:] += a[:, :2]
    b[:, 2:] += b[:, :2]
    assert wider_ref.overlaps(a, b)[0, 0] == 0.5 == iou
    assert R.WIDER_HAND["iou-one-ulp-under-thresh"][3] > 0.5
    s = R.WIDER_HAND["score-equals-threshold"][0][0][0, 4]
    assert s == 1 - 3 / 7 and R.WIDER_HAND["score-one-ulp-under-threshold"][0][0][0, 4] < s
    p, g, _, _, _, _ = R.WIDER_HAND["zero-over-zero"]
    a, b = p[0][:, :4].copy(), g[0].copy()
    a[:, 2:] += a[:, :2]
    b[:, 2:] += b[:, :2]
    assert np.isnan(wider_ref.overlaps(a, b)[0, 0])


def test_sets_are_not_trivial():
    """The big image recalls faces, turns ignored hits into non-proposals and
    has unsorted scores; the curve is monotone in neither trivial way."""
    preds, gts, igs = R.wider_set(R.WIDER_SETS["700x300-unsorted"], 3)
    assert (np.diff(preds[0][:, 4]) > 0).any() and (np.diff(preds[0][:, 4]) < 0).any()
    rec, prop = wider_ref.image_eval(preds[0], gts[0], igs[0], 0.5)
    assert rec[-1] >= 30 and 30 <= (prop == -1).sum() <= 670
    assert 0 < (igs[0] == 0).sum() < 300


# ------------------------------------------------------------------- GPU parity
def _gpu(cuda, preds, gts, igs, iou, T):
    from jabd_amd import ops
    igs = [np.asarray(i, np.uint8) for i in igs]
    return ops.wider_pr_curve(preds, gts, igs, iou, T, device=cuda).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.WIDER_HAND))
def test_hand_case_parity(cuda, name):
    preds, gts, igs, iou, T, expected = R.WIDER_HAND[name]
    assert np.array_equal(_gpu(cuda, preds, gts, igs, iou, T), np.asarray(expected, np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.WIDER_SETS))
def test_set_parity(cuda, name):
    preds, gts, igs = R.wider_set(R.WIDER_SETS[name], 3)
    T = 1000 if len(preds) < 10 else 50   # the oracle's threshold loop is per image
    for iou in (0.5, 0.3):
        ref = _oracle(preds, gts, igs, iou, T)
        assert np.array_equal(_gpu(cuda, preds, gts, igs, iou, T), ref)
        assert (name == "all-empty") == (not ref.any())


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 7, 255, 256, 257, 1000])
def test_thresh_num_parity(cuda, T):
    preds, gts, igs = R.wider_set([(300, 40), (0, 3), (5, 260)], 4)
    assert np.array_equal(_gpu(cuda, preds, gts, igs, 0.5, T), _oracle(preds, gts, igs, 0.5, T))


@pytest.mark.gpu
@pytest.mark.parametrize("ignore", [0, 1])
def test_ignore_all_parity(cuda, ignore):
    preds, gts, igs = R.wider_set([(300, 40), (20, 260)], 5, ignore=ignore)
    ref = _oracle(preds, gts, igs, 0.5, 100)
    assert np.array_equal(_gpu(cuda, preds, gts, igs, 0.5, 100), ref)
    assert not ref[:, 1].any() if ignore == 0 else ref[-1, 0] == 320   # nothing recalled / all proposals


# ------------------------------------------------------------------ C-ABI contract
def _abi_args(cuda, preds, gts, igs):
    import torch
    def cat(xs, shape, dt):
        flat = np.concatenate([np.asarray(x, dt).reshape(shape) for x in xs])
        offs = np.zeros(len(xs) + 1, np.int64)
        offs[1:] = np.cumsum([len(np.asarray(x).reshape(shape)) for x in xs])
        return torch.from_numpy(flat).to(cuda), torch.from_numpy(offs).to(cuda), int(offs[-1])
    p, poff, n_p = cat(preds, (-1, 5), np.float64)
    g, goff, n_g = cat(gts, (-1, 4), np.float64)
    ig, _, _ = cat(igs, (-1,), np.uint8)
    return p, poff, g, ig, goff, n_p, n_g


@pytest.mark.gpu
def test_abi_accumulates_and_refuses(cuda):
    import torch
    from jabd_amd import ops
    from jabd_amd._lib import c_size, call
    preds, gts, igs = R.wider_set([(40, 12), (0, 2), (9, 7)], 6)
    T = 50
    ref = _oracle(preds, gts, igs, 0.5, T)
    assert ref.any()
    p, poff, g, ig, goff, n_p, n_g = _abi_args(cuda, preds, gts, igs)
    need = c_size(0)
    call("jabd_wider_eval_workspace_size", n_p, n_g, ctypes.byref(need))
    ws = torch.empty(need.value, dtype=torch.uint8, device=cuda)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def run(pr, num_images=len(preds), ws_bytes=need.value):
        call("jabd_wider_eval_f64", ptr(p), ptr(poff), ptr(g), ptr(ig), ptr(goff), num_images,
             n_p, n_g, 0.5, T, ptr(pr), ptr(ws), ws_bytes, ops._stream())
        return pr.cpu().numpy()

    pr = torch.zeros(T, 2, dtype=torch.float64, device=cuda)
    assert np.array_equal(run(pr), ref)
    assert np.array_equal(run(pr), 2 * ref), "a second call adds to pr_curve"
    fill = np.arange(2.0 * T).reshape(T, 2) * 3 + 1
    pr = torch.from_numpy(fill).to(cuda)
    assert np.array_equal(run(pr), fill + ref), "a pre-filled pr_curve is added to"
    pr = torch.from_numpy(fill).to(cuda)
    assert np.array_equal(run(pr, num_images=0), fill), "num_images == 0 writes nothing"
    with pytest.raises(RuntimeError, match="workspace too small"):
        run(pr, ws_bytes=need.value - 1)
    assert np.array_equal(pr.cpu().numpy(), fill), "a refused call writes nothing"
