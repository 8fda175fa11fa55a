"""Gaussian Soft-NMS (jabd_batched_soft_nms_f32 / jabd_detect_soft_f32) through
jabd_amd.ops, utils.utils_bbox and jabd_amd.predict.

tests/_softnms_ref.py holds the references: two numpy restatements of the
reference's softer_nms loop (literal and vectorised sweep, numpy.exp) and the C
twin, the literal loop on the arithmetic of csrc/softnms_math.h, which the
kernel compiles too.  The device must equal the twin in every index and every
score bit; the twin equals numpy's arithmetic wherever the restatement's
margin (the closest pair of scores it had to tell apart) allows."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _softnms_ref as R


def _clustered(n, seed, scale=1.0, ties=True):
    """Pixel boxes in clusters of ~8 (scale 1/700: normalised), scores in
    (0.02, 1); with ties: an exact duplicate row, equal scores on three rows."""
    rng = np.random.default_rng(seed)
    nc = max(1, n // 8)
    cx, cy, sz = rng.uniform(0, 600, nc), rng.uniform(0, 600, nc), rng.uniform(10, 80, nc)
    k = rng.integers(0, nc, n)
    x, y = cx[k] + rng.normal(0, 4, n), cy[k] + rng.normal(0, 4, n)
    w, h = sz[k] * rng.uniform(0.8, 1.2, n), sz[k] * rng.uniform(0.8, 1.2, n)
    b = np.stack([x, y, x + w, y + h], 1).astype(np.float32) * np.float32(scale)
    s = rng.uniform(0.02, 1, n).astype(np.float32)
    if ties and n >= 30:
        b[10], s[10] = b[3], s[3]
        s[20] = s[21] = s[22]
    return b, s


def _disjoint(n, step=20.0):
    """n boxes 10 x 10 on a grid of pitch `step`: no two overlap, even with
    offset 1."""
    i = np.arange(n)
    x, y = (i % 64) * step, (i // 64) * step
    return np.stack([x, y, x + 10, y + 10], 1).astype(np.float32)


def _rows(b, s):
    return np.concatenate([b, s[:, None]], 1).astype(np.float32)


# ------------------------------------------------------------------ CPU: restatements
@pytest.mark.parametrize("offset", [0.0, 1.0])
def test_literal_loop_equals_vectorised_sweep(offset):
    """The swap-order equivalence the kernel rests on: the position-by-position
    loop and the one-sweep form (dead positions below N', ascending, filled by
    the survivors at or above N', descending) give the same lists and the same
    score bits -- with duplicate rows, equal scores on disjoint boxes, and
    sigmas small enough that whole clusters die in one sweep."""
    cases = [(_clustered(n, seed), sigma) for n in (2, 37, 150, 300) for seed in (0, 1)
             for sigma in (0.5, 0.05)]
    db = _disjoint(40)
    cases.append(((db, np.full(40, 0.5, np.float32)), 0.5))           # all scores equal
    dup = np.concatenate([db[:5]] * 6)                                  # six copies of five boxes
    cases.append(((dup, np.tile(np.float32([0.9, 0.8, 0.8, 0.7, 0.9]), 6)), 0.1))
    for (b, s), sigma in cases:
        k1, s1, _ = R.softnms_literal(_rows(b, s), sigma, offset)
        k2, s2 = R.softnms_sweep(_rows(b, s), sigma, offset)
        assert k1.tolist() == k2.tolist()
        assert s1.tobytes() == s2.tobytes()
        assert len(k1) == len(set(k1.tolist())) >= 1


def _all_impls(b, s, **kw):
    got = [R.run(b, s, impl=impl, **kw) for impl in (R.softnms_literal, R.softnms_sweep,
                                                      R.softnms_c)]
    for g in got[1:]:
        assert g[0].tolist() == got[0][0].tolist()
    return got


def test_kat_two_overlapping_boxes():
    # offset 0: inter 5 x 10 = 50, union 100 + 100 - 50 -> o = 1/3;
    # offset 1: inter 6 x 11 = 66, union 121 + 121 - 66 = 176 -> o = 0.375
    b = np.float32([[0, 0, 10, 10], [5, 0, 15, 10]])
    s = np.float32([0.9, 0.8])
    for offset, o in ((0.0, np.float32(50) / np.float32(150)), (1.0, np.float32(66) / np.float32(176))):
        want = np.float32(float(np.float32(0.8)) * math.exp(-float(o) * float(o) / 0.5))
        for keep, sc, *_ in _all_impls(b, s, sigma=0.5, offset=offset):
            assert keep.tolist() == [0, 1]
            assert sc[0] == np.float32(0.9)
            assert abs(int(sc[1].view(np.int32)) - int(want.view(np.int32))) <= 1


def test_kat_disjoint_boxes_come_in_descending_score_order_untouched():
    b = _disjoint(6)
    s = np.float32([0.3, 0.9, 0.5, 0.9, 0.1, 0.7])
    for keep, sc, *_ in _all_impls(b, s, offset=1.0):
        # rows 1 and 3 tie: the first position holding the maximum goes first.
        # The swaps then order the rest: [0.9a, 0.3, 0.5, 0.9b, ...] -> row 3 next
        assert keep.tolist() == [1, 3, 5, 2, 0, 4]
        assert sc.tolist() == s[[1, 3, 5, 2, 0, 4]].tolist()


def test_kat_three_identical_boxes_small_sigma_leave_one():
    # o = 1: exp(-1 / 0.05) = 2e-9, both copies fall below prune at once
    b = np.float32([[1, 2, 30, 40]] * 3)
    for keep, sc, *_ in _all_impls(b, np.float32([0.5, 0.7, 0.6]), sigma=0.05):
        assert keep.tolist() == [1] and sc.tolist() == [np.float32(0.7)]


def test_kat_nan_coordinate_decays_nothing():
    b = np.float32([[0, 0, 10, 10], [1, 1, 11, np.nan], [2, 2, 12, 12]])
    s = np.float32([0.9, 0.8, 0.7])
    for keep, sc, *_ in _all_impls(b, s):
        assert keep.tolist() == [0, 1, 2]
        assert sc[1] == np.float32(0.8)       # NaN overlap with rows 0 and 2
        assert sc[2] < np.float32(0.7)        # decayed by row 0 only
    only0 = R.run(b[[0, 2]], s[[0, 2]])[1][1]
    assert R.run(b, s)[1][2] == only0


def test_kat_nan_score_is_dropped():
    b = _disjoint(4)
    s = np.float32([0.5, np.nan, 0.7, 0.6])
    for keep, sc, *_ in _all_impls(b, s):
        assert keep.tolist() == [2, 3, 0]
    assert R.candidates(s).tolist() == [0, 2, 3]
    assert R.candidates(s, score_threshold=0.6).tolist() == [2, 3]
    assert R.candidates(s, n_valid=1).tolist() == [0]


def test_kat_top_k_cut_with_a_tie_at_the_cut():
    # scores 0.9 | 0.8 0.8 0.8 | 0.1: top_k = 3 takes 0.9 and the two 0.8 of the
    # lower rows (1 and 2); row 3 is no candidate.  They start in row order.
    b = _disjoint(5)
    s = np.float32([0.1, 0.8, 0.8, 0.8, 0.9])
    assert R.candidates(s, top_k=3).tolist() == [1, 2, 4]
    for keep, sc, *_ in _all_impls(b, s, top_k=3):
        assert keep.tolist() == [4, 2, 1]     # 0.9 swaps with row 1, then the first 0.8
    assert R.candidates(s, top_k=0).tolist() == [0, 1, 2, 3, 4]
    assert R.candidates(s, top_k=9).tolist() == [0, 1, 2, 3, 4]


def test_shared_exp_against_numpy():
    """csrc/softnms_math.h's exp on [-750, 0] against numpy.exp evaluated in
    extended precision.  Normal results: relative error <= 2^-50.  Subnormal
    results (x < -708.4) cannot carry a relative bound -- the format resolves
    them to 2^-1074 absolute -- and are held to one unit of that grid; below
    the underflow edge the result is 0.  exp(0) is exactly 1."""
    x = np.concatenate([np.linspace(-750.0, 0.0, 150001), -np.logspace(-12, 2.875, 20000),
                        [0.0, -0.0, -1e-300, -2.0 ** -28, -0.34657359027997264, -708.3964185322641,
                         -709.0, -744.0, -745.1332191019411, -745.1332191019412, -745.2, -750.0]])
    y = R.exp_nonpos(x)
    assert y[x == 0.0].tolist() == [1.0] * int((x == 0.0).sum())
    ref = np.exp(x.astype(np.longdouble))
    assert np.finfo(np.longdouble).nmant >= 63, "needs an extended-precision long double"
    err = np.abs(y.astype(np.longdouble) - ref)
    normal = ref >= np.longdouble(2.0) ** -1022
    rel = float((err[normal] / ref[normal]).max())
    sub = float((err[~normal] / np.longdouble(2.0) ** -1074).max())
    print(f"exp: max relative error {rel:.3e} (2^-50 = {2.0 ** -50:.3e}); "
          f"subnormal results within {sub:.3f} grid units")
    assert (~normal).sum() > 1000 and (y[~normal] > 0).sum() > 1000
    assert rel <= 2.0 ** -50
    assert sub <= 1.0
    assert y[x < -745.14].tolist() == [0.0] * int((x < -745.14).sum())
    assert np.all(np.diff(y[:150001]) >= 0)      # monotone over the grid
    # and numpy's own double exp is no further than its rounding from it
    assert float((np.abs(y - np.exp(x))[normal] / np.exp(x)[normal]).max()) <= 2.0 ** -50


# seeds chosen so that the restatement's margin is >= 1e-6 (asserted below)
@pytest.mark.parametrize("n,seed,offset", [(50, 0, 0.0), (50, 1, 1.0), (150, 0, 0.0), (150, 2, 1.0),
                                           (300, 0, 0.0), (300, 2, 0.0), (300, 0, 1.0),
                                           (300, 1, 1.0)])
def test_c_twin_against_the_numpy_restatement(n, seed, offset):
    """The twin's exp is its own, numpy's is the reference's arithmetic: where
    no two scores that had to be told apart are closer than 1e-6 (relative;
    nor a decayed score to prune), the lists are equal and every score is
    within 4 fp32 ulp (a decay is one fp32 rounding of a double product whose
    factor differs by < 2^-50; the ulps of successive decays add up)."""
    b, s = _clustered(n, seed, scale=1.0 if offset else 1.0 / 700)
    kn, sn, margin = R.softnms_literal(_rows(b, s), 0.5, offset)
    print(f"n={n} seed={seed} offset={offset}: {len(kn)} rows, margin {margin:.3e}")
    assert margin >= 1e-6
    kc, sc = R.softnms_c(_rows(b, s), 0.5, offset)
    assert kc.tolist() == kn.tolist()
    ulp = np.abs(sn.view(np.int32).astype(np.int64) - sc.view(np.int32).astype(np.int64))
    assert int(ulp.max()) <= 4


def test_key_orders_scores_as_numpy_argmax():
    key = R._twin().softnms_ref_key
    vals = [-np.inf, -2.0, -1e-40, -0.0, 0.0, 1e-40, 0.5, 1.0, np.inf, np.nan]
    keys = [key(float(v)) for v in vals]
    assert keys[3] == keys[4]                              # -0 == +0
    assert keys == sorted(keys) and len(set(keys)) == len(keys) - 1
    assert min(keys) > 0 and keys[-1] == 0xFFFFFFFF         # 0 is free for "no element"


# ------------------------------------------------------------------ CPU: argument checks
def test_bad_arguments_raise_before_any_device_work():
    from jabd_amd import ops
    from utils import utils_bbox
    b, s = torch.zeros(1, 3, 4), torch.zeros(1, 3)      # CPU tensors: never reached
    for kw in ({"sigma": 0.0}, {"sigma": -1.0}, {"sigma": math.inf}, {"sigma": math.nan},
               {"offset": math.inf}, {"offset": math.nan}, {"prune": math.nan},
               {"prune": math.inf}):
        with pytest.raises(ValueError):
            ops.batched_soft_nms(b, s, **kw)
    det = (torch.zeros(1, 3, 4), torch.zeros(1, 3, 2), torch.zeros(1, 3, 10), torch.zeros(3, 4),
           [0.1, 0.2])
    for kw in ({"sigma": 0.0}, {"sigma": math.nan}, {"soft_offset": math.inf}):
        with pytest.raises(ValueError):
            ops.detect(*det, nms_kind="softnms", **kw)
        with pytest.raises(ValueError):
            utils_bbox.non_max_suppression(torch.zeros(3, 15), nms_kind="softernms", **kw)
    with pytest.raises(ValueError):
        utils_bbox.softer_nms(torch.zeros(3, 15), sigma=0.0)
    with pytest.raises(ValueError):
        utils_bbox.softer_nms(torch.zeros(3, 4))
    for kind in ("softnmsx", "soft", "linear", None):
        with pytest.raises(ValueError):
            ops.detect(*det, nms_kind=kind)
    # the index-list entry points have no soft kind
    for kind in ("softnms", "softernms"):
        with pytest.raises(ValueError):
            ops.batched_nms(b, s, 0.3, kind=kind)
    assert ops.is_soft_kind("softnms") and ops.is_soft_kind("softernms")
    assert not ops.is_soft_kind("greedynms") and not ops.is_soft_kind(0)


def test_c_entry_points_return_einval():
    """sigma / offset / prune are checked before any device work: with null
    pointers and no GPU the calls return JABD_EINVAL (1) and say why."""
    from jabd_amd import _lib
    h = _lib.lib()
    ok = (0.5, 1.0, 0.001)
    bad = [(0.0, 1.0, 0.001), (-0.5, 1.0, 0.001), (math.inf, 1.0, 0.001), (math.nan, 1.0, 0.001),
           (0.5, math.inf, 0.001), (0.5, math.nan, 0.001), (0.5, 1.0, math.nan),
           (0.5, 1.0, -math.inf)]
    for sigma, offset, prune in bad:
        for batch, n in ((1, 5), (0, 0), (2, 0)):
            st = h.jabd_batched_soft_nms_f32(None, 4, 0, None, 1, 0, None, batch, n, sigma, offset,
                                             prune, 0.5, 0, None, None, None, None, 0, None)
            assert st == 1, (sigma, offset, prune, batch, n)
            assert "soft_nms" in _lib.last_error()
            st = h.jabd_detect_soft_f32(None, None, None, None, batch, n, 0.1, 0.2, 0.5, sigma,
                                        offset, prune, 0, None, None, None, 0, None)
            assert st == 1, (sigma, offset, prune, batch, n)
    # an empty batch with good arguments launches nothing and succeeds
    assert h.jabd_batched_soft_nms_f32(None, 4, 0, None, 1, 0, None, 0, 0, *ok, 0.5, 0, None, None,
                                       None, None, 0, None) == 0
    assert h.jabd_detect_soft_f32(None, None, None, None, 0, 0, 0.1, 0.2, 0.5, *ok, 0, None, None,
                                  None, 0, None) == 0
    assert h.jabd_batched_soft_nms_f32(None, 3, 0, None, 1, 0, None, 1, 5, *ok, 0.5, 0, None, None,
                                       None, None, 0, None) == 1     # row stride < 4
    out = ctypes.c_size_t(0)
    assert h.jabd_soft_nms_workspace_size(2, 100, ctypes.byref(out)) == 0 and out.value > 0
    assert h.jabd_detect_soft_workspace_size(2, 100, ctypes.byref(out)) == 0 and out.value > 0
    assert h.jabd_soft_nms_workspace_size(-1, 100, ctypes.byref(out)) == 1


def test_graph_key_holds_the_soft_parameters(monkeypatch):
    """graphed_detect: sigma, soft_offset and top_k are part of the key of the
    soft kind, nms_thres and beta1 (ignored by it) are not, and both names
    share graphs; the hard kinds still build GraphedDetect with their old
    positional arguments."""
    from jabd_amd import predict

    class Net:
        pass

    built = []

    class Fake:
        def __init__(self, net, shape, priors, variances, conf_thres, nms_thres, device, nms_kind,
                     beta1, top_k, **kw):
            self.gen, self.pri = predict.hipmodule.generation(), priors
            built.append((nms_kind, kw))

        def __call__(self, x):
            return None

    monkeypatch.setattr(predict, "GraphedDetect", Fake)
    monkeypatch.setattr(predict, "GRAPH_CACHE", 16)
    net, x, pri = Net(), torch.zeros(1, 3, 8, 8), torch.zeros(4, 4)
    calls = [dict(nms_kind="softnms"), dict(nms_kind="softernms"),
             dict(nms_kind="softnms", nms_thres=0.7, beta1=2.0),
             dict(nms_kind="softnms", sigma=0.3), dict(nms_kind="softnms", soft_offset=1.0),
             dict(nms_kind="softnms", top_k=50), dict(nms_kind="greedynms"),
             dict(nms_kind="greedynms", sigma=0.3)]
    for kw in calls:
        predict.graphed_detect(net, x, pri, [0.1, 0.2], 0.5, **kw)
    assert [b[0] for b in built] == ["softnms", "softnms", "softnms", "softnms", "greedynms"]
    assert built[0][1] == {"sigma": 0.5, "soft_offset": 0.0}
    assert built[1][1] == {"sigma": 0.3, "soft_offset": 0.0}
    assert built[2][1] == {"sigma": 0.5, "soft_offset": 1.0}
    assert built[4][1] == {}
    with pytest.raises(ValueError):
        predict.graphed_detect(net, x, pri, [0.1, 0.2], 0.5, nms_kind="softnms", sigma=0.0)


# ------------------------------------------------------------------ GPU: device against the twin
LDS, WS = ("soft_nms_lds", 1), ("soft_nms_ws", 2)
LDS_ROWS = 16000     # the kernel's LDS-state bound on candidates (jabd.h)


def _check(cuda, boxes, scores, n_valid=None, form=None, **kw):
    """ops.batched_soft_nms on [B, N, C] boxes against the twin, image by
    image: n_keep, every keep index, every keep_scores bit."""
    from jabd_amd import _lib, ops
    boxes, scores = np.asarray(boxes, np.float32), np.asarray(scores, np.float32)
    B = scores.shape[0]
    nv = None if n_valid is None else torch.tensor(n_valid, dtype=torch.int64, device=cuda)
    _lib.launch_log_reset()
    keep, ks, nk = ops.batched_soft_nms(torch.from_numpy(boxes).to(cuda),
                                        torch.from_numpy(scores).to(cuda), n_valid=nv, **kw)
    log = _lib.launch_log()
    keep, ks, nk = keep.cpu().numpy(), ks.cpu().numpy(), nk.cpu().numpy()
    if form is not None:
        assert log == [form]
    for b in range(B):
        rk, rs = R.run(boxes[b], scores[b], n_valid=None if n_valid is None else n_valid[b], **kw)
        k = int(nk[b])
        assert k == len(rk), (b, k, len(rk))
        assert keep[b, :k].tolist() == rk.tolist(), b
        assert ks[b, :k].tobytes() == rs.tobytes(), b
    return nk


@pytest.mark.gpu
@pytest.mark.parametrize("cands", [0, 1, 2, 63, 64, 65, 1023, 1024, 1025])
def test_candidate_counts_around_the_wave_and_workgroup_sizes(cuda, cands):
    """`cands` candidates among rows that also hold NaN scores and scores below
    the threshold (1024 threads: one case on each side of the workgroup)."""
    n = cands + 9
    b, s = _clustered(n, seed=cands, ties=cands >= 30)
    out = np.linspace(0, n - 1, 9).astype(int)
    s[out[::2]] = np.nan
    s[out[1::2]] = 0.01
    nk = _check(cuda, b[None], s[None], score_threshold=0.02, form=LDS)
    assert (cands == 0) == (int(nk[0]) == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n,top_k,form", [(LDS_ROWS, 0, LDS), (LDS_ROWS + 1, 0, WS),
                                          (LDS_ROWS + 1, LDS_ROWS, LDS),
                                          (LDS_ROWS + 2, LDS_ROWS + 1, WS)])
def test_each_side_of_the_state_form_switch(cuda, n, top_k, form):
    """The state is in LDS up to 16000 candidates -- bounded by n, or by top_k
    when it cuts lower -- and in the workspace above; the witness names the
    form and both give the twin's result."""
    b, s = _clustered(n, seed=3)
    _check(cuda, b[None], s[None], top_k=top_k, form=form)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["all_die", "none_die", "dead_tail", "dead_front", "alternate"])
def test_relocation_sweeps(cuda, case):
    """First sweeps with a known relocation, three positions per thread:
    all_die     2500 copies of one box, sigma 0.05: every remaining row dies;
    none_die    disjoint boxes: nothing decays, nothing moves;
    dead_tail   the copies of the selected box fill the tail: N shrinks, no move;
    dead_front  the copies come first and as many survivors sit in the tail:
                every hole below N' is filled from the top, in reverse;
    alternate   every second row is a copy: the thread whose positions straddle
                N' has a hole (1250), then a survivor to move (1251)."""
    n, h = 2500, 1000
    dj = _disjoint(n)
    rng = np.random.default_rng(11)
    low = rng.uniform(0.1, 0.8, n).astype(np.float32)
    top = np.float32([0, 0, 10, 10])
    if case == "all_die":
        b, s = np.tile(np.float32([5, 5, 50, 60]), (n, 1)), low.copy()
    elif case == "none_die":
        b, s = dj, low.copy()
    else:
        b, s = dj.copy(), low.copy()
        s[0] = 0.9
        b[0] = top
        if case == "dead_tail":
            b[n - h:] = top
        elif case == "dead_front":
            b[1:h + 1] = top
        else:
            b, s = np.concatenate([b, b[:1] + 5000]), np.append(s, np.float32(0.5))
            b[2::2] = top
            h = 1250
    nk = _check(cuda, b[None], s[None], sigma=0.05, offset=1.0, form=LDS)
    assert int(nk[0]) == {"all_die": 1, "none_die": n}.get(case, len(s) - h)
    if case == "dead_front":      # the holes 1..h took the last h rows, reversed
        k, _ = R.run(b, s, sigma=0.05)
        assert k[0] == 0 and sorted(k.tolist()) == [0] + list(range(h + 1, n))


@pytest.mark.gpu
def test_ties_and_duplicate_rows(cuda):
    """Few distinct scores, every box four times: the selection's tie rule (the
    lowest position) and the swaps decide the whole order."""
    b, s = _clustered(300, seed=5, ties=False)
    b = np.tile(b, (4, 1))
    s = np.tile(np.round(s * 8) / 8 + np.float32(0.125), 4).astype(np.float32)
    nk = _check(cuda, np.stack([b, b[::-1]]), np.stack([s, s[::-1]]), form=LDS)
    assert int(nk[0]) > 0 and int(nk[1]) > 0
    eq = np.full(700, 0.5, np.float32)                    # equal scores on disjoint boxes
    _check(cuda, _disjoint(700)[None], eq[None], form=LDS)


@pytest.mark.gpu
def test_batch_n_valid_and_threshold(cuda):
    """B = 3 with n_valid 700 / 0 / 1300 of 1300 rows; then a threshold that
    removes every row of the middle image."""
    bs, ss = zip(*[_clustered(1300, seed=20 + i) for i in range(3)])
    b, s = np.stack(bs), np.stack(ss)
    nk = _check(cuda, b, s, n_valid=[700, 0, 1300], form=LDS)
    assert int(nk[1]) == 0 and int(nk[0]) > 0 and int(nk[2]) > int(nk[0])
    s[1] *= np.float32(0.29)
    nk = _check(cuda, b, s, score_threshold=0.3, form=LDS)
    assert int(nk[1]) == 0 and int(nk[0]) > 0


@pytest.mark.gpu
def test_rows_of_15_columns_with_scores_aliasing_column_4(cuda):
    """The C entry point on [B, N, 15] rows with the score pointer inside the
    rows (stride 15), as jabd_detect_soft_f32 calls it; the input is left
    unchanged."""
    from jabd_amd import ops
    from jabd_amd._lib import call
    B, N = 2, 900
    rows = np.random.default_rng(2).uniform(0, 1, (B, N, 15)).astype(np.float32)
    for i in range(B):
        b, s = _clustered(N, seed=30 + i)
        rows[i, :, :4], rows[i, :, 4] = b, s
    t = torch.from_numpy(rows).to(cuda)
    keep = torch.empty((B, N), dtype=torch.int64, device=cuda)
    ks = torch.empty((B, N), dtype=torch.float32, device=cuda)
    nk = torch.empty((B,), dtype=torch.int64, device=cuda)
    ws = ops._ws(ops._size_query("jabd_soft_nms_workspace_size", B, N), cuda)
    call("jabd_batched_soft_nms_f32", ops._p(t), 15, N * 15, ctypes.c_void_p(t.data_ptr() + 16), 15,
         N * 15, None, B, N, 0.5, 1.0, 0.001, 0.25, 0, ops._p(keep), ops._p(ks), ops._p(nk),
         ops._p(ws), ws.numel(), ops._stream())
    assert np.array_equal(t.cpu().numpy(), rows)
    for i in range(B):
        rk, rs = R.run(rows[i], rows[i, :, 4], score_threshold=0.25)
        k = int(nk[i])
        assert keep[i, :k].cpu().tolist() == rk.tolist()
        assert ks[i, :k].cpu().numpy().tobytes() == rs.tobytes()


@pytest.mark.gpu
def test_top_k_cut_with_a_tie_at_the_cut(cuda):
    """Scores on a grid of 40 values over 2000 rows: the top_k-th best score is
    shared by ~50 rows, of which the lower rows are taken."""
    b, s = _clustered(2000, seed=8, ties=False)
    s = (np.ceil(s * 40) / 40).astype(np.float32)
    for top_k in (1, 333, 1999, 2000, 5000):
        cand = R.candidates(s, top_k=top_k)
        assert len(cand) == min(top_k, 2000)
        _check(cuda, b[None], s[None], top_k=top_k, form=LDS)
    cut = np.sort(s)[::-1][332]
    assert (s == cut).sum() > 10 and (s[R.candidates(s, top_k=333)] == cut).sum() < (s == cut).sum()


@pytest.mark.gpu
def test_offset_0_on_normalised_and_1_on_pixel_boxes(cuda):
    b, s = _clustered(1500, seed=9)
    n1 = _check(cuda, b[None], s[None], offset=1.0, form=LDS)
    bn = b * np.float32(1 / 700)
    n0 = _check(cuda, bn[None], s[None], offset=0.0, form=LDS)
    assert 0 < int(n0[0]) < 1500 and 0 < int(n1[0]) < 1500
    # the pixel +1 on normalised boxes: every pair overlaps, every sweep decays every row
    _check(cuda, bn[None], s[None], offset=1.0, form=LDS)


@pytest.mark.gpu
def test_nan_boxes_and_infinite_scores(cuda):
    b, s = _clustered(800, seed=12)
    b[5, 2] = b[77, 0] = b[300, 3] = np.nan
    s[9], s[10] = np.inf, -np.inf
    s[400] = -0.0
    _check(cuda, b[None], s[None], form=LDS)


@pytest.mark.gpu
@pytest.mark.parametrize("batch,n", [(2, 4096), (1, 20000)])
def test_larger_clustered_images(cuda, batch, n):
    bs, ss = zip(*[_clustered(n, seed=40 + i) for i in range(batch)])
    nk = _check(cuda, np.stack(bs), np.stack(ss), form=LDS if n <= LDS_ROWS else WS)
    assert all(n // 8 < int(k) < n for k in nk)


@pytest.mark.gpu
def test_empty_inputs(cuda):
    from jabd_amd import ops
    keep, ks, nk = ops.batched_soft_nms(torch.zeros(3, 0, 4, device=cuda),
                                        torch.zeros(3, 0, device=cuda))
    assert keep.shape == (3, 0) and nk.cpu().tolist() == [0, 0, 0]
    keep, ks, nk = ops.batched_soft_nms(torch.zeros(0, 5, 4, device=cuda),
                                        torch.zeros(0, 5, device=cuda))
    assert nk.shape == (0,)


# ------------------------------------------------------------------ GPU: public surfaces
@pytest.mark.gpu
def test_softer_nms_and_non_max_suppression(cuda):
    from utils import utils_bbox
    b, s = _clustered(600, seed=14)
    det = np.random.default_rng(3).uniform(0, 1, (600, 15)).astype(np.float32)
    det[:, :4], det[:, 4] = b, s
    t = torch.from_numpy(det).to(cuda)
    conf = torch.arange(600, device=cuda)
    rows, keep = utils_bbox.softer_nms(t, conf, sigma=0.4)        # pixel boxes, offset 1
    rk, rs = R.run(det, s, sigma=0.4, offset=1.0)
    assert keep.dtype == torch.int64 and keep.cpu().tolist() == rk.tolist()
    want = det[rk].copy()
    want[:, 4] = rs
    assert np.array_equal(rows.cpu().numpy(), want)
    assert np.array_equal(t.cpu().numpy(), det)                   # the input is not modified
    assert conf[keep].cpu().tolist() == rk.tolist()
    # non_max_suppression: normalised rows, offset 0 by default, score filter
    dn = det.copy()
    dn[:, :4] *= np.float32(1 / 700)
    for name in ("softnms", "softernms"):
        got = utils_bbox.non_max_suppression(torch.from_numpy(dn).to(cuda), conf_thres=0.4,
                                             nms_thres=0.9, nms_kind=name, sigma=0.4)
        rk, rs = R.run(dn, s, sigma=0.4, offset=0.0, score_threshold=0.4)
        want = dn[rk].copy()
        want[:, 4] = rs
        assert np.array_equal(got, want)
    assert utils_bbox.non_max_suppression(torch.from_numpy(dn).to(cuda), conf_thres=2.0,
                                          nms_kind="softnms") == []
    e_rows, e_keep = utils_bbox.softer_nms(torch.zeros(0, 15, device=cuda))
    assert e_rows.shape == (0, 15) and e_keep.shape == (0,)


@pytest.mark.gpu
def test_detect_soft_equals_decode_plus_batched_soft_nms(cuda):
    """ops.detect(nms_kind="softnms") on the 64 x 64 anchor set: the rows are
    decode / decode_landm / conf[:, 1] gathered through batched_soft_nms's
    keep, with its decayed scores in column 4."""
    from jabd_amd import ops
    from utils.anchors import Anchors
    from utils.config import cfg_mnet
    pri = Anchors(cfg_mnet, image_size=(64, 64)).get_anchors().to(cuda).float().contiguous()
    A, B = pri.shape[0], 2
    g = torch.Generator().manual_seed(5)
    loc = (torch.randn(B, A, 4, generator=g) * 1.5).to(cuda)
    conf = torch.softmax(torch.randn(B, A, 2, generator=g) * 2, -1).to(cuda)
    landm = torch.randn(B, A, 10, generator=g).to(cuda)
    var = cfg_mnet["variance"]
    for kw in ({}, {"sigma": 0.2, "top_k": 40}):
        rows, nk = ops.detect(loc, conf, landm, pri, var, 0.5, 0.3, nms_kind="softnms", **kw)
        boxes, lm = ops.decode(loc, pri, var), ops.decode_landm(landm, pri, var)
        keep, ks, nk2 = ops.batched_soft_nms(boxes, conf[..., 1].contiguous(), offset=0.0,
                                             score_threshold=0.5, **kw)
        assert torch.equal(nk, nk2)
        for b in range(B):
            k = int(nk[b])
            assert 0 < k <= (kw.get("top_k") or A)
            idx = keep[b, :k]
            assert torch.equal(rows[b, :k, :4], boxes[b, idx])
            assert torch.equal(rows[b, :k, 4], ks[b, :k])
            assert torch.equal(rows[b, :k, 5:], lm[b, idx])
        assert bool((ks[0, :int(nk[0])] < conf[0, keep[0, :int(nk[0])], 1]).any())   # decayed


@pytest.mark.gpu
def test_graphed_detect_soft_equals_eager(cuda):
    """The soft kind captured in a HIP graph (no host synchronisation, no
    memset) replays to the eager call's rows, on two inputs."""
    import bench
    from jabd_amd import functional as F
    from jabd_amd import ops
    from jabd_amd.predict import graphed_detect
    from utils.anchors import Anchors
    net, cfg = bench._weights_init_model("mnv3")
    net = net.eval().to(cuda)
    size = 640      # 16 800 anchors: the workspace form, a few hundred candidates
    pri = Anchors(cfg, image_size=(size, size)).get_anchors().to(cuda).float()
    var = cfg["variance"]
    g = torch.Generator().manual_seed(size)
    for _ in range(2):
        x = (torch.rand(1, 3, size, size, generator=g) * 255 - 117).to(cuda)
        with torch.no_grad():
            with F.split_k():
                out = net(x)
            r0, n0 = ops.detect(*out, pri, var, 0.5, 0.3, nms_kind="softnms", sigma=0.3)
            r1, n1 = graphed_detect(net, x, pri, var, 0.5, 0.3, nms_kind="softnms", sigma=0.3)
        k = int(n0[0])
        assert int(n1[0]) == k and k > 0
        assert torch.equal(r0[0, :k], r1[0, :k])
