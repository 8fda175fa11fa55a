"""DIoU-NMS (kind 1 of jabd_batched_nms_ex_f32 / jabd_detect_ex_f32), beta1 and
top_k, through jabd_amd.ops, utils.utils_bbox and jabd_amd.predict.

The reference is tests/_diou_ref.py, a numpy fp32 restatement of the
reference's diounms (utils/box_utils.py:450-526).  The device index lists must
equal its lists exactly; "margin" is the restatement's smallest
|value - threshold| over the decisions it made on an input."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import _diou_ref as R


# ------------------------------------------------------------------ CPU: the restatement's KATs
def test_kat_two_boxes_iou_suppresses_diou_keeps():
    # inter 50, union 150 -> IoU 1/3; centres 5 apart, enclosing box 15 x 10:
    # u = 25 / 325; DIoU = 0.25641
    b = np.float32([[0, 0, 10, 10], [5, 0, 15, 10]])
    s = np.float32([0.9, 0.8])
    ki, mi = R.diounms(b, s, 0.3, kind="iou")
    kd, md = R.diounms(b, s, 0.3)
    assert ki.tolist() == [0] and kd.tolist() == [0, 1]
    assert abs(mi - (1 / 3 - 0.3)) < 1e-6
    assert abs(md - (0.3 - (1 / 3 - 25 / 325))) < 1e-6


def test_kat_identical_boxes_are_suppressed():
    b = np.float32([[1, 2, 3, 4]] * 3)
    assert R.diounms(b, np.float32([0.5, 0.7, 0.6]), 0.3)[0].tolist() == [1]


def test_kat_identical_point_boxes_are_both_kept():
    # c = 0: u = 0 / 0 = NaN, and a NaN value never suppresses
    b = np.float32([[0.5, 0.5, 0.5, 0.5]] * 2)
    assert R.diounms(b, np.float32([0.9, 0.8]), 0.0)[0].tolist() == [0, 1]


def test_kat_top_k_cuts_before_suppression():
    # row 1 overlaps row 0 (suppressed), row 2 is far away: with top_k = 2 row 2
    # is no candidate at all, so the cut cannot have come after suppression
    b = np.float32([[0, 0, 10, 10], [0, 0, 10, 9], [50, 50, 60, 60]])
    s = np.float32([0.9, 0.8, 0.7])
    for kind in ("iou", "diou"):
        assert R.diounms(b, s, 0.3, top_k=0, kind=kind)[0].tolist() == [0, 2]
        assert R.diounms(b, s, 0.3, top_k=2, kind=kind)[0].tolist() == [0]
        assert R.diounms(b, s, 0.3, top_k=1, kind=kind)[0].tolist() == [0]


def test_kat_three_boxes_differ_with_beta1():
    # vs row 0: row 1 has IoU 60/140, u = 16/296; row 2 has IoU 1/3, u = 25/325
    #   beta1 0.5: row 1 0.196 kept, row 2 0.056 vs row 0 but 0.751 vs row 1
    #   beta1 1  : row 1 0.375 suppressed, row 2 0.256 kept
    #   beta1 2  : row 1 0.426 suppressed, row 2 0.327 suppressed
    b = np.float32([[0, 0, 10, 10], [4, 0, 14, 10], [5, 0, 15, 10]])
    s = np.float32([0.9, 0.8, 0.7])
    got = {be: R.diounms(b, s, 0.3, beta1=be)[0].tolist() for be in (0.5, 1.0, 2.0)}
    assert got == {0.5: [0, 1], 1.0: [0, 2], 2.0: [0]}


def test_c_twin_agrees_with_the_restatement():
    """tests/_diou_ref.c (used for the 24k-row cases) against the numpy
    restatement: the same lists and the same margins, bit for bit at beta1 = 1
    (clustered boxes with score ties, NaN coordinates, degenerate boxes, both
    kinds, a top_k cut); beta1 != 1 under test_diou_beta1's margin condition."""
    b, s = _clustered(3000, seed=7)
    nb = b.copy()
    nb[7, 0] = nb[100, 3] = np.nan
    deg = np.float32([[0, 0, 1, 1]] * 5 + [[0.5, 0.5, 0.5, 0.5]] * 3 + [[0, 0, 2, 2], [2, 2, 1, 1]])
    degs = np.float32([0.5] * 5 + [0.0, -0.0, 0.0] + [0.5, 0.7])
    cases = [(b, s, thr, {"kind": kind, "top_k": top_k})
             for thr in (0.0, 0.3, 0.7) for kind in ("diou", "iou") for top_k in (0, 700)]
    cases += [(nb, s, 0.3, {}), (deg, degs, 0.0, {}), (deg, degs, 0.3, {}),
              (b[:0], s[:0], 0.3, {}), (b[:1], s[:1], 0.3, {})]
    for bx, sc, thr, kw in cases:
        kn, mn = R.diounms(bx, sc, thr, **kw)
        kc, mc = R.diounms_c(bx, sc, thr, **kw)
        assert kn.tolist() == kc.tolist() and mn == mc, (thr, kw)
    for beta1 in (0.5, 2.0):
        kn, mn = R.diounms(b, s, 0.3, beta1=beta1)
        kc, mc = R.diounms_c(b, s, 0.3, beta1=beta1)
        assert mn >= 1e-5 and abs(mn - mc) < 1e-6
        assert kn.tolist() == kc.tolist()


def test_c_twin_first_use_from_threads(tmp_path, monkeypatch):
    """The twin's first users are _ref_many's threads: from an empty temporary
    directory, with nothing loaded, three concurrent calls build it once and
    all succeed."""
    import tempfile
    monkeypatch.setattr(tempfile, "tempdir", str(tmp_path))
    monkeypatch.setattr(R, "_twin_fn", None)
    b = np.float32([[0, 0, 10, 10], [5, 0, 15, 10]])
    s = np.float32([0.9, 0.8])
    got = _ref_many([((b, s, 0.3), {}), ((b, s, 0.3), {"kind": "iou"}), ((b, s, 0.2), {})])
    assert [g[0].tolist() for g in got] == [[0, 1], [0], [0]]
    left = sorted(p.name for p in tmp_path.iterdir())
    assert len(left) == 1 and left[0].endswith(".so"), left


def test_graph_key_ignores_beta1_for_the_iou_kind(monkeypatch):
    """graphed_detect's cache: the IoU kind ignores beta1, so it is not part of
    that kind's key; kind, the DIoU kind's beta1 and top_k are."""
    from jabd_amd import predict

    class Net:
        pass

    built = []

    class Fake:
        def __init__(self, net, shape, priors, *a):
            self.gen, self.pri = predict.hipmodule.generation(), priors
            built.append(a[-3:])

        def __call__(self, x):
            return None

    monkeypatch.setattr(predict, "GraphedDetect", Fake)
    net, x, pri = Net(), torch.zeros(1, 3, 8, 8), torch.zeros(4, 4)
    calls = [("greedynms", 1.0, 0), ("greedynms", 2.0, 0), ("iou", 0.5, 0), ("diounms", 1.0, 0),
             ("diounms", 2.0, 0), ("diou", 2.0, 0), ("diounms", 2.0, 100), ("greedynms", 1.0, 100)]
    for kind, beta1, top_k in calls:
        predict.graphed_detect(net, x, pri, [0.1, 0.2], 0.5, 0.3, kind, beta1, top_k)
    assert built == [("greedynms", 1.0, 0), ("diounms", 1.0, 0), ("diounms", 2.0, 0),
                     ("diounms", 2.0, 100), ("greedynms", 1.0, 100)]


def test_abi_declares_the_ex_entry_points():
    import test_abi
    from jabd_amd import _lib
    names = {"jabd_batched_nms_ex_f32", "jabd_detect_ex_f32"}
    assert names <= set(test_abi._header_functions())
    assert names <= set(_lib.SIGNATURES)
    assert all(hasattr(_lib.lib(), n) for n in names)
    test_abi.test_library_exports_every_header_symbol()
    old, new = _lib.SIGNATURES["jabd_batched_nms_f32"], _lib.SIGNATURES["jabd_batched_nms_ex_f32"]
    assert new[:len(old)] == old and len(new) == len(old) + 3
    old, new = _lib.SIGNATURES["jabd_detect_f32"], _lib.SIGNATURES["jabd_detect_ex_f32"]
    assert new[:len(old)] == old and len(new) == len(old) + 3


def test_unknown_kind_and_bad_beta1_raise_value_error():
    from jabd_amd import ops
    b, s = torch.zeros(1, 3, 4), torch.zeros(1, 3)
    with pytest.raises(ValueError):
        ops.batched_nms(b, s, 0.3, kind="x")
    with pytest.raises(ValueError):
        ops.batched_nms_stats(b, s, 0.3, kind="softnms")
    with pytest.raises(ValueError):
        ops.detect(torch.zeros(1, 3, 4), torch.zeros(1, 3, 2), torch.zeros(1, 3, 10),
                   torch.zeros(3, 4), [0.1, 0.2], nms_kind="x")
    for beta1 in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ops.batched_nms(b, s, 0.3, kind="diou", beta1=beta1)


def test_c_abi_rejects_bad_kind_and_beta1():
    """The library checks its own arguments (before any device work: an empty
    batch needs no GPU); kind 0 ignores beta1."""
    from jabd_amd._lib import call

    def ex(kind, beta1):
        call("jabd_batched_nms_ex_f32", None, 4, 0, None, 1, 0, None, 0, 0, 0.3,
             float("-inf"), None, None, None, 0, None, kind, beta1, 0)
    ex(0, 1.0)
    ex(1, 0.5)
    ex(0, 0.0)
    for kind, beta1 in ((2, 1.0), (-1, 1.0), (1, 0.0), (1, -2.0), (1, float("inf")),
                        (1, float("nan"))):
        with pytest.raises(RuntimeError, match="beta1|kind"):
            ex(kind, beta1)


def test_diounms_empty_input():
    from utils.utils_bbox import diounms
    keep, count = diounms(torch.zeros(0, 4), torch.zeros(0))
    assert count == 0 and keep.dtype == torch.int64 and keep.numel() == 0


# ------------------------------------------------------------------ GPU: equal to the restatement
def _clustered(n, seed):
    from jabd_amd import synth
    b, s = synth.nms_boxes(1, n, seed=seed, tie_frac=0.05)
    return b[0], s[0]


@functools.lru_cache(maxsize=None)
def _ref3000(thr, kind, beta1=1.0):
    b, s = _clustered(3000, seed=7)
    return R.diounms(b, s, thr, kind=kind, beta1=beta1)


@functools.lru_cache(maxsize=None)
def _boxes24k():
    from jabd_amd import synth
    return synth.nms_boxes(2, 24_000, seed=23)


def _ref_many(jobs):
    """R.diounms_c(*args, **kw) for every (args, kw) of jobs, in threads: the C
    twin of the restatement (test_c_twin_agrees_with_the_restatement), whose
    call drops the GIL -- the 24k-row cases take seconds each in numpy."""
    with ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        return list(ex.map(lambda j: R.diounms_c(*j[0], **j[1]), jobs))


def _gpu(cuda, b, s, thr, **kw):
    """Kept index lists of ops.batched_nms for [N,4] / [B,N,4] numpy input."""
    from jabd_amd import ops
    b, s = np.asarray(b, np.float32), np.asarray(s, np.float32)
    one = b.ndim == 2
    if one:
        b, s = b[None], s[None]
    keep, nk = ops.batched_nms(torch.from_numpy(b).to(cuda), torch.from_numpy(s).to(cuda), thr, **kw)
    keep, nk = keep.cpu().numpy(), nk.cpu().numpy()
    out = [keep[i, : nk[i]].tolist() for i in range(len(b))]
    return out[0] if one else out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1000, 4096])
def test_diou_parity_sizes(cuda, n):
    b, s = _clustered(max(n, 1), seed=n + 11)
    b, s = b[:n], s[:n]
    assert _gpu(cuda, b, s, 0.3, kind="diou") == R.diounms(b, s, 0.3)[0].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.0, 0.3, 0.5, 0.7, 1.0])
def test_diou_parity_thresholds(cuda, thr):
    b, s = _clustered(3000, seed=7)
    ref = _ref3000(thr, "diou")[0].tolist()
    assert _gpu(cuda, b, s, thr, kind="diounms") == ref
    if thr in (0.3, 0.5):   # 77 / 13 rows apart on this input: the kind matters
        iou = _ref3000(thr, "iou")[0].tolist()
        assert set(iou) != set(ref)
        assert _gpu(cuda, b, s, thr, kind="greedynms") == iou


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.3, 0.5])
def test_diou_grid_producer(cuda, thr):
    """2 x 24k rows: both images on the grid producer (above nms.hip's 20480-row
    dense limit), exact; the DIoU and IoU sets of image 0 differ (1310 / 338
    rows), so a grid producer that ignored the kind would fail."""
    from jabd_amd import ops
    bx, sc = _boxes24k()
    r0, r1, i0 = _ref_many([((bx[0], sc[0], thr), {}), ((bx[1], sc[1], thr), {}),
                            ((bx[0], sc[0], thr), {"kind": "iou"})])
    got = _gpu(cuda, bx, sc, thr, kind="diou")
    assert got[0] == r0[0].tolist() and got[1] == r1[0].tolist()
    assert set(i0[0].tolist()) != set(r0[0].tolist())
    _, _, _, dense = ops.batched_nms_stats(torch.from_numpy(bx).to(cuda),
                                           torch.from_numpy(sc).to(cuda), thr, kind="diou")
    assert dense.tolist() == [False, False]


@pytest.mark.gpu
def test_diou_dense_fallback_in_the_same_call(cuda):
    """Image 0 is test_nms_pair_capacity_dense_fallback's tight cluster (more
    candidate pairs than the workspace holds: dense producer), image 1 ordinary
    clustered boxes on the grid producer, in one call; both exact."""
    from jabd_amd import ops, synth
    n = 24_000
    rng = np.random.default_rng(17)
    ctr = 0.5 + rng.normal(0, 0.002, (n, 2))
    wh = 0.1 * (1 + rng.uniform(0, 0.05, (n, 2)))
    b0 = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)
    s0 = rng.uniform(0.5, 1.0, n).astype(np.float32)
    b1, s1 = synth.nms_boxes(1, n, seed=23)
    bx, sc = np.stack([b0, b1[0]]), np.stack([s0, s1[0]])
    refs = _ref_many([((bx[b], sc[b], 0.3), {}) for b in range(2)])
    got = _gpu(cuda, bx, sc, 0.3, kind="diou")
    for b in range(2):
        assert got[b] == refs[b][0].tolist(), b
    _, _, _, dense = ops.batched_nms_stats(torch.from_numpy(bx).to(cuda),
                                           torch.from_numpy(sc).to(cuda), 0.3, kind="diou")
    assert dense.tolist() == [True, False]


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [False, True])
@pytest.mark.parametrize("thr", [0.3, 0.5])
def test_diou_near_threshold_orientation(cuda, thr, grid):
    """400 nested pairs [x0,y0,x0+1,y0+1], [x0,y0,x0+s,y0+1]: IoU = s, centres
    (1-s)/2 apart, enclosing box the unit square, so DIoU = s - (1-s)^2 / 8;
    s solves DIoU = thr (s = 5 - sqrt(24 - 8 thr)) and is moved by k * 2e-7,
    k in [-8, 8].  Each pair comes in either row order, and the larger box has
    the higher score in half of them: the union (area_j - inter) + area_i
    rounds differently when (i, j) are swapped, which decides pairs this close.
    grid: 210 far-away clusters of 100 equal boxes lift the image over the
    dense-rows limit, so the same pairs are decided by the grid producer (which
    meets a pair from either side)."""
    from jabd_amd import ops
    rng = np.random.default_rng(11)
    s0 = 5.0 - np.sqrt(24.0 - 8.0 * thr)
    rows, scores = [], []
    for k in range(400):
        x0, y0 = rng.uniform(0, 50, 2).astype(np.float32)
        s = np.float32(s0 + rng.integers(-8, 9) * 2e-7)
        pair = [[x0, y0, x0 + 1, y0 + 1], [x0, y0, x0 + s, y0 + 1]]
        sc = [1.0 - k * 1e-3, 0.5 - k * 1e-4]       # the larger box first ...
        if (k >> 1) & 1:
            sc = sc[::-1]                           # ... or the smaller one
        if k & 1:
            pair, sc = pair[::-1], sc[::-1]         # either row order
        rows += pair
        scores += sc
    b = np.asarray(rows, np.float32)
    sc = np.asarray(scores, np.float32)
    if grid:
        fb, fs = _fillers()
        b, sc = np.concatenate([b, fb]), np.concatenate([sc, fs])
    ref, margin = R.diounms(b, sc, thr)
    assert margin < 1e-6        # the case has not gone slack
    near = [i for i in ref.tolist() if i < 800]
    assert 400 < len(near) < 800    # every pair keeps one box; the second ones straddle
    assert _gpu(cuda, b, sc, thr, kind="diou") == ref.tolist()
    if grid:
        _, _, _, dense = ops.batched_nms_stats(torch.from_numpy(b[None]).to(cuda),
                                               torch.from_numpy(sc[None]).to(cuda), thr,
                                               kind="diou")
        assert dense.tolist() == [False]


def _fillers():
    """210 far-away clusters of 100 equal boxes (21 000 rows, 210 kept): they
    lift an image over nms.hip's dense-rows limit at little cost to the
    restatement."""
    rows, scores = [], []
    for c in range(210):
        x, y = 100.0 + 3.0 * (c % 15), 100.0 + 3.0 * (c // 15)
        rows += [[x, y, x + 1, y + 1]] * 100
        scores += [0.4 - 1e-4 * c] * 100
    return np.asarray(rows, np.float32), np.asarray(scores, np.float32)


@functools.lru_cache(maxsize=None)
def _asymmetric_pairs(count=3):
    """Overlapping pairs (A, B) whose fp32 DIoU depends on which box is the
    kept one: (area_B - inter) + area_A and (area_A - inter) + area_B round
    differently.  Found by a seeded search with the restatement itself: at
    thr 0 its margin on a two-box input is the pair's value.  -> [(A, B,
    value with A kept, value with B kept)]."""
    rng = np.random.default_rng(5)
    out = []
    hi, lo = np.float32([0.9, 0.8]), np.float32([0.8, 0.9])
    for _ in range(4000):
        xy = rng.uniform(0, 1, 2)
        a = np.concatenate([xy, xy + rng.uniform(0.1, 0.5, 2)]).astype(np.float32)
        b = (a + rng.uniform(-0.05, 0.05, 4)).astype(np.float32)
        pair = np.stack([a, b])
        va, vb = R.diounms(pair, hi, 0.0)[1], R.diounms(pair, lo, 0.0)[1]
        if va != vb and 0.2 < min(va, vb) and max(va, vb) < 0.9:
            out.append((a, b, va, vb))
            if len(out) == count:
                return out
    raise AssertionError("no order-dependent pair found")


def test_asymmetric_pairs_depend_on_the_kept_box():
    """The inputs of test_diou_pair_orientation really decide on the order:
    with thr between the two values, exactly one score order suppresses."""
    for a, b, va, vb in _asymmetric_pairs():
        thr = (va + vb) / 2
        pair = np.stack([a, b])
        ka = R.diounms(pair, np.float32([0.9, 0.8]), thr)[0].tolist()
        kb = R.diounms(pair, np.float32([0.8, 0.9]), thr)[0].tolist()
        assert sorted((len(ka), len(kb))) == [1, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [False, True])
def test_diou_pair_orientation(cuda, grid):
    """One pair per call whose decision depends on which of its boxes is taken
    as the kept one (thr lies between its two fp32 values), in both score
    orders and both row orders: a producer that evaluated (this lane's box,
    candidate) instead of (lower rank, higher rank) gets one of them wrong.
    grid: the pair sits in an image large enough for the grid producer, which
    meets a pair once, from either side."""
    from jabd_amd import ops
    fb, fs = _fillers()
    for a, b, va, vb in _asymmetric_pairs():
        thr = (va + vb) / 2
        for boxes, sc in ((np.stack([a, b]), [0.9, 0.8]), (np.stack([a, b]), [0.8, 0.9]),
                          (np.stack([b, a]), [0.9, 0.8]), (np.stack([b, a]), [0.8, 0.9])):
            sc = np.float32(sc)
            if grid:
                boxes, sc = np.concatenate([boxes, fb]), np.concatenate([sc, fs])
            ref = R.diounms(boxes, sc, thr)[0].tolist()
            assert _gpu(cuda, boxes, sc, thr, kind="diou") == ref
    if grid:
        _, _, _, dense = ops.batched_nms_stats(torch.from_numpy(boxes[None]).to(cuda),
                                               torch.from_numpy(sc[None]).to(cuda), thr,
                                               kind="diou")
        assert dense.tolist() == [False]


@pytest.mark.gpu
def test_diou_degenerate(cuda):
    # identical boxes, zero-area (point) boxes, all-equal scores, -0.0 vs 0.0
    # scores (test_nms_parity_degenerate's input): the point boxes are all kept
    b = np.float32([[0, 0, 1, 1]] * 5 + [[0.5, 0.5, 0.5, 0.5]] * 3 + [[0, 0, 2, 2], [2, 2, 1, 1]])
    s = np.float32([0.5] * 5 + [0.0, -0.0, 0.0] + [0.5, 0.7])
    for thr in (0.0, 0.3, 0.99):
        ref = R.diounms(b, s, thr)[0].tolist()
        assert {5, 6, 7} <= set(ref)
        assert _gpu(cuda, b, s, thr, kind="diou") == ref, thr


@pytest.mark.gpu
def test_diou_nan_boxes(cuda):
    """test_nms_parity_nan_boxes' input: a NaN coordinate in either box of a
    pair makes the pair non-suppressing (fminf / fmaxf would drop the NaN)."""
    b, s = _clustered(500, seed=3)
    b = b.copy()
    b[7, 0] = np.nan
    b[100, 3] = np.nan
    ref = R.diounms(b, s, 0.3)[0].tolist()
    assert 7 in ref and 100 in ref
    assert _gpu(cuda, b, s, 0.3, kind="diou") == ref


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["iou", "diou"])
@pytest.mark.parametrize("top_k", [1, 200, 5000])
def test_top_k_with_score_filter(cuda, kind, top_k):
    from jabd_amd import synth
    B, n = 3, 5000
    bx, sc = synth.nms_boxes(B, n, seed=3)
    sc = sc - 0.25  # half the rows fall under the 0.5 filter
    got = _gpu(cuda, bx, sc, 0.3, score_threshold=0.5, kind=kind, top_k=top_k)
    for b in range(B):
        m = np.nonzero(sc[b] >= 0.5)[0]
        ref = m[R.diounms(bx[b][m], sc[b][m], 0.3, top_k=top_k, kind=kind)[0]]
        assert got[b] == ref.tolist(), b
    if top_k == 1:
        assert [len(g) for g in got] == [1] * B


@pytest.mark.gpu
def test_top_k_single_image_compacted_keys(cuda):
    """One image above 16 800 rows with the score filter: the compacted-key
    path (nms_keys_compact), whose sorted keys hold the candidates alone."""
    from jabd_amd import synth
    n = 17_000
    bx, sc = synth.nms_boxes(1, n, seed=n, tie_frac=0.05)
    sc = sc - 0.25
    m = np.nonzero(sc[0] >= 0.5)[0]
    assert len(m) > 3000
    for top_k in (300, 0):
        ref = m[R.diounms(bx[0][m], sc[0][m], 0.3, top_k=top_k)[0]]
        got = _gpu(cuda, bx, sc, 0.3, score_threshold=0.5, kind="diou", top_k=top_k)[0]
        assert got == ref.tolist(), top_k


@pytest.mark.gpu
@pytest.mark.parametrize("beta1", [0.5, 2.0])
def test_diou_beta1(cuda, beta1):
    """beta1 != 1 goes through pow on both sides.  A condition, not a
    tolerance: no decision of the restatement lies within 1e-5 of the
    threshold on this input (7.6e-4 at 0.5, 1.7e-4 at 2.0), so a last-place
    difference between the device and host pow cannot flip one, and the lists
    must be equal."""
    b, s = _clustered(3000, seed=7)
    ref, margin = _ref3000(0.3, "diou", beta1)
    assert margin >= 1e-5
    assert ref.tolist() != _ref3000(0.3, "diou")[0].tolist()
    assert _gpu(cuda, b, s, 0.3, kind="diou", beta1=beta1) == ref.tolist()


@pytest.mark.gpu
def test_beta1_and_top_k_on_the_grid_producer(cuda):
    """beta1 != 1 and a top_k cut on an image of the grid producer: the 3000
    clustered rows of test_diou_beta1 ranked above 21 000 filler rows; the cuts
    fall among the fillers, so the count stays above the 8192-candidate gate
    under which an image takes the dense producer.  The margin condition is
    test_diou_beta1's."""
    from jabd_amd import ops
    b, s = _clustered(3000, seed=7)
    fb, fs = _fillers()
    b, s = np.concatenate([b, fb]), np.concatenate([s, fs * np.float32(0.01)])
    for beta1, top_k in ((0.5, 0), (1.0, 22_000), (2.0, 21_000)):
        ref, margin = R.diounms(b, s, 0.3, beta1=beta1, top_k=top_k)
        assert margin >= 1e-5
        assert _gpu(cuda, b, s, 0.3, kind="diou", beta1=beta1, top_k=top_k) == ref.tolist()
        _, _, _, dense = ops.batched_nms_stats(torch.from_numpy(b[None]).to(cuda),
                                               torch.from_numpy(s[None]).to(cuda), 0.3,
                                               kind="diou", beta1=beta1)
        assert dense.tolist() == [False]


@pytest.mark.gpu
def test_utils_bbox_diounms_contract(cuda):
    """utils.utils_bbox.diounms: (keep, count) with keep int64 [N], zero past
    count; non_max_suppression(nms_kind="diounms") gathers the same rows."""
    from utils import utils_bbox
    b, s = _clustered(3000, seed=7)
    ref = R.diounms(b, s, 0.3, top_k=200)[0]
    tb, ts = torch.from_numpy(b).to(cuda), torch.from_numpy(s).to(cuda)
    keep, count = utils_bbox.diounms(tb, ts, 0.3, top_k=200)
    assert keep.dtype == torch.int64 and keep.shape == (3000,) and count == len(ref)
    assert keep[:count].cpu().numpy().tolist() == ref.tolist()
    assert not keep[count:].any()
    det = torch.cat([tb, ts[:, None]], 1)
    m = np.nonzero(s >= 0.5)[0]
    want = m[R.diounms(b[m], s[m], 0.3)[0]]
    rows = utils_bbox.non_max_suppression(det, 0.5, 0.3, nms_kind="diounms")
    assert np.array_equal(rows, det.cpu().numpy()[want])


@pytest.mark.gpu
def test_detect_diounms(cuda):
    """ops.detect(nms_kind="diounms") at A = 16 800 (640^2): its rows equal
    decode, the >= 0.5 filter, the restatement and a gather, composed by hand
    (ops.decode / decode_landm are the same device arithmetic)."""
    from jabd_amd import ops
    from utils.anchors import Anchors
    from utils.config import cfg_mnet
    pri = Anchors(cfg_mnet, image_size=(640, 640)).get_anchors().float().to(cuda)
    A = pri.shape[0]
    assert A == 16800
    g = torch.Generator().manual_seed(16800)
    loc = (torch.randn(2, A, 4, generator=g) * 0.5).to(cuda)
    p1 = torch.rand(2, A, generator=g)
    conf = torch.stack([1 - p1, p1], -1).to(cuda)
    landm = torch.randn(2, A, 10, generator=g).to(cuda)
    var = cfg_mnet["variance"]
    rows, nk = ops.detect(loc, conf, landm, pri, var, 0.5, 0.3, nms_kind="diounms")
    iou_rows, iou_nk = ops.detect(loc, conf, landm, pri, var, 0.5, 0.3)
    det = torch.cat([ops.decode(loc, pri, var), conf[..., 1:2],
                     ops.decode_landm(landm, pri, var)], -1).cpu().numpy()
    for b in range(2):
        m = np.nonzero(det[b][:, 4] >= 0.5)[0]
        assert len(m) > 5000
        ref = m[R.diounms(det[b][m, :4], det[b][m, 4], 0.3)[0]]
        assert int(nk[b]) == len(ref)
        assert np.array_equal(rows[b, : len(ref)].cpu().numpy(), det[b][ref])
    assert nk.tolist() != iou_nk.tolist()


@pytest.mark.gpu
def test_detect_image_diounms_graph(cuda, monkeypatch):
    """detect_image(nms_kind="diounms") on a weights_init MNv3 at 320^2: the
    graphed path (captured by the first call, replayed by the second) equals
    the eager path, and a following greedynms call gets the IoU result, not a
    replay of the DIoU graph (the rule is part of the graph cache key)."""
    import bench
    from jabd_amd import predict
    net, cfg = bench._weights_init_model("mnv3")
    net = net.eval().to(cuda)
    img = np.random.default_rng(320).integers(0, 256, (240, 320, 3)).astype(np.float32)
    args = (net, img, (320, 320), cfg)
    assert predict.PREDICT_GRAPH
    first = predict.detect_image(*args, nms_kind="diounms")
    replay = predict.detect_image(*args, nms_kind="diounms")
    greedy = predict.detect_image(*args, nms_kind="greedynms")
    assert len(net.__dict__["_jabd_graphs"]) == 2
    monkeypatch.setattr(predict, "PREDICT_GRAPH", False)
    eager = predict.detect_image(*args, nms_kind="diounms")
    eager_greedy = predict.detect_image(*args)
    assert len(eager) > 0
    assert np.array_equal(first, eager) and np.array_equal(replay, eager)
    assert np.array_equal(greedy, eager_greedy)
    assert greedy.shape != eager.shape or not np.array_equal(greedy, eager)
