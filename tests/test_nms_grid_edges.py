"""Edges of csrc/nms.hip's grid producer and pull scan that clustered boxes in
[0, 1] never reach: incoming lists at and above the pull scan's pair ring,
every dense-fallback flag and its boundary, inactive boxes, signed pixel
coordinates, the extreme thresholds, top_k / score filter / n_valid on the
grid, several sort passes, and the score order of hard NMS.

Every device result is an index list compared with oracle/box_ref.nms
(oracle/nms_ref.c), or tests/_diou_ref.py for the DIoU kind: equal or not, no
tolerance.  Every call of at most 254 images goes through
ops.batched_nms_stats(return_flags=True): jabd_nms_pair_stats is the one
reader of the pull scan's time-out word, so a timed-out scan raises here, and
the producer word of each image (include/jabd.h) is asserted as named.

The CPU tests are conditions on the inputs (tests/_nms_edge_inputs.py), not
measurements of the kernel: they show that the inputs reach the branch they
are meant for."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import _diou_ref as R
import _nms_edge_inputs as E
from oracle import box_ref

N = E.N


# ----------------------------------------------------------------------------- shared inputs
@functools.lru_cache(maxsize=None)
def _built(name):
    b, s = getattr(E, name)()
    b.setflags(write=False)
    s.setflags(write=False)
    return b, s


@functools.lru_cache(maxsize=None)
def _synth(n=N, seed=31, batch=1):
    from jabd_amd import synth
    b, s = synth.nms_boxes(batch, n, seed=seed)
    b.setflags(write=False)
    s.setflags(write=False)
    return b, s


def _ref_one(b, s, thr, kind="iou", score_threshold=None, n_valid=None, top_k=0):
    """The reference for one image: the rows that pass the filter and lie under
    n_valid, cut to the stable top k, then the oracle on those rows."""
    m = np.arange(len(s))
    if n_valid is not None:
        m = m[:n_valid]
    if score_threshold is not None:
        m = m[s[m] >= np.float32(score_threshold)]   # NaN fails, as the device's s >= thr
    if top_k > 0:
        m = np.sort(m[E.order_desc(s[m])[:top_k]])
    if len(m) == 0:
        return []
    if kind == "iou":
        k = box_ref.nms(b[m], s[m], thr)
    else:
        k = R.diounms_c(b[m], s[m], thr)[0]
    return m[k].tolist()


def _ref(bx, sc, thr, n_valid=None, **kw):
    """_ref_one per image, in threads (both C references drop the GIL)."""
    nv = [None] * len(bx) if n_valid is None else list(n_valid)
    with ThreadPoolExecutor(max_workers=min(len(bx), 8)) as ex:
        return list(ex.map(lambda i: _ref_one(bx[i], sc[i], thr, n_valid=nv[i], **kw),
                           range(len(bx))))


def _run(cuda, bx, sc, thr, n_valid=None, **kw):
    """-> (kept lists, n_keep list, producer words list) of batched_nms_stats."""
    from jabd_amd import ops
    if n_valid is not None:
        n_valid = torch.tensor(list(n_valid), dtype=torch.int64, device=cuda)
    keep, nk, _, flags = ops.batched_nms_stats(
        torch.tensor(bx, dtype=torch.float32, device=cuda),
        torch.tensor(sc, dtype=torch.float32, device=cuda), thr, n_valid=n_valid,
        return_flags=True, **kw)
    keep, nk = keep.cpu().numpy(), nk.cpu().numpy()
    return [keep[i, : nk[i]].tolist() for i in range(len(bx))], nk.tolist(), flags.tolist()


def _check(got, ref, what=""):
    for i, (g, r) in enumerate(zip(got, ref)):
        assert len(g) == len(r), (what, i, len(g), len(r))
        assert g == r, (what, i)


def _stack(*pairs):
    return np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])


# ----------------------------------------------------------------------------- CPU: the builders
def test_stats_call_takes_batched_nms_arguments():
    """ops.batched_nms_stats is batched_nms' signature (names, order, defaults)
    plus return_flags=False, so a test swaps one for the other."""
    import inspect
    from jabd_amd import ops
    nms = list(inspect.signature(ops.batched_nms).parameters.values())
    stats = list(inspect.signature(ops.batched_nms_stats).parameters.values())
    assert stats[:len(nms)] == nms
    assert [(p.name, p.default) for p in stats[len(nms):]] == [("return_flags", False)]


def test_pair_predicate_agrees_with_the_references():
    """E.suppresses (what cluster_incoming counts) decides two-box inputs as
    the two references do, for either order of the pair."""
    rng = np.random.default_rng(0)
    for _ in range(200):
        xy = rng.uniform(0, 1, 2)
        a = np.concatenate([xy, xy + rng.uniform(0.1, 0.5, 2)]).astype(np.float32)
        b = (a + rng.uniform(-0.12, 0.12, 4)).astype(np.float32)
        for first, second in ((a, b), (b, a)):
            pair, s = np.stack([first, second]), np.float32([0.9, 0.8])
            assert E.suppresses(first, second, 0.5)[0, 0] == (len(box_ref.nms(pair, s, 0.5)) == 1)
            assert E.suppresses(first, second, 0.5, "diou")[0, 0] == \
                (len(R.diounms(pair, s, 0.5)[0]) == 1)


@pytest.mark.parametrize("kind", ["iou", "diou"])
def test_chain_cluster_reaches_the_ring_paths(kind):
    """chain_cluster at its defaults, under either kind's predicate: incoming
    lists above the 16384-entry ring and between 64 and the ring, a greedy
    result inside the chain that is not the best row alone, and few enough
    off-block pairs for the image's overflow region.  (IoU: lists up to 21537,
    4 above the ring, 11 between, 4 rows kept, 621 suppressed by a row other
    than the best, 172 608 off-block pairs against 327 696.  DIoU: up to 19948,
    3 / 12, 5 kept, 655, 159 135.)"""
    b, s = _built("chain_cluster")
    rows = E.cluster_rows(s)
    assert len(rows) == 1024
    assert E.order_desc(s[0])[:1024].tolist() == rows.tolist()   # ranks 0..M-1
    inc = E.cluster_incoming(b, s, rows, 0.5, kind)
    assert (inc > E.RING).sum() >= 1
    assert ((inc > 64) & (inc <= E.RING)).sum() >= 1
    assert inc.sum() < E.OVF_PER_BOX * N
    kept = np.intersect1d(_ref_one(b[0], s[0], 0.5, kind), rows)
    assert len(kept) >= 3
    _, S = E.cluster_pairs(b, s, rows, 0.5, kind)
    by_best = int(S[0].sum())             # rows the best row suppresses itself
    assert len(rows) - len(kept) - by_best >= 100


def test_solid_cluster_fills_the_ring_exactly():
    b, s = _built("solid_cluster")
    rows = E.cluster_rows(s)
    assert E.order_desc(s[0])[:448].tolist() == rows.tolist()
    inc = E.cluster_incoming(b, s, rows, 0.5)
    assert inc.tolist() == [0, 4096, 8192, 12288, 16384, 20480, 24576]
    assert inc[4] == E.RING
    assert inc.sum() < E.OVF_PER_BOX * N


def test_far_and_inactive_rows_neither_suppress_nor_are_suppressed():
    """The oracle keeps every far and every inactive row, and taking those
    rows out changes nothing else of its result: they suppress nothing."""
    for name, count in (("far_tiny", 32), ("inactive_mix", 4 * 204), ("all_inactive", N)):
        b, s = _built(name)
        special = E.far_rows(b) if name == "far_tiny" else E.inactive_rows(b)
        assert len(special) == count, name
        keep = box_ref.nms(b[0], s[0], 0.5)
        assert np.isin(special, keep).all(), name
        rest = np.setdiff1d(np.arange(N), special)
        if len(rest):
            alone = rest[box_ref.nms(b[0][rest], s[0][rest], 0.5)]
            assert alone.tolist() == keep[~np.isin(keep, special)].tolist(), name
    b, _ = _built("inactive_mix")
    assert np.isinf(b).any() and not np.isnan(b).any()


def test_signed_and_sparse_inputs_are_what_they_claim():
    for kw in ({}, {"smin": 1.0}):
        b, _ = E.signed_pixels(**kw)
        ctr, wh = (b[0, :, :2] + b[0, :, 2:]) / 2, b[0, :, 2:] - b[0, :, :2]
        assert (ctr.min(0) < -900).all() and (ctr.max(0) > 900).all()
        assert (wh > 0).all() and wh.max() / wh.min() > 500
    b, _ = _built("sparse_small")
    wh = b[0, :, 2:] - b[0, :, :2]
    assert (wh > 0).all() and wh.max() <= 0.0101


# ----------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_ring_paths_iou(cuda):
    """Case 1: chain_cluster (lists above the ring: the scan wave reads them
    from HBM; lists under it with more than 64 late pairs), solid_cluster (a
    list of exactly the ring's size) and plain clustered boxes in one call."""
    bx, sc = _stack(_built("chain_cluster"), _built("solid_cluster"), _synth())
    got, nk, flags = _run(cuda, bx, sc, 0.5)
    print("ring paths iou: flags", flags, "n_keep", nk)
    _check(got, _ref(bx, sc, 0.5))
    assert flags == [0, 0, 0]


@pytest.mark.gpu
def test_ring_paths_diou(cuda):
    """Case 1, DIoU kind: the chain image, whose lists exceed the ring under
    the DIoU predicate too (test_chain_cluster_reaches_the_ring_paths[diou])."""
    bx, sc = _built("chain_cluster")
    got, nk, flags = _run(cuda, bx, sc, 0.5, kind="diou")
    print("ring paths diou: flags", flags, "n_keep", nk)
    _check(got, _ref(bx, sc, 0.5, kind="diou"))
    assert flags == [0]


@pytest.mark.gpu
def test_row_limit_boundary(cuda):
    """Case 2: 20480 rows run no grid producer (word 1 for the image), 20481
    rows do (word 0)."""
    bx, sc = _synth()
    words = []
    for n in (N - 1, N):
        got, nk, flags = _run(cuda, bx[:, :n], sc[:, :n], 0.5)
        print("row limit: n", n, "flags", flags, "n_keep", nk)
        _check(got, _ref(bx[:, :n], sc[:, :n], 0.5), n)
        words.append(flags[0])
    assert words[0] != 0 and words[1] == 0


@pytest.mark.gpu
def test_candidate_limit_boundary(cuda):
    """Case 3: the score filter leaves exactly 8192 candidates (word 8: the
    dense producer) and exactly 8193 (word 0: the grid)."""
    bx, sc = _synth()
    rows = np.random.default_rng(3).permutation(N)
    words = []
    for cand in (8192, 8193):
        s = sc.copy()
        s[0, rows[cand:]] -= np.float32(0.5)
        assert int((s[0] >= np.float32(0.5)).sum()) == cand
        got, nk, flags = _run(cuda, bx, s, 0.5, score_threshold=0.5)
        print("candidate limit:", cand, "flags", flags, "n_keep", nk)
        _check(got, _ref(bx, s, 0.5, score_threshold=0.5), cand)
        words.append(flags[0])
    assert words == [8, 0]


@pytest.mark.gpu
def test_cell_index_out_of_range_beside_a_grid_image(cuda):
    """Case 4: far_tiny's 1e-4 boxes at x = y = 50 are cell 1.4e6 (word 2), the
    image beside it stays on the grid."""
    bx, sc = _stack(_built("far_tiny"), _synth())
    got, nk, flags = _run(cuda, bx, sc, 0.5)
    print("far tiny: flags", flags, "n_keep", nk)
    _check(got, _ref(bx, sc, 0.5))
    assert flags == [2, 0]


@pytest.mark.gpu
def test_inactive_boxes_on_the_grid(cuda):
    """Case 5: zero-width, inverted, infinite and area-overflow boxes get no
    grid key; an image of such boxes alone in the middle of the batch and as
    the last image of the key order (istart[] of the count sort)."""
    bx, sc = _stack(_built("inactive_mix"), _built("all_inactive"), _synth(),
                    _built("all_inactive"))
    got, nk, flags = _run(cuda, bx, sc, 0.5)
    print("inactive: flags", flags, "n_keep", nk)
    _check(got, _ref(bx, sc, 0.5))
    assert nk[1] == N and nk[3] == N
    assert flags == [0, 0, 0, 0]


@functools.lru_cache(maxsize=None)
def _signed(smin):
    return E.signed_pixels(smin=smin)


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.3, 0.7])
def test_signed_pixel_coordinates(cuda, thr):
    """Case 6: centres in [-1024, 1024]^2 (negative cell coordinates), extents
    over three decades (tens of size classes per axis), on the grid.  The cell
    of a box is its centre over about f x its extent, f = (1 - thr) / (1 + thr),
    and the grid keys hold +-2^14 cells: at 1024 px an extent under 0.34 px
    (thr 0.7) is out of range by construction, which is word 2's case, so the
    on-grid image draws its extents from [1, 1e3].  The same builder with
    extents from 1e-3 runs beside it for exactness, whatever its producer."""
    bx, sc = _stack(_signed(1.0), _signed(1e-3))
    got, nk, flags = _run(cuda, bx, sc, thr)
    print("signed pixels: thr", thr, "flags", flags, "n_keep", nk)
    _check(got, _ref(bx, sc, thr), thr)
    assert flags[0] == 0
    assert 0 < nk[0] < N and 0 < nk[1] < N


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.0, 1e-3, 1.0, 1.5])
def test_threshold_sweep_on_the_grid(cuda, thr):
    """Case 7: thr 0 (no ratio pruning, one size class), a tiny thr, 1 (cell
    scale clamped to 0.05) and above 1 (class width clamped) with sparse_small
    on the grid; plain clustered boxes beside it for exactness, whatever their
    producer."""
    bx, sc = _stack(_built("sparse_small"), _synth())
    got, nk, flags = _run(cuda, bx, sc, thr)
    print("threshold sweep: thr", thr, "flags", flags, "n_keep", nk)
    _check(got, _ref(bx, sc, thr), thr)
    assert flags[0] == 0
    if thr >= 1.0:
        assert nk == [N, N]


@pytest.mark.gpu
@pytest.mark.parametrize("top_k", [0, 9000])
def test_top_k_filter_and_n_valid_on_the_grid(cuda, top_k):
    """Case 8, IoU kind: three images with the score filter, n_valid =
    [n, 15000, 0] and a top_k above the 8192-candidate gate.  Scores are shifted
    by 0.15 (0.25 would leave image 1 about 7500 candidates, under the gate)."""
    bx, sc = _synth(seed=37, batch=3)
    sc = sc - np.float32(0.15)
    nv = [N, 15000, 0]
    cand = [int((sc[i, : nv[i]] >= np.float32(0.5)).sum()) for i in range(3)]
    assert cand[0] > 9000 and cand[1] > 9000 and cand[2] == 0
    got, nk, flags = _run(cuda, bx, sc, 0.3, n_valid=nv, score_threshold=0.5, top_k=top_k)
    print("top_k / filter / n_valid: top_k", top_k, "candidates", cand, "flags", flags,
          "n_keep", nk)
    _check(got, _ref(bx, sc, 0.3, n_valid=nv, score_threshold=0.5, top_k=top_k), top_k)
    assert flags == [0, 0, 8] and nk[2] == 0


@pytest.mark.gpu
def test_multi_pass_batch(cuda):
    """Case 9: 300 images make two sort passes (254 + 46); per-image n_valid
    cycling through {0, 1, 64, 65} and a score filter.  Every image differs, so
    a wrong image offset in scores, boxes, n_valid, keep or n_keep shows."""
    from jabd_amd import ops, synth
    B, n = 300, 65
    bx, sc = synth.nms_boxes(B, n, seed=41, centres=8)
    nv = [(0, 1, 64, 65)[i % 4] for i in range(B)]
    keep, nk = ops.batched_nms(torch.from_numpy(bx).to(cuda), torch.from_numpy(sc).to(cuda), 0.3,
                               score_threshold=0.6,
                               n_valid=torch.tensor(nv, dtype=torch.int64, device=cuda))
    keep, nk = keep.cpu().numpy(), nk.cpu().numpy()
    ref = [_ref_one(bx[i], sc[i], 0.3, score_threshold=0.6, n_valid=nv[i]) for i in range(B)]
    print("multi pass: n_keep sum", int(nk.sum()), "max", int(nk.max()))
    assert nk.tolist() == [len(r) for r in ref]
    for i in range(B):
        assert keep[i, : nk[i]].tolist() == ref[i], i
    assert sum(len(r) < v for r, v in zip(ref, nv)) > 100    # the filter and the NMS both cut
    assert len({tuple(r) for r in ref[3::4]}) > 60           # the images do differ


_ODD_SCORES = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-40, 0.5, -0.5]


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 2])
def test_hard_nms_score_order(cuda, batch):
    """Case 10: 200 disjoint boxes, so the kept list is the sort order: NaN
    first, then +inf ... -inf, -0.0 tied with 0.0, denormals in place, ties by
    row.  One image takes nms_keys_compact and the counted sort, two take
    nms_keys.  With score_threshold 0 the filter s >= thr drops NaN, the
    negatives and the negative denormal, and keeps -0.0."""
    n = 200
    k = np.arange(n)
    boxes = np.stack([2.0 * (k % 20), 2.0 * (k // 20), 2.0 * (k % 20) + 1, 2.0 * (k // 20) + 1],
                     1).astype(np.float32)
    rng = np.random.default_rng(10)
    sc = np.float32(_ODD_SCORES)[rng.integers(0, len(_ODD_SCORES), (batch, n))]
    bx = np.stack([boxes] * batch)
    for st in (None, 0.0):
        kw = {} if st is None else {"score_threshold": st}
        got, nk, flags = _run(cuda, bx, sc, 0.5, **kw)
        ref = _ref(bx, sc, 0.5, score_threshold=st)
        print("score order: batch", batch, "score_threshold", st, "flags", flags, "n_keep", nk)
        _check(got, ref, st)
        assert nk == ([n] * batch if st is None else
                      [int(((sc[i] >= 0) & ~np.isnan(sc[i])).sum()) for i in range(batch)])
        assert flags == [1] * batch
    assert np.isnan(sc[0, _ref(bx, sc, 0.5)[0][0]])           # NaN rows rank first


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [-0.1, -1.0])
def test_negative_thresholds(cuda, thr):
    """Case 11, IoU kind: the dense producer's exact loop (thr < 0: disjoint
    boxes suppress, IoU 0 > thr), with two NaN boxes and two zero-area boxes
    (IoU 0 / 0 between them)."""
    from jabd_amd import synth
    bx, sc = synth.nms_boxes(1, 200, seed=11, centres=20)
    bx = bx.copy()
    bx[0, 5, 0] = bx[0, 120, 3] = np.nan
    bx[0, 40] = bx[0, 41] = np.float32([0.5, 0.5, 0.5, 0.5])
    first = sc.copy()
    first[0, 40] = 2.0           # a zero-area box ranks first: its twin (0 / 0) survives it
    for name, s in (("as drawn", sc), ("zero-area first", first)):
        got, nk, flags = _run(cuda, bx, s, thr)
        print("negative threshold:", thr, name, "flags", flags, "n_keep", nk)
        _check(got, _ref(bx, s, thr), (thr, name))
        assert {5, 120} <= set(got[0])                        # a NaN IoU never suppresses
        assert flags == [1]
    assert got[0][0] == 40 and sorted(got[0]) == [5, 40, 41, 120]
