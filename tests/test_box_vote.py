"""Box voting (jabd_box_vote_f32) through jabd_amd.ops and utils.utils_bbox
against tests/_vote_ref.py, the numpy restatement of the rule in jabd.h.

Seeds, votes, owners, the result order, the score column and the columns from
5 on are integer facts or copies and must equal the oracle exactly (the fp32
IoU is the same operations in the same order on both sides).  A box coordinate
is float32(S_k / S) with S_k = sum score*coord and S = sum score accumulated in
float64: the products are exact, each sum carries a relative error of at most
votes * 2^-53 whatever the order (the test coordinates are non-negative:
nothing cancels), so device and oracle can differ in the final rounding to
fp32 only: 1 ulp."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _vote_ref as V
from test_soft_nms import _clustered

LDS, WS = ("box_vote_lds", 1), ("box_vote_ws", 2)
LDS_ROWS = 6656      # the kernel's LDS-state bound on n (jabd.h)


def _rows(b, s, cols=5, seed=0):
    r = np.random.default_rng(seed).uniform(0, 1, (len(s), cols)).astype(np.float32)
    r[:, :4], r[:, 4] = b, s
    return r


# ------------------------------------------------------------------ CPU: the oracle's KATs
def test_kat_iou_exactly_at_the_threshold_merges():
    # offset 0: inter 5 x 10 = 50, union 100 + 100 - 50 -> fp32(50 / 150) == fp32(1 / 3)
    r = np.float32([[0, 0, 10, 10, 0.9], [5, 0, 15, 10, 0.3]])
    got = V.vote(r, thresh=1 / 3, offset=0.0)
    assert got["votes"].tolist() == [2] and got["seeds"].tolist() == [0]
    assert got["margin"] == 0.0
    want_x1 = np.float32((0.9 * 0 + float(np.float32(0.3)) * 5) /
                         (float(np.float32(0.9)) + float(np.float32(0.3))))
    assert got["rows"][0, 0] == want_x1 and got["rows"][0, 1] == 0 and got["rows"][0, 4] == r[0, 4]
    above = V.vote(r, thresh=float(np.nextafter(np.float32(1 / 3), np.float32(1))), offset=0.0)
    assert above["votes"].tolist() == [1, 1]


def test_kat_min_votes_drops_a_singleton():
    r = np.float32([[0, 0, 10, 10, 0.9], [1, 0, 11, 10, 0.8], [100, 100, 110, 110, 0.85]])
    got = V.vote(r, min_votes=2)
    assert got["seeds"].tolist() == [0] and got["votes"].tolist() == [2]
    assert got["owner"].tolist() == [0, 0, -1]


def test_kat_max_out_cuts_after_filtering():
    # clusters in seed order: {0, 1} (2 votes), {4} (dropped by min_votes), {2, 3}, {5, 6}
    r = np.float32([[0, 0, 10, 10, 0.9], [1, 0, 11, 10, 0.2], [50, 0, 60, 10, 0.7],
                    [51, 0, 61, 10, 0.3], [100, 0, 110, 10, 0.8], [150, 0, 160, 10, 0.6],
                    [151, 0, 161, 10, 0.5]])
    got = V.vote(r, min_votes=2, max_out=2)
    assert got["seeds"].tolist() == [0, 2] and got["votes"].tolist() == [2, 2]
    assert got["owner"].tolist() == [0, 0, 1, 1, -1, -1, -1]
    assert V.vote(r, min_votes=2, max_out=0)["seeds"].tolist() == [0, 2, 5]


def test_kat_equal_scores_seed_the_lower_row():
    r = np.float32([[50, 0, 60, 10, 0.5], [0, 0, 10, 10, 0.7], [1, 0, 11, 10, 0.7]])
    got = V.vote(r)
    assert got["seeds"].tolist() == [1, 0] and got["votes"].tolist() == [2, 1]
    assert got["rows"][0, 0] == np.float32(0.5)      # equal weights: the mean


def test_kat_nan_coordinate_joins_no_cluster_but_seeds_its_own():
    r = np.float32([[0, 0, 10, 10, 0.9], [0, 0, 10, np.nan, 0.8], [1, 0, 11, 10, 0.7]])
    got = V.vote(r)
    assert got["seeds"].tolist() == [0, 1] and got["votes"].tolist() == [2, 1]
    assert got["owner"].tolist() == [0, 1, 0]
    assert np.isnan(got["rows"][1, 3]) and got["rows"][1, 4] == np.float32(0.8)


def test_kat_nan_score_is_dropped():
    r = np.float32([[0, 0, 10, 10, np.nan], [0, 0, 10, 10, 0.5]])
    got = V.vote(r)
    assert got["seeds"].tolist() == [1] and got["votes"].tolist() == [1]
    assert got["owner"].tolist() == [-1, 0]


def test_kat_three_identical_boxes_give_the_identical_box():
    r = np.float32([[3, 7, 41, 59, 0.3], [3, 7, 41, 59, 0.9], [3, 7, 41, 59, 0.6]])
    got = V.vote(r)
    assert got["seeds"].tolist() == [1] and got["votes"].tolist() == [3]
    assert got["rows"][0].tolist() == [3, 7, 41, 59, np.float32(0.9)]


@pytest.mark.parametrize("n,offset", [(300, 1.0), (300, 0.0), (2000, 1.0)])
def test_oracle_boxes_do_not_depend_on_the_member_order(n, offset):
    """The ground the 1-ulp bound stands on, checked on the GPU tests' inputs:
    float64 accumulation in three random member orders rounds to the same
    fp32 boxes; the cases hold merged clusters and singletons."""
    b, s = _clustered(n, seed=1, scale=1.0 if offset else 1.0 / 700)
    base = V.vote(_rows(b, s), offset=offset)
    assert (base["votes"] >= 2).any() and (base["votes"] == 1).any() and base["margin"] > 0
    rng = np.random.default_rng(0)
    for _ in range(3):
        got = V.vote(_rows(b, s), offset=offset, member_order=rng)
        assert got["seeds"].tolist() == base["seeds"].tolist()
        assert int(V.ulp_diff(got["rows"][:, :4], base["rows"][:, :4]).max()) <= 1


def test_unmirror_is_an_involution_on_exact_values():
    r = (np.random.default_rng(0).integers(0, 65, (6, 15)) / 64).astype(np.float32)
    m = V.unmirror(r)
    assert m[0, 0] == 1 - r[0, 2] and m[0, 5] == 1 - r[0, 7] and m[0, 6] == r[0, 8]
    assert m[0, 9] == 1 - r[0, 9] and m[0, 11] == 1 - r[0, 13] and m[0, 14] == r[0, 12]
    assert np.array_equal(V.unmirror(m), r)


# ------------------------------------------------------------------ CPU: argument checks, ABI
def test_bad_arguments_raise_before_the_library_is_touched(monkeypatch):
    from jabd_amd import _lib, ops

    def absent(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(ops, "call", absent)
    monkeypatch.setattr(_lib, "lib", absent)
    rows = torch.zeros(1, 3, 5)           # a CPU tensor: never reached
    for kw in ({"vote_threshold": math.nan}, {"offset": math.inf}, {"offset": math.nan},
               {"min_votes": 0}, {"min_votes": -3}):
        with pytest.raises(ValueError):
            ops.box_vote(rows, **kw)
    with pytest.raises(ValueError):
        ops.box_vote(torch.zeros(1, 3, 4))            # fewer than 5 columns
    with pytest.raises(ValueError):
        ops.box_vote(torch.zeros(3, 5))               # no batch dimension
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.box_vote(rows)                            # good arguments, CPU tensor


def test_c_entry_points_return_einval():
    from jabd_amd import _lib
    h = _lib.lib()

    def vote(thr=0.4, offset=1.0, cols=5, min_votes=1, batch=1, n=5, stride=None):
        stride = cols if stride is None else stride
        return h.jabd_box_vote_f32(None, stride, 0, cols, None, batch, n, thr, offset, 0.0,
                                   min_votes, 0, None, None, None, None, None, None, 0, None)
    for batch, n in ((1, 5), (0, 0), (2, 0)):
        for kw in ({"thr": math.nan}, {"offset": math.inf}, {"offset": math.nan}, {"cols": 4},
                   {"min_votes": 0}, {"n": 1 << 24}, {"stride": 4}):
            assert vote(**{"batch": batch, "n": n, **kw}) == 1, (batch, n, kw)
            assert "box_vote" in _lib.last_error()
    assert vote(batch=0, n=0) == 0 and vote(batch=0, n=7) == 0      # launches nothing
    out = ctypes.c_size_t(7)
    assert h.jabd_box_vote_workspace_size(2, 100, ctypes.byref(out)) == 0 and out.value == 0
    assert h.jabd_box_vote_workspace_size(2, LDS_ROWS + 1, ctypes.byref(out)) == 0
    assert out.value >= 2 * (LDS_ROWS + 1) * 24
    assert h.jabd_box_vote_workspace_size(-1, 100, ctypes.byref(out)) == 1
    assert h.jabd_tta_collect_f32(None, None, 4, None, 4, None, 0, 8, 8, 8, 8, 1, 0, None) == 1
    assert h.jabd_tta_collect_f32(None, None, 4, None, 4, None, -1, 8, 8, 8, 8, 1, 0, None) == 1


def test_new_names_are_declared_everywhere():
    import os
    from conftest import ROOT
    from jabd_amd import _lib
    header = open(os.path.join(ROOT, "include", "jabd.h")).read()
    for name in ("jabd_box_vote_workspace_size", "jabd_box_vote_f32", "jabd_tta_collect_f32"):
        assert name in _lib.SIGNATURES and name + "(" in header
    assert len(_lib.SIGNATURES["jabd_box_vote_f32"]) == 20
    assert len(_lib.SIGNATURES["jabd_tta_collect_f32"]) == 14


# ------------------------------------------------------------------ GPU: device against the oracle
def _check(cuda, rows, n_valid=None, form=None, **kw):
    """ops.box_vote on [B, N, C] rows, twice (bit-identical), against the oracle
    image by image.  Returns the oracle's results."""
    from jabd_amd import _lib, ops
    rows = np.asarray(rows, np.float32)
    B, N, C = rows.shape
    nv = None if n_valid is None else torch.tensor(n_valid, dtype=torch.int64, device=cuda)
    t = torch.from_numpy(rows).to(cuda)
    _lib.launch_log_reset()
    first = ops.box_vote(t, n_valid=nv, return_owner=True, **kw)
    log = _lib.launch_log()
    again = ops.box_vote(t, n_valid=nv, return_owner=True, **kw)
    if form is not None and B > 0:
        assert log == [form]
    out, n_out, seed, votes, owner = (x.cpu().numpy() for x in first)
    assert out.shape == (B, N, C) and seed.shape == votes.shape == owner.shape == (B, N)
    assert np.array_equal(t.cpu().numpy(), rows, equal_nan=True)     # the input is not modified
    refs = []
    okw = {"thresh": kw.get("vote_threshold", 0.4), "offset": kw.get("offset", 1.0),
           "score_threshold": kw.get("score_threshold", -np.inf),
           "min_votes": kw.get("min_votes", 1), "max_out": kw.get("max_out", 750)}
    for b in range(B):
        ref = V.vote(rows[b], n_valid=None if n_valid is None else n_valid[b], **okw)
        k = int(n_out[b])
        nmax = int(ref["votes"].max()) if len(ref["votes"]) else 0
        print(f"image {b}: n={N} rows={k} max votes={nmax} margin={ref['margin']:.3e}")
        assert k == len(ref["seeds"]), (b, k, len(ref["seeds"]))
        assert seed[b, :k].tolist() == ref["seeds"].tolist(), b
        assert votes[b, :k].tolist() == ref["votes"].tolist(), b
        assert owner[b].tolist() == ref["owner"].tolist(), b
        assert out[b, :k, 4:].tobytes() == ref["rows"][:, 4:].tobytes(), b
        ulp = V.ulp_diff(out[b, :k, :4], ref["rows"][:, :4])
        print(f"image {b}: max box ulp {int(ulp.max()) if k else 0}")
        assert k == 0 or int(ulp.max()) <= 1, b
        refs.append(ref)
    # the second call: every bit again (rows past n_out are not written)
    out2, n_out2, seed2, votes2, owner2 = (x.cpu().numpy() for x in again)
    assert n_out2.tolist() == n_out.tolist() and owner2.tobytes() == owner.tobytes()
    for b in range(B):
        k = int(n_out[b])
        for a, c in ((out, out2), (seed, seed2), (votes, votes2)):
            assert a[b, :k].tobytes() == c[b, :k].tobytes(), b
    return refs


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0.0, 1.0])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 300, 2000])
def test_row_counts_around_the_wave_size_and_clustered_images(cuda, n, offset):
    """Clustered boxes with a duplicate row and a three-way score tie (n >= 30);
    offset 0 on normalised boxes (scale 1/700), 1 on pixel boxes."""
    b, s = _clustered(n, seed=n, scale=1.0 if offset else 1.0 / 700)
    ref, = _check(cuda, _rows(b, s)[None], offset=offset, max_out=0, form=LDS if n else None)
    assert len(ref["seeds"]) >= min(n, 1)
    if n >= 300:
        assert (ref["votes"] >= 2).any() and (ref["votes"] == 1).any()
        assert ref["margin"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n,form", [(LDS_ROWS, LDS), (LDS_ROWS + 1, WS)])
def test_each_side_of_the_state_form_switch(cuda, n, form):
    """The state is in LDS up to n = 6656 (the largest dynamic LDS the kernel
    asks for) and in the workspace above; the witness names the form."""
    b, s = _clustered(n, seed=3)
    ref, = _check(cuda, _rows(b, s, cols=15)[None], form=form)
    assert len(ref["seeds"]) == 750                       # the default max_out cuts
    assert (ref["votes"] >= 2).any() and (ref["votes"] == 1).any()
    assert (ref["owner"] == -1).any()


@pytest.mark.gpu
def test_batch_n_valid_threshold_and_15_columns(cuda):
    """B = 3 images of 15-column rows with n_valid 200 / 0 / 500 of 500 and a
    score threshold that cuts about a third of the rows."""
    rows = np.stack([_rows(*_clustered(500, seed=20 + i), cols=15, seed=i) for i in range(3)])
    refs = _check(cuda, rows, n_valid=[200, 0, 500], score_threshold=0.35, form=LDS)
    assert len(refs[1]["seeds"]) == 0 and 0 < len(refs[0]["seeds"]) < len(refs[2]["seeds"])
    for ref in (refs[0], refs[2]):
        assert (ref["votes"] >= 2).any() and (ref["votes"] == 1).any()
    assert (refs[2]["owner"] == -1).sum() >= (rows[2, :, 4] < 0.35).sum() > 100


@pytest.mark.gpu
def test_min_votes_and_max_out(cuda):
    b, s = _clustered(800, seed=6)
    rows = _rows(b, s, cols=7)[None]
    all_, = _check(cuda, rows, max_out=0, form=LDS)
    two, = _check(cuda, rows, min_votes=2, max_out=0, form=LDS)
    assert two["seeds"].tolist() == all_["seeds"][all_["votes"] >= 2].tolist()
    assert 0 < len(two["seeds"]) < len(all_["seeds"])
    cut, = _check(cuda, rows, min_votes=2, max_out=17, form=LDS)
    assert cut["seeds"].tolist() == two["seeds"][:17].tolist()
    assert (cut["owner"] >= 0).sum() == cut["votes"].sum() < (two["owner"] >= 0).sum()
    _check(cuda, rows, vote_threshold=2.0, max_out=0, form=LDS)      # no pair merges
    everything, = _check(cuda, rows, vote_threshold=-1.0, form=LDS)   # one cluster
    assert everything["votes"].tolist() == [800]


@pytest.mark.gpu
def test_nan_boxes_ties_and_duplicates(cuda):
    """Few distinct scores and every box twice: the lower row seeds; NaN
    coordinates seed clusters of their own."""
    b, s = _clustered(400, seed=5, ties=False)
    b = np.tile(b, (2, 1))
    s = np.tile(np.round(s * 8) / 8 + np.float32(0.125), 2).astype(np.float32)
    b[5, 2] = b[77, 0] = b[300, 3] = np.nan
    ref, = _check(cuda, _rows(b, s)[None], max_out=0, form=LDS)
    k = ref["seeds"].tolist()
    assert all(ref["votes"][k.index(r)] == 1 for r in (5, 77, 300))


@pytest.mark.gpu
def test_row_stride_larger_than_the_columns(cuda):
    """The C entry point on rows of 15 columns inside rows of 19 floats, B = 2,
    without owner (NULL): the outputs are compact [B, N, 15]."""
    from jabd_amd import ops
    from jabd_amd._lib import call
    B, N, C, S = 2, 700, 15, 19
    wide = np.random.default_rng(4).uniform(0, 1, (B, N, S)).astype(np.float32)
    for i in range(B):
        b, s = _clustered(N, seed=60 + i)
        wide[i, :, :4], wide[i, :, 4] = b, s
    t = torch.from_numpy(wide).to(cuda)
    out = torch.full((B, N, C), -7.0, device=cuda)
    n_out = torch.empty(B, dtype=torch.int64, device=cuda)
    seed = torch.empty((B, N), dtype=torch.int64, device=cuda)
    votes = torch.empty((B, N), dtype=torch.int32, device=cuda)
    call("jabd_box_vote_f32", ops._p(t), S, N * S, C, None, B, N, 0.4, 1.0, -math.inf, 1, 0,
         ops._p(out), ops._p(n_out), ops._p(seed), ops._p(votes), None, None, 0, ops._stream())
    assert np.array_equal(t.cpu().numpy(), wide)
    for i in range(B):
        ref = V.vote(wide[i, :, :C])
        k = int(n_out[i])
        assert k == len(ref["seeds"]) and seed[i, :k].cpu().tolist() == ref["seeds"].tolist()
        assert votes[i, :k].cpu().tolist() == ref["votes"].tolist()
        got = out[i].cpu().numpy()
        assert got[:k, 4:].tobytes() == ref["rows"][:, 4:].tobytes()
        assert int(V.ulp_diff(got[:k, :4], ref["rows"][:, :4]).max()) <= 1
        assert (got[k:] == -7.0).all()                    # nothing written past the result


@pytest.mark.gpu
def test_empty_inputs_and_bbox_vote(cuda):
    from jabd_amd import ops
    from utils import utils_bbox
    out, n_out, seed, votes = ops.box_vote(torch.zeros(3, 0, 5, device=cuda))
    assert out.shape == (3, 0, 5) and n_out.cpu().tolist() == [0, 0, 0]
    out, n_out, seed, votes = ops.box_vote(torch.zeros(0, 4, 5, device=cuda))
    assert n_out.shape == (0,)
    b, s = _clustered(300, seed=2)
    det = _rows(b, s, cols=15)
    ref = V.vote(det, thresh=0.5, min_votes=2, max_out=20)
    for arg in (det, torch.from_numpy(det).to(cuda)):
        got = utils_bbox.bbox_vote(arg, thresh=0.5, min_votes=2, max_out=20)
        assert got.shape == ref["rows"].shape and got[:, 4:].tobytes() == ref["rows"][:, 4:].tobytes()
        assert int(V.ulp_diff(got[:, :4], ref["rows"][:, :4]).max()) <= 1
    assert utils_bbox.bbox_vote(det, min_votes=1000) == []
