"""jabd_tile_collect_f32 through ops.tile_collect: a batch of tiles' detect
rows passes the edge filter, is brought to image pixels and appended to the
merged list in tile and row order, against the numpy restatement of
tests/_tile_ref.py — bytes equal, since the arithmetic is fully specified.

Tiles are 64 x 64 on a 96 x 160 image at a corner origin (left and top on the
image boundary), an interior origin (all four sides inside) and a last-row
origin (right and bottom on the boundary).  A = 700 rows per tile: above the
256-row chunk of the rank kernel and no multiple of 64."""
import math

import numpy as np
import pytest
import torch

import _tile_ref as R

TILE, IMAGE = (64, 64), (96, 160)
ORIGINS = np.array([[0, 0], [16, 48], [32, 96]], np.int32)
# which sides filter: (left, right, top, bottom) per origin
SIDES = [(False, True, False, True), (True, True, True, True), (True, False, True, False)]
A, BORDER = 700, 2.5
SENTINEL = -77.0


def _special():
    """Rows at the filter's limits, in normalised tile coordinates: a pair per
    side, the first exactly at the limit (kept), the second one fp32 ulp past
    it (dropped where that side filters); then two NaN rows (kept)."""
    lo, hi = np.float32(BORDER / 64), np.float32((64 - BORDER) / 64)
    assert float(lo) * 64 == BORDER and float(hi) * 64 == 64 - BORDER     # exact in fp32
    base = np.array([0.3, 0.3, 0.6, 0.6], np.float32)
    rows = []
    for col, at, past in ((0, lo, np.nextafter(lo, np.float32(0))),
                          (2, hi, np.nextafter(hi, np.float32(1))),
                          (1, lo, np.nextafter(lo, np.float32(0))),
                          (3, hi, np.nextafter(hi, np.float32(1)))):
        for v in (at, past):
            b = base.copy()
            b[col] = v
            rows.append(b)
    rows.append(np.full(4, np.nan, np.float32))
    rows.append(np.array([np.nan, 0.3, 0.6, 0.6], np.float32))
    return np.asarray(rows, np.float32)


def _expected_special(sides):
    left, right, top, bottom = sides
    return [True, not left, True, not right, True, not top, True, not bottom, True, True]


def _rows(seed):
    """[3, A, 15]: random boxes all over the tile (many touch its sides), the
    special rows first in every tile and again behind the first chunk."""
    rng = np.random.default_rng(seed)
    rows = rng.random((3, A, 15)).astype(np.float32)
    c = rng.random((3, A, 2)).astype(np.float32)
    half = (rng.random((3, A, 2)) * 0.2).astype(np.float32)
    rows[:, :, 0:2] = c - half
    rows[:, :, 2:4] = c + half
    sp = _special()
    rows[:, :len(sp), :4] = sp
    rows[:, 300:300 + len(sp), :4] = sp
    rows[:, len(sp) - 2, :] = np.nan                     # the all-NaN row: score and landmarks too
    return rows


@pytest.fixture(scope="module")
def rows():
    r = _rows(11)
    r.setflags(write=False)
    return r


def _device_collect(cuda, rows, n_keep, origins, border, cap, pass_index=0, state=None,
                    n_offsets=2, start=0):
    """ops.tile_collect into a sentinel-filled store whose first cap rows are
    `merged`; returns (store, offsets) as numpy and the device pair."""
    from jabd_amd import ops
    if state is None:
        store = torch.full((cap + 8, 15), SENTINEL, device=cuda)
        offsets = torch.zeros(n_offsets, dtype=torch.int64, device=cuda)
        offsets[0] = start
        state = (store, offsets)
    store, offsets = state
    ops.tile_collect(torch.from_numpy(np.array(rows, np.float32)).to(cuda),   # a writable copy
                     torch.tensor(n_keep, dtype=torch.int64, device=cuda),
                     torch.from_numpy(np.ascontiguousarray(origins)).to(cuda), store[:cap],
                     offsets, pass_index, TILE, IMAGE, border=border)
    return store.cpu().numpy(), offsets.cpu().numpy(), state


def _oracle(rows, n_keep, origins, border, cap, pass_index=0, state=None, n_offsets=2, start=0):
    if state is None:
        store = np.full((cap + 8, 15), SENTINEL, np.float32)
        offsets = np.zeros(n_offsets, np.int64)
        offsets[0] = start
        state = (store, offsets)
    store, offsets = state
    masks = R.collect(rows, n_keep, origins, TILE, IMAGE, border, store[:cap], offsets, pass_index)
    return store, offsets, masks


def _same(got, want):
    """Bytes equal; NaNs must sit in the same places (their payload is not compared)."""
    assert got.shape == want.shape
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn)
    assert np.where(gn, np.float32(0), got).tobytes() == np.where(wn, np.float32(0), want).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n_keep", [[0, 700, 257], [10 ** 6, -4, 1]])
def test_edge_filter_and_placement_against_the_oracle(cuda, rows, n_keep):
    cap = 3 * A
    want, want_off, masks = _oracle(rows, n_keep, ORIGINS, BORDER, cap, start=5)
    # the oracle itself on the rows at the limits: exactly at the limit kept, one
    # ulp past it dropped, but kept on a side that lies on the image boundary
    clamped = [max(0, min(k, A)) for k in n_keep]
    assert [len(m) for m in masks] == clamped
    for t, m in enumerate(masks):
        exp = _expected_special(SIDES[t])
        assert m[:10].tolist() == exp[:len(m[:10])], t
        if len(m) >= 310:
            assert m[300:310].tolist() == exp, t
    survivors = sum(int(m.sum()) for m in masks)
    assert want_off.tolist() == [5, 5 + survivors]
    assert any(0 < m.sum() < len(m) for m in masks)              # some dropped, some kept
    got, got_off, _ = _device_collect(cuda, rows, n_keep, ORIGINS, BORDER, cap, start=5)
    assert got_off.tolist() == want_off.tolist()
    _same(got, want)
    assert (got[:5] == SENTINEL).all() and (got[5 + survivors:] == SENTINEL).all()
    again, again_off, _ = _device_collect(cuda, rows, n_keep, ORIGINS, BORDER, cap, start=5)
    assert again.tobytes() == got.tobytes() and again_off.tolist() == got_off.tolist()


@pytest.mark.gpu
def test_minus_infinity_keeps_every_row(cuda, rows):
    n_keep = [700, 257, 700]
    got, off, _ = _device_collect(cuda, rows, n_keep, ORIGINS, -math.inf, 3 * A)
    want, want_off, masks = _oracle(rows, n_keep, ORIGINS, -math.inf, 3 * A)
    assert all(m.all() for m in masks) and want_off.tolist() == [0, sum(n_keep)]
    assert off.tolist() == want_off.tolist()
    _same(got, want)


@pytest.mark.gpu
def test_origin_zero_gives_the_bits_of_correct_boxes(cuda, rows):
    from jabd_amd import ops
    src = np.ascontiguousarray(rows[1, 20:300])                   # no NaN rows among them
    three = np.stack([src, src, src])
    got, off, _ = _device_collect(cuda, three, [len(src), 0, 0], np.zeros((1, 2), np.int32),
                                  -math.inf, len(src))
    want = ops.correct_boxes(torch.from_numpy(src.copy()).to(cuda), TILE, TILE, letterbox=False,
                             to_pixels=True).cpu().numpy()
    assert off.tolist() == [0, len(src)]
    assert got[:len(src)].tobytes() == want.tobytes()


@pytest.mark.gpu
def test_two_chained_passes(cuda, rows):
    other = _rows(12)
    cap = 6 * A
    want, want_off, state = None, None, None
    dev_state = None
    for p, (r, nk) in enumerate(((rows, [0, 700, 257]), (other, [10 ** 6, -4, 1]))):
        want, want_off, _ = _oracle(r, nk, ORIGINS, BORDER, cap, p, state, n_offsets=3)
        state = (want, want_off)
        got, got_off, dev_state = _device_collect(cuda, r, nk, ORIGINS, BORDER, cap, p, dev_state,
                                                  n_offsets=3)
    assert 0 < want_off[1] < want_off[2] < cap
    assert got_off.tolist() == want_off.tolist()
    _same(got, want)


@pytest.mark.gpu
def test_capacity_cuts_in_the_middle_of_a_tile(cuda, rows):
    n_keep = [0, 700, 257]
    _, full_off, masks = _oracle(rows, n_keep, ORIGINS, BORDER, 3 * A)
    s1, s2 = int(masks[1].sum()), int(masks[2].sum())
    assert s1 > 300 and s2 > 10
    for cap in (300, s1 + 10):                         # inside tile 1's rows, inside tile 2's
        want, want_off, _ = _oracle(rows, n_keep, ORIGINS, BORDER, cap)
        got, got_off, _ = _device_collect(cuda, rows, n_keep, ORIGINS, BORDER, cap)
        assert want_off.tolist() == [0, cap] and got_off.tolist() == [0, cap]
        _same(got, want)
        assert (got[cap:] == SENTINEL).all()           # nothing lands beyond the capacity


@pytest.mark.gpu
def test_fewer_tiles_than_slots_and_an_empty_pass(cuda, rows):
    n_keep = [700, 700, 700]
    want, want_off, _ = _oracle(rows, n_keep, ORIGINS[:2], BORDER, 3 * A, start=3)
    got, got_off, _ = _device_collect(cuda, rows, n_keep, ORIGINS[:2], BORDER, 3 * A, start=3)
    assert got_off.tolist() == want_off.tolist()
    _same(got, want)
    got, got_off, _ = _device_collect(cuda, rows, n_keep, ORIGINS[:0], BORDER, 3 * A, start=3)
    assert got_off.tolist() == [3, 3] and (got == SENTINEL).all()


@pytest.mark.gpu
def test_argument_errors(cuda):
    from jabd_amd import ops
    rows = torch.zeros((2, 8, 15), device=cuda)
    n_keep = torch.zeros(2, dtype=torch.int64, device=cuda)
    org = torch.zeros((2, 2), dtype=torch.int32, device=cuda)
    merged = torch.zeros((16, 15), device=cuda)
    offsets = torch.zeros(2, dtype=torch.int64, device=cuda)
    ops.tile_collect(rows, n_keep, org, merged, offsets, 0, TILE, IMAGE)
    with pytest.raises(ValueError):
        ops.tile_collect(rows[0], n_keep, org, merged, offsets, 0, TILE, IMAGE)
    with pytest.raises(ValueError):
        ops.tile_collect(rows, n_keep, torch.zeros((3, 2), dtype=torch.int32, device=cuda),
                         merged, offsets, 0, TILE, IMAGE)
    with pytest.raises(ValueError):
        ops.tile_collect(rows, n_keep, org, merged, offsets, 1, TILE, IMAGE)
    with pytest.raises(ValueError):
        ops.tile_collect(rows, n_keep, org, merged[:, :14], offsets, 0, TILE, IMAGE)
    with pytest.raises(ValueError):
        ops.tile_collect(rows, n_keep, org, merged, offsets, 0, TILE, IMAGE, border=math.nan)
    with pytest.raises(TypeError):
        ops.tile_collect(rows, n_keep.int(), org, merged, offsets, 0, TILE, IMAGE)
