"""jabd_batch_collect_f32 through ops.batch_collect: a letterboxed batch's
detect rows brought to each image's own pixels and packed, against
tests/_batch_ref.collect (oracle/prep_ref.correct_rows per slot), bytes equal:
the per-image terms and every row's arithmetic are the float64 expressions of
the numpy restatement, each rounded once, and the score column is a copy."""
import numpy as np
import pytest
import torch

import _batch_ref as R

A = 20
INPUT = (64, 96)
SIZES = [(100, 41), (37, 100), (64, 96), (1, 1), (0, 0), (500, 333)]
N_KEEP = [0, 20, 25, -3, 9, 7]
SENTINEL = np.float32(-777.25)
NEG_ZERO, NAN_PAYLOAD = 0x80000000, 0x7fc12345


def _inputs():
    rng = np.random.default_rng(5)
    rows = rng.uniform(-0.2, 1.2, (len(SIZES), A, 15)).astype(np.float32)
    bits = rows.view(np.uint32)
    bits[1, 3, 4] = NEG_ZERO
    bits[2, 1, 4] = NAN_PAYLOAD
    rows[1, 2, 6] = np.nan                                       # a coordinate
    return rows, np.array(N_KEEP, np.int64)


def _desc(sizes):
    d, off = np.zeros((len(sizes), 3), np.int64), 0
    for i, (ih, iw) in enumerate(sizes):
        d[i] = (off, ih, iw)
        off += ih * iw * 3
    return d


def _run(cuda, rows, n_keep, sizes, max_det, cap):
    from jabd_amd import ops
    out = torch.full((cap, 15), float(SENTINEL), dtype=torch.float32, device=cuda)
    got, offsets = ops.batch_collect(torch.from_numpy(rows).to(cuda),
                                     torch.from_numpy(n_keep).to(cuda),
                                     torch.from_numpy(_desc(sizes)).to(cuda), INPUT,
                                     max_det=max_det, out=out)
    assert got is out and offsets.dtype == torch.int64
    assert tuple(offsets.shape) == (len(sizes) + 1,)
    return out.cpu().numpy(), offsets.cpu().numpy()


def _check(cuda, max_det, cap, sizes=SIZES):
    rows, n_keep = _inputs()
    got, offsets = _run(cuda, rows, n_keep, sizes, max_det, cap)
    want, want_offsets = R.collect(rows, n_keep, sizes, INPUT, max_det, cap)
    assert offsets.tolist() == want_offsets.tolist()
    n = int(offsets[-1])
    assert n == len(want)
    assert got[:n].tobytes() == want.tobytes()
    assert (got[n:] == SENTINEL).all()                           # rows beyond stay untouched
    return got, offsets.tolist()


@pytest.mark.gpu
def test_every_kept_row_of_every_slot(cuda):
    from jabd_amd import _lib
    _lib.launch_log_reset()
    got, offsets = _check(cuda, 0, len(SIZES) * A + 3)
    assert _lib.launch_log() == [("batch_collect", 0)]           # one launch
    # counts: clamped to [0, A]; nothing from the empty slot
    assert offsets == [0, 0, 20, 40, 40, 40, 47]
    bits = got.view(np.uint32)
    assert bits[3, 4] == NEG_ZERO and bits[20 + 1, 4] == NAN_PAYLOAD   # the score is a bit copy
    assert np.isnan(got[2, 6]) and np.isfinite(got[2, [5, 7]]).all()
    # the slots were corrected with their own sizes: image pixels beyond the canvas
    assert np.nanmax(got[40:47, :4]) > 96


@pytest.mark.gpu
def test_max_det_cuts_every_slot(cuda):
    _, offsets = _check(cuda, 5, 64)
    assert np.diff(offsets).tolist() == [0, 5, 5, 0, 0, 5]


@pytest.mark.gpu
def test_the_capacity_cuts_the_last_slot(cuda):
    _, offsets = _check(cuda, 5, 12)
    assert offsets == [0, 0, 5, 10, 10, 10, 12]


@pytest.mark.gpu
def test_fewer_table_rows_than_slots_read_only_those(cuda):
    _, offsets = _check(cuda, 0, 64, sizes=SIZES[:3])
    assert offsets == [0, 0, 20, 40]


@pytest.mark.gpu
def test_no_slots_write_only_the_first_offset(cuda):
    from jabd_amd import ops
    rows, n_keep = _inputs()
    out = torch.full((8, 15), float(SENTINEL), dtype=torch.float32, device=cuda)
    offsets = torch.full((3,), -5, dtype=torch.int64, device=cuda)
    ops.batch_collect(torch.from_numpy(rows).to(cuda), torch.from_numpy(n_keep).to(cuda),
                      torch.empty((0, 3), dtype=torch.int64, device=cuda), INPUT, out=out,
                      offsets=offsets)
    assert offsets.cpu().tolist() == [0, -5, -5]
    assert (out.cpu().numpy() == SENTINEL).all()


@pytest.mark.gpu
def test_two_runs_give_identical_bytes_and_defaults_allocate(cuda):
    from jabd_amd import ops
    rows, n_keep = _inputs()
    a = _run(cuda, rows, n_keep, SIZES, 0, 128)
    b = _run(cuda, rows, n_keep, SIZES, 0, 128)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    out, offsets = ops.batch_collect(torch.from_numpy(rows).to(cuda),
                                     torch.from_numpy(n_keep).to(cuda),
                                     torch.from_numpy(_desc(SIZES)).to(cuda), INPUT)
    assert tuple(out.shape) == (len(SIZES) * A, 15)
    n = int(a[1][-1])
    assert out[:n].cpu().numpy().tobytes() == a[0][:n].tobytes()
    assert offsets.cpu().numpy().tobytes() == a[1].tobytes()


@pytest.mark.gpu
def test_argument_errors(cuda):
    from jabd_amd import ops
    rows = torch.zeros((2, A, 15), device=cuda)
    nk = torch.zeros(2, dtype=torch.int64, device=cuda)
    desc = torch.tensor([[0, 4, 4], [48, 4, 4]], dtype=torch.int64, device=cuda)
    with pytest.raises(TypeError):
        ops.batch_collect(rows.double(), nk, desc, INPUT)
    with pytest.raises(TypeError):
        ops.batch_collect(rows, nk.int(), desc, INPUT)
    with pytest.raises(TypeError):
        ops.batch_collect(rows, nk, desc.int(), INPUT)
    with pytest.raises(ValueError):
        ops.batch_collect(rows[:, :, :14], nk, desc, INPUT)
    with pytest.raises(ValueError):
        ops.batch_collect(rows, nk, desc[:, :2], INPUT)
    with pytest.raises(ValueError):
        ops.batch_collect(rows[:1], nk, desc, INPUT)             # more table rows than slots
    with pytest.raises(ValueError):
        ops.batch_collect(rows, nk[:1], desc, INPUT)
    with pytest.raises(ValueError):
        ops.batch_collect(rows, nk, desc, (0, 96))
    with pytest.raises(ValueError):
        ops.batch_collect(rows, nk, desc, INPUT, out=torch.zeros((4, 14), device=cuda))
    with pytest.raises(ValueError):
        ops.batch_collect(rows, nk, desc, INPUT, out=torch.zeros((4, 15)))
    with pytest.raises(ValueError):
        ops.batch_collect(rows, nk, desc, INPUT, offsets=nk)     # needs n + 1 entries
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.batch_collect(rows.cpu(), nk, desc, INPUT)
