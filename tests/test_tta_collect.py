"""jabd_tta_collect_f32 through ops.tta_collect: a pass's detect rows are
un-mirrored, corrected as ops.correct_boxes corrects them and appended to the
merged rows, bit for bit; the offsets chain; the surplus beyond the capacity
is dropped."""
import numpy as np
import pytest
import torch

import _vote_ref as V

SHAPES = [((96, 128), (75, 133)), ((64, 64), (64, 64)), ((160, 96), (301, 97))]


def _pass_rows(n, seed):
    """Normalised detect rows: boxes and landmarks in (0, 1), a score."""
    return np.random.default_rng(seed).uniform(0.05, 0.95, (n, 15)).astype(np.float32)


def _collect(cuda, rows, k, cap, flip, input_shape, image_shape, letterbox=True):
    from jabd_amd import ops
    merged = torch.full((cap, 15), -5.0, device=cuda)
    offsets = torch.tensor([0, -9], dtype=torch.int64, device=cuda)
    ops.tta_collect(torch.from_numpy(rows).to(cuda), torch.tensor([k], device=cuda), merged,
                    offsets, 0, input_shape, image_shape, letterbox=letterbox, flip=flip)
    return merged.cpu().numpy(), offsets.cpu().tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("input_shape,image_shape", SHAPES)
def test_rows_equal_unmirror_then_correct_boxes(cuda, flip, input_shape, image_shape):
    from jabd_amd import ops
    n, k = 300, 257                       # more than one workgroup, a ragged last one
    rows = _pass_rows(n, seed=1)
    for letterbox in (True, False):
        got, offsets = _collect(cuda, rows, k, n, flip, input_shape, image_shape, letterbox)
        src = V.unmirror(rows) if flip else rows.copy()
        want = ops.correct_boxes(torch.from_numpy(src).to(cuda), input_shape, image_shape,
                                 letterbox=letterbox, to_pixels=True).cpu().numpy()
        assert offsets == [0, k]
        assert got[:k].tobytes() == want[:k].tobytes()
        assert (got[k:] == -5.0).all()    # rows past n_keep are not collected
    if flip:                              # the un-mirror did something: eyes exchanged
        plain, _ = _collect(cuda, rows, k, n, False, input_shape, image_shape, letterbox)
        assert not np.array_equal(plain[:k], got[:k])
        assert np.array_equal(plain[:k, 6], got[:k, 8])     # the y of eye 0 is eye 1's now


@pytest.mark.gpu
def test_offsets_chain_over_three_passes_one_of_them_empty(cuda):
    from jabd_amd import ops
    inp, img = (96, 128), (75, 133)
    passes = [(_pass_rows(40, 2), 33, False), (_pass_rows(25, 3), 0, True),
              (_pass_rows(60, 4), 60, True)]
    merged = torch.full((200, 15), -5.0, device=cuda)
    offsets = torch.zeros(4, dtype=torch.int64, device=cuda)
    want = []
    for p, (rows, k, flip) in enumerate(passes):
        ops.tta_collect(torch.from_numpy(rows).to(cuda), torch.tensor([k], device=cuda), merged,
                        offsets, p, inp, img, flip=flip)
        src = V.unmirror(rows) if flip else rows.copy()
        want.append(ops.correct_boxes(torch.from_numpy(src).to(cuda), inp, img).cpu().numpy()[:k])
    want = np.concatenate(want)
    assert offsets.cpu().tolist() == [0, 33, 33, 93]
    got = merged.cpu().numpy()
    assert got[:93].tobytes() == want.tobytes() and (got[93:] == -5.0).all()
    # a caller's non-zero offsets[0] is where the first pass starts
    offsets2 = torch.tensor([7, 0], dtype=torch.int64, device=cuda)
    merged2 = torch.full((50, 15), -5.0, device=cuda)
    ops.tta_collect(torch.from_numpy(passes[0][0]).to(cuda), torch.tensor([33], device=cuda),
                    merged2, offsets2, 0, inp, img)
    assert offsets2.cpu().tolist() == [7, 40]
    assert merged2.cpu().numpy()[7:40].tobytes() == want[:33].tobytes()
    assert (merged2[:7] == -5.0).all() and (merged2[40:] == -5.0).all()


@pytest.mark.gpu
def test_surplus_beyond_the_capacity_is_dropped(cuda):
    from jabd_amd import ops
    inp, img = (64, 64), (64, 64)
    a, b, c = _pass_rows(30, 5), _pass_rows(30, 6), _pass_rows(30, 7)
    # a guard row behind the capacity: the kernel is told 45 rows
    store = torch.full((46, 15), -5.0, device=cuda)
    merged = store[:45]
    offsets = torch.zeros(4, dtype=torch.int64, device=cuda)
    for p, rows in enumerate((a, b, c)):
        ops.tta_collect(torch.from_numpy(rows).to(cuda), torch.tensor([30], device=cuda), merged,
                        offsets, p, inp, img)
    assert offsets.cpu().tolist() == [0, 30, 45, 45]
    want = np.concatenate([ops.correct_boxes(torch.from_numpy(r.copy()).to(cuda), inp, img)
                           .cpu().numpy() for r in (a, b)])[:45]
    assert merged.cpu().numpy().tobytes() == want.tobytes()
    assert (store[45] == -5.0).all()
    # n_keep beyond the pass's own rows is clamped to them
    offsets = torch.zeros(2, dtype=torch.int64, device=cuda)
    ops.tta_collect(torch.from_numpy(a).to(cuda), torch.tensor([10 ** 6], device=cuda), store,
                    offsets, 0, inp, img)
    assert offsets.cpu().tolist() == [0, 30]
