"""jabd_letterbox_batch_u8 through ops.letterbox_batch: images of different
sizes letterboxed into one [n, 3, h, w] batch, against the numpy restatement
of tests/_batch_ref.py (oracle/prep_ref.py per image) and against
ops.letterbox on the same image as float32, bytes equal: the uint8 -> float32
conversion is exact and the arithmetic is the same, so nothing is tolerated.
ops.pack_images is host only and tested without a GPU."""
import numpy as np
import pytest
import torch

import _batch_ref as R

MEAN = (104.0, 117.0, 123.0)
CANVAS = (64, 96)                                               # (h, w)
# (ih, iw) in pool order, with (nw, nh, top, left) on the 64 x 96 canvas
MAIN = [((100, 41), (26, 64, 0, 35)),      # both image edges inside a four-pixel group
        ((1, 1), (64, 64, 0, 16)),         # every tap clamped; later offsets are 3 mod 4
        ((37, 100), (96, 35, 14, 0)),      # bars above and below
        ((128, 192), (96, 64, 0, 0)),      # exact 2x: the INTER_AREA path
        ((32, 48), (96, 64, 0, 0)),        # 2x up-scale
        ((500, 333), (42, 64, 0, 27)),     # down-scale beyond 2x
        ((64, 96), (96, 64, 0, 0)),        # identity
        ((0, 0), None)]                    # empty slot


def _image(i, ih, iw):
    return np.random.default_rng(i + 1).integers(0, 256, (ih, iw, 3)).astype(np.uint8)


def _images(sizes):
    return [_image(i, ih, iw) if ih > 0 and iw > 0 else None for i, (ih, iw) in enumerate(sizes)]


def _pack(images):
    """(pool, desc) numpy for a list with None for an empty slot (0 x 0, its
    offset where the next image starts)."""
    from jabd_amd import ops
    pool, table = ops.pack_images([im for im in images if im is not None])
    table = table.numpy()
    desc, k = np.zeros((len(images), 3), np.int64), 0
    for i, im in enumerate(images):
        if im is None:
            desc[i] = (table[k, 0] if k < len(table) else pool.numel(), 0, 0)
        else:
            desc[i], k = table[k], k + 1
    return pool.numpy().copy(), desc


def _run(cuda, images, canvas, pool_bytes=None, **kw):
    from jabd_amd import ops
    pool, desc = _pack(images)
    got = ops.letterbox_batch(torch.from_numpy(pool).to(cuda), torch.from_numpy(desc).to(cuda),
                              (canvas[1], canvas[0]), pool_bytes=pool_bytes, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(images), 3) + tuple(canvas)
    return got.cpu().numpy()


def _check(cuda, sizes, canvas, **kw):
    from jabd_amd import ops
    images = _images(sizes)
    got = _run(cuda, images, canvas, **kw)
    fill, mean = kw.get("fill", 84.0), kw.get("mean", MEAN)
    want = R.letterbox_batch(images, canvas, fill, mean)
    for i, im in enumerate(images):
        assert got[i].tobytes() == want[i].tobytes(), (i, sizes[i])
        if im is None:
            blank = (np.float32(fill) - np.array(mean, np.float32))[:, None, None]
            assert (got[i] == blank).all()
        else:
            one = ops.letterbox(torch.from_numpy(im).to(cuda).float(), (canvas[1], canvas[0]),
                                fill=fill, mean=mean)
            assert got[i].tobytes() == one[0].cpu().numpy().tobytes(), (i, sizes[i])
    return got


def test_the_main_case_has_the_geometry_it_is_meant_to_have():
    h, w = CANVAS
    for (ih, iw), geom in MAIN:
        if geom is None:
            assert R.is_empty(ih, iw, h, w)
            continue
        nw, nh = R.sides(ih, iw, h, w)
        assert (nw, nh, (h - nh) // 2, (w - nw) // 2) == geom, (ih, iw)
    assert R.sides(80, 100, 40, 50) == (50, 40)                  # exact 2x on the odd canvas


@pytest.mark.gpu
def test_mixed_sizes_in_one_call(cuda):
    from jabd_amd import _lib
    sizes = [s for s, _ in MAIN]
    _, desc = _pack(_images(sizes))
    assert (desc[2:7, 0] % 4 == 3).all()                         # unaligned image starts
    _lib.launch_log_reset()
    got = _check(cuda, sizes, CANVAS)
    assert _lib.launch_log()[0] == ("letterbox_batch", 4)
    # the slots differ: a swapped slot would not pass
    assert len({got[i].tobytes() for i in range(len(sizes))}) == len(sizes)


@pytest.mark.gpu
def test_a_width_that_is_no_multiple_of_four_takes_the_one_pixel_form(cuda):
    from jabd_amd import _lib
    _lib.launch_log_reset()
    _check(cuda, [(80, 100), (100, 41)], (40, 50))
    assert _lib.launch_log()[0] == ("letterbox_batch", 1)


@pytest.mark.gpu
def test_other_fill_and_mean(cuda):
    got = _check(cuda, [(100, 41), (37, 100), (0, 0), (128, 192)], CANVAS, fill=7.5,
                 mean=(1.0, 2.0, 3.0))
    assert (got[0, :, :, :35] == np.array([6.5, 5.5, 4.5], np.float32)[:, None, None]).all()


@pytest.mark.gpu
def test_no_slots_launch_nothing(cuda):
    from jabd_amd import _lib, ops
    _lib.launch_log_reset()
    got = ops.letterbox_batch(torch.empty(0, dtype=torch.uint8, device=cuda),
                              torch.empty((0, 3), dtype=torch.int64, device=cuda), (96, 64))
    assert tuple(got.shape) == (0, 3, 64, 96)
    assert _lib.launch_log() == []


@pytest.mark.gpu
def test_a_range_that_leaves_the_pool_makes_an_empty_slot(cuda):
    """pool_bytes is set below the real allocation, so the last image's range
    ends past it while every byte it names exists; a negative offset and one
    past the end name nothing and are never added to the pool pointer."""
    from jabd_amd import ops
    sizes = [(100, 41), (37, 100), (32, 48)]
    images = _images(sizes)
    whole = _run(cuda, images, CANVAS)
    pool, desc = _pack(images)
    cut = _run(cuda, images, CANVAS, pool_bytes=len(pool) - 1)
    blank = (np.float32(84) - np.array(MEAN, np.float32))[:, None, None]
    assert cut[:2].tobytes() == whole[:2].tobytes()
    assert (cut[2] == blank).all() and not (whole[2] == blank).all()
    bad = desc.copy()
    bad[0, 0], bad[1, 0] = -1, len(pool) + 1
    got = ops.letterbox_batch(torch.from_numpy(pool).to(cuda), torch.from_numpy(bad).to(cuda),
                              (96, 64)).cpu().numpy()
    assert (got[0] == blank).all() and (got[1] == blank).all()
    assert got[2].tobytes() == whole[2].tobytes()


@pytest.mark.gpu
def test_argument_errors(cuda):
    from jabd_amd import ops
    pool = torch.zeros(48, dtype=torch.uint8, device=cuda)
    desc = torch.tensor([[0, 4, 4]], dtype=torch.int64, device=cuda)
    with pytest.raises(TypeError):
        ops.letterbox_batch(pool.float(), desc, (96, 64))
    with pytest.raises(TypeError):
        ops.letterbox_batch(pool, desc.int(), (96, 64))
    with pytest.raises(ValueError):
        ops.letterbox_batch(pool.reshape(4, 12), desc, (96, 64))
    with pytest.raises(ValueError):
        ops.letterbox_batch(pool, desc[:, :2], (96, 64))
    with pytest.raises(ValueError):
        ops.letterbox_batch(pool, desc, (0, 64))
    with pytest.raises(ValueError):
        ops.letterbox_batch(pool, desc, (96, 64), pool_bytes=49)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.letterbox_batch(pool.cpu(), desc, (96, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.letterbox_batch(pool, desc.cpu(), (96, 64))
    many = torch.zeros((65536, 3), dtype=torch.int64, device=cuda)
    with pytest.raises(RuntimeError, match="65535"):
        ops.letterbox_batch(pool, many, (1, 1))


def test_pack_images_lays_the_images_back_to_back():
    from jabd_amd import ops
    images = [_image(0, 5, 7), _image(1, 1, 1), _image(2, 4, 4)[:, ::2]]   # one not contiguous
    pool, desc = ops.pack_images(images, size=(96, 64))
    assert pool.dtype == torch.uint8 and pool.dim() == 1 and pool.numel() == 105 + 3 + 24
    assert desc.dtype == torch.int64
    assert desc.tolist() == [[0, 5, 7], [105, 1, 1], [108, 4, 2]]
    p = pool.numpy()
    for im, (off, ih, iw) in zip(images, desc.tolist()):
        assert np.array_equal(p[off:off + ih * iw * 3].reshape(ih, iw, 3), im)
    assert pool.is_pinned() == desc.is_pinned() == torch.cuda.is_available()
    # whatever np.asarray turns into a uint8 [H, W, 3] array is an image
    class Wrapped:
        def __array__(self, dtype=None, copy=None):
            return images[0]
    pool, desc = ops.pack_images(iter([Wrapped()]))
    assert desc.tolist() == [[0, 5, 7]] and np.array_equal(pool.numpy(), images[0].reshape(-1))
    pool, desc = ops.pack_images([])                             # no images: an empty pool
    assert pool.numel() == 0 and tuple(desc.shape) == (0, 3)


def test_pack_images_errors():
    from jabd_amd import ops
    ok = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(TypeError, match="image 1"):
        ops.pack_images([ok, ok.astype(np.float32)])
    with pytest.raises(TypeError):
        ops.pack_images([ok.astype(np.int32)])
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8),
                np.zeros((0, 4, 3), np.uint8), np.zeros((1, 4, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            ops.pack_images([bad])
    # nh = int(3 * 0.096) = 0 on a 64 x 96 canvas
    assert R.sides(3, 1000, 64, 96)[1] == 0
    with pytest.raises(ValueError, match="image 2"):
        ops.pack_images([ok, ok, np.zeros((3, 1000, 3), np.uint8)], size=(96, 64))
    ops.pack_images([np.zeros((3, 1000, 3), np.uint8)])          # no canvas, no collapse
